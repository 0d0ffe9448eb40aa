"""Constrained beam search timing on one GPU at the generation benchmark's shape (bench.py cfg5: GMM prior, 128 images, gen_z_samples 10,
V = 10 000, max_len 30, default model sizes), beside the group beam search of the same rows:
  calls  : ms per batch of constrained_beam_search(2 constraints of 2 words per image, beam_size 4: 4 states x 4 beams) and of
           diverse_beam_search(groups=4, group_size=4) -- 2048 rows each, both with the two-call softmax + top-k (8 and 16 words a row).
           Host clock around a synchronised call, after warm-up, the two alternating; the median of --reps calls.
  kernels: us per round of vc_beam_update_constrained(C 2, Wc 2, w 4, 8 listed words per row) and of vc_beam_update_groups(4 x 4, 16
           candidates per row) alone, on full heaps (rows of random probabilities over a 50-word vocabulary without <EOS>: every bank
           keeps its beams).  Device events around a hipGraph replay of 20 rounds, after vc_beam_init and 4 rounds that fill the heaps;
           the two alternating; the median of --reps such runs.
Prints one JSON line per part.
    python tools/experiments/cbs_time.py [--reps 9] [--part calls kernels]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi, spec, synth  # noqa: E402
from vae_captioning_amd.abi import ptr as P  # noqa: E402
from vae_captioning_amd.engine import CaptionEngine  # noqa: E402
from vae_captioning_amd.generate import CaptionGenerator  # noqa: E402
from vae_captioning_amd.utils.parameters import Parameters  # noqa: E402

V, B, C, WC, W, G = 10000, 128, 2, 2, 4, 4


def time_calls(lib, reps):
    p = Parameters()
    p.mode, p.num_captions, p.prior, p.gen_z_samples = "inference", 1, "GMM", 10
    rng = np.random.default_rng(0)
    eng = CaptionEngine(p, V, lib=lib, seed=0)
    eng.load_params(spec.init_caption_params(p, V, seed=1))
    gen = CaptionGenerator(eng)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, p.cnn_feature_size), dtype=np.float32), 0)).cuda()
    cv = np.zeros((B, 90), np.float32)
    eps = rng.standard_normal((p.gen_z_samples, B, p.latent_size), dtype=np.float32)
    cons = [rng.choice(np.arange(3, V), C * WC, replace=False).reshape(C, WC).tolist() for _ in range(B)]
    group = lambda: gen.diverse_beam_search(feats, cv, eps, synth.BOS, synth.EOS, groups=G, group_size=W, diversity=0.5, max_len=p.gen_max_len)
    forced = lambda: gen.constrained_beam_search(feats, cons, cv, eps, synth.BOS, synth.EOS, beam_size=W, max_len=p.gen_max_len)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(3):
        group()
        forced()
    t_group, t_forced = [], []
    for _ in range(reps):
        ms, _ = clock(group)
        t_group.append(ms)
        ms, res = clock(forced)
        t_forced.append(ms)
    met = float(np.mean([bin(state).count("1") for _, state in res]))
    print(json.dumps({"part": "calls", "images": B, "rows": B * (1 << C) * W, "vocab": V, "max_len": p.gen_max_len, "reps": reps,
                      "diverse_beam_search_4x4_ms": round(float(np.median(t_group)), 3),
                      "constrained_beam_search_C2_w4_ms": round(float(np.median(t_forced)), 3),
                      "diverse_beam_search_4x4_ms_min_max": [round(min(t_group), 3), round(max(t_group), 3)],
                      "constrained_beam_search_C2_w4_ms_min_max": [round(min(t_forced), 3), round(max(t_forced), 3)],
                      "constraints_met_per_image": round(met, 2), "captured_graphs": len(gen._graphs),
                      "clock": "host perf_counter around a synchronised call, median"}))


def time_kernels(lib, reps):
    S, L, H, fill, timed, Vk = 1 << C, 32, 8, 4, 20, 50   # (captions grow one token a round: 1 + fill + timed < L)
    w, Bv, kc_c, kc_g = W, B * (1 << C), W + C * WC, G * W
    M = Bv * w
    st = lambda: torch.cuda.current_stream().cuda_stream
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(1)
    probs_h = rng.uniform(1e-4, 0.3, size=(M, Vk)).astype(np.float32)
    probs_h[:, :3] = 0.0   # no <PAD> / <BOS> / <EOS>: every row keeps its beams
    order = np.argsort(-probs_h, axis=1, kind="stable")
    probs = torch.from_numpy(probs_h).cuda()
    ti = {k: torch.from_numpy(order[:, :k].astype(np.int32).copy()).cuda() for k in (kc_c, kc_g)}
    tv = {k: torch.from_numpy(np.take_along_axis(probs_h, order[:, :k], axis=1).copy()).cuda() for k in (kc_c, kc_g)}
    cons = torch.from_numpy(np.stack([rng.choice(np.arange(3, Vk), C * WC, replace=False).reshape(C, WC) for _ in range(B)]).astype(np.int32)).cuda()
    c_in, c_out = torch.zeros(Bv, H, device="cuda"), torch.zeros(M, H, device="cuda")
    runs = {}
    for name in ("vc_beam_update_groups_4x4", "vc_beam_update_constrained_C2_w4"):
        pcount, ccount, c_free = i32(Bv), i32(Bv), i32(Bv)
        p_score, p_logprob, p_len = f64(M), f64(M), i32(M)
        sent = [i32(M, L), i32(M, L)]
        c_score, c_logprob, c_len, c_slot, c_sent = f64(M), f64(M), i32(M), i32(M), i32(Bv * (w + 1), L)
        parent, tok = i32(M), i32(M)

        def state(it, b=(pcount, ccount, p_score, p_logprob, p_len, sent, c_score, c_logprob, c_len, c_slot, c_free, c_sent, parent, tok)):
            return (P(b[0]), P(b[1]), P(b[2]), P(b[3]), P(b[4]), P(b[5][it & 1]), P(b[5][1 - (it & 1)]), P(b[6]), P(b[7]), P(b[8]), P(b[9]), P(b[10]),
                    P(b[11]), P(b[12]), P(b[13]))

        def round_(it, name=name, state=state):
            if name.endswith("4x4"):
                lib.vc_beam_update_groups(st(), B, G, w, kc_g, L, synth.EOS, 0.7, 0.5, P(tv[kc_g]), P(ti[kc_g]), *state(it))
            else:
                lib.vc_beam_update_constrained(st(), B, C, WC, w, kc_c, L, synth.EOS, 0.7, P(cons), P(tv[kc_c]), P(ti[kc_c]), P(probs), Vk, Vk, *state(it))

        def start(name=name, state=state, round_=round_, pcount=pcount):
            lib.vc_beam_init(st(), Bv, w, L, synth.BOS, H, P(c_in), P(c_in), P(c_out), P(c_out), *state(0))
            if not name.endswith("4x4"):
                pcount.view(B, S)[:, 1:] = 0
            for it in range(fill):
                round_(it)

        def rounds(round_=round_):
            for it in range(fill, fill + timed):
                round_(it)

        start()
        rounds()   # (eager once: code objects loaded before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rounds()
        runs[name] = (start, graph, pcount, [])
    for rep in range(reps + 1):   # (the first run of each is the warm-up; the two alternate)
        for name, (start, graph, pcount, us) in runs.items():
            start()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                us.append(e0.elapsed_time(e1) * 1e3 / timed)
            assert int(pcount.min()) == w, "the timed rounds must run on full heaps"
    out = {}
    for name, (_, _, _, us) in runs.items():
        out[name + "_us"] = round(float(np.median(us)), 2)
        out[name + "_us_min_max"] = [round(min(us), 2), round(max(us), 2)]
    out.update(part="kernels", images=B, rows=M, reps=reps, rounds_per_run=timed,
               clock="device events around one hipGraph replay of 20 rounds (a chain of launches, their gaps included), median of the runs")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--part", nargs="+", default=["calls", "kernels"], choices=["calls", "kernels"])
    a = ap.parse_args()
    lib = abi.load()
    lib.vc_device_check(0)
    if "calls" in a.part:
        time_calls(lib, a.reps)
    if "kernels" in a.part:
        time_kernels(lib, a.reps)


if __name__ == "__main__":
    main()
