"""Group beam search timing on one GPU at the generation benchmark's shape (bench.py cfg5: GMM prior, 128 images, gen_z_samples 10,
V = 10 000, default model sizes), beside the plain beam search of the same rows and the same logits product:
  calls  : ms per batch of diverse_beam_search(groups=5, group_size=2) and of beam_search(beam_size=10) -- 1280 rows each.  Host clock
           around a synchronised call, after warm-up, the two alternating; the median of --reps calls.
  kernels: us per round of vc_beam_update_groups(5 x 2, 10 candidates per row) and of vc_beam_update(beam 10) alone, on full heaps
           (tables of random probabilities over a 50-word vocabulary without <EOS>: every row keeps its beams, words repeat across
           groups).  Device events around a hipGraph replay of 20 rounds, after vc_beam_init and 4 rounds that fill the heaps; the
           median of --reps such runs.  --plain-beams 5,8,9,16 adds vc_beam_update alone at those widths, the same way.
Prints one JSON line per part.
    python tools/experiments/dbs_time.py [--reps 9] [--part calls kernels] [--plain-beams 5,8,9,16] [--once]
--once: one warm call then one call of each search only (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
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

V, B, G, W, LAM = 10000, 128, 5, 2, 0.5


def time_calls(lib, reps, once):
    p = Parameters()
    p.mode, p.num_captions, p.prior, p.gen_z_samples = "inference", 1, "GMM", 10
    rng = np.random.default_rng(0)
    eng = CaptionEngine(p, V, lib=lib, seed=0)
    eng.load_params(spec.init_caption_params(p, V, seed=1))
    gen = CaptionGenerator(eng)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, p.cnn_feature_size), dtype=np.float32), 0)).cuda()
    cv = np.zeros((B, 90), np.float32)
    eps = rng.standard_normal((p.gen_z_samples, B, p.latent_size), dtype=np.float32)
    plain = lambda: gen.beam_search(feats, cv, eps, synth.BOS, synth.EOS, beam_size=G * W, max_len=p.gen_max_len)
    group = lambda: gen.diverse_beam_search(feats, cv, eps, synth.BOS, synth.EOS, groups=G, group_size=W, diversity=LAM, max_len=p.gen_max_len)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(1 if once else 3):
        plain()
        group()
    t_plain, t_group = [], []
    for _ in range(1 if once else reps):
        ms, res_p = clock(plain)
        t_plain.append(ms)
        ms, res_g = clock(group)
        t_group.append(ms)
    distinct = float(np.mean([len({tuple(s) for g in im for s, _ in g}) for im in res_g]))
    print(json.dumps({"part": "calls", "images": B, "rows": B * G * W, "vocab": V, "max_len": p.gen_max_len, "reps": len(t_plain),
                      "beam_search_10_ms": round(float(np.median(t_plain)), 3), "diverse_beam_search_5x2_ms": round(float(np.median(t_group)), 3),
                      "beam_search_10_ms_min_max": [round(min(t_plain), 3), round(max(t_plain), 3)],
                      "diverse_beam_search_5x2_ms_min_max": [round(min(t_group), 3), round(max(t_group), 3)],
                      "distinct_captions_per_image": round(distinct, 2), "mean_plain_caption_len": round(float(np.mean([len(r[0][0]) for r in res_p])), 2),
                      "clock": "host perf_counter around a synchronised call, median"}))


def time_kernels(lib, reps, plain_beams=()):
    L, H, fill, timed = 32, 8, 4, 20   # (captions grow one token a round: 1 + fill + timed < L)
    st = lambda: torch.cuda.current_stream().cuda_stream
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    out = {}
    # (name, groups, beams per group): the two searches of 10 rows per image, then vc_beam_update alone at every width asked for
    cases = [("vc_beam_update_10", 0, G * W), ("vc_beam_update_groups_5x2", G, W)] + [("vc_beam_update_plain_%d" % n, 0, n) for n in plain_beams]
    for name, groups, w in cases:
        n = max(groups, 1) * w               # rows per image = candidates per row
        M, Bv = B * n, B * max(groups, 1)
        rng = np.random.default_rng(1)
        tv = torch.from_numpy(np.sort(rng.uniform(1e-4, 0.3, size=(M, n)).astype(np.float32), axis=1)[:, ::-1].copy()).cuda()
        ti = torch.from_numpy(np.stack([rng.permutation(np.arange(3, 53))[:n] for _ in range(M)]).astype(np.int32)).cuda()
        c_in, c_out = torch.zeros(Bv, H, device="cuda"), torch.zeros(M, H, device="cuda")
        pcount, ccount, c_free = i32(Bv), i32(Bv), i32(Bv)
        p_score, p_logprob, p_len = f64(M), f64(M), i32(M)
        sent = [i32(M, L), i32(M, L)]
        c_score, c_logprob, c_len, c_slot, c_sent = f64(M), f64(M), i32(M), i32(M), i32(Bv * (w + 1), L)
        parent, tok = i32(M), i32(M)
        state = lambda it: (P(pcount), P(ccount), P(p_score), P(p_logprob), P(p_len), P(sent[it & 1]), P(sent[1 - (it & 1)]), P(c_score),
                            P(c_logprob), P(c_len), P(c_slot), P(c_free), P(c_sent), P(parent), P(tok))

        def round_(it):
            if groups:
                lib.vc_beam_update_groups(st(), B, groups, w, n, L, synth.EOS, 0.7, LAM, P(tv), P(ti), *state(it))
            else:
                lib.vc_beam_update(st(), B, n, L, synth.EOS, 0.7, P(tv), P(ti), *state(it))

        def start():
            lib.vc_beam_init(st(), Bv, w, L, synth.BOS, H, P(c_in), P(c_in), P(c_out), P(c_out), *state(0))
            for it in range(fill):
                round_(it)

        def rounds():
            for it in range(fill, fill + timed):
                round_(it)

        start()
        rounds()   # (eager once: code objects loaded before the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rounds()
        us = []
        for rep in range(reps + 1):   # (the first run is the warm-up)
            start()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                us.append(e0.elapsed_time(e1) * 1e3 / timed)
        assert int(pcount.min()) == w, "the timed rounds must run on full heaps"
        out[name + "_us"] = round(float(np.median(us)), 2)
        out[name + "_us_min_max"] = [round(min(us), 2), round(max(us), 2)]
    out.update(part="kernels", images=B, rows=B * G * W, reps=reps, rounds_per_run=timed,
               clock="device events around one hipGraph replay of 20 rounds (a chain of launches, their gaps included), median of the runs")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--part", nargs="+", default=["calls", "kernels"], choices=["calls", "kernels"])
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--plain-beams", type=lambda v: [int(x) for x in v.split(",")], default=[],
                    help="kernels part: also time vc_beam_update alone at these widths, e.g. 5,8,9,16 (the slim kernel and both edges of the general one)")
    a = ap.parse_args()
    lib = abi.load()
    lib.vc_device_check(0)
    if "calls" in a.part:
        time_calls(lib, a.reps, a.once)
    if "kernels" in a.part and not a.once:
        time_kernels(lib, a.reps, a.plain_beams)


if __name__ == "__main__":
    main()
