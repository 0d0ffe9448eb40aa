"""Contrastive search timing on one GPU at the generation benchmark's model (bench.py cfg5: GMM prior, gen_z_samples 10, V = 10 000,
default model sizes), 128 images, beside the beam search of the same width k (k = 5 and k = 16): both run one LSTM step over 128 * k
rows per round; the beam search's logits product, softmax and top-k run over 128 * k rows, contrastive search's over 128.
  calls  : ms per batch and per round of contrastive_search(k) and of beam_search(beam_size=k), check_every=0 (every round runs: 30 and
           29).  Host clock around a synchronised call, after warm-up, the two alternating; the median of --reps calls.
  kernels: us per launch of vc_contrastive_pick_f32 alone (128 rows, k candidates, H = 512; the history grows from 1 to 20 vectors over
           the 20 timed launches, as in a caption's first 20 rounds) and of what differs between the two rounds: the logits product and
           softmax + top-k over 128 and over 128 * k rows, and vc_beam_update.  Device events around a hipGraph replay of 20 launches,
           the median of --reps runs.
Prints one JSON line per part.
    python tools/experiments/contrastive_time.py [--reps 9] [--part calls kernels]"""
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

V, B, H, KS, TIMED = 10000, 128, 512, (5, 16), 20
st = lambda: torch.cuda.current_stream().cuda_stream


def engine(lib):
    p = Parameters()
    p.mode, p.num_captions, p.prior, p.gen_z_samples = "inference", 1, "GMM", 10
    eng = CaptionEngine(p, V, lib=lib, seed=0)
    eng.load_params(spec.init_caption_params(p, V, seed=1))
    return p, eng


def time_calls(lib, reps):
    p, eng = engine(lib)
    gen = CaptionGenerator(eng)
    L = p.gen_max_len
    out = {"part": "calls", "images": B, "vocab": V, "max_len": L, "alpha": 0.6, "reps": reps,
           "clock": "host perf_counter around a synchronised call, median"}
    rng = np.random.default_rng(0)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, p.cnn_feature_size), dtype=np.float32), 0)).cuda()
    cv = np.zeros((B, 90), np.float32)
    eps = rng.standard_normal((p.gen_z_samples, B, p.latent_size), dtype=np.float32)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    for k in KS:
        beam = lambda: gen.beam_search(feats, cv, eps, synth.BOS, synth.EOS, beam_size=k, max_len=L, check_every=0)
        cs = lambda: gen.contrastive_search(feats, cv, eps, synth.BOS, synth.EOS, k=k, alpha=0.6, max_len=L, check_every=0)
        for _ in range(3):
            beam()
            cs()
        t_beam, t_cs = [], []
        for _ in range(reps):
            t_beam.append(clock(beam)[0])
            ms, res = clock(cs)
            t_cs.append(ms)
        mb, mc = float(np.median(t_beam)), float(np.median(t_cs))
        out["k_%d" % k] = {"rows": B * k, "beam_search_ms": round(mb, 3), "contrastive_search_ms": round(mc, 3),
                           "beam_search_ms_min_max": [round(min(t_beam), 3), round(max(t_beam), 3)],
                           "contrastive_search_ms_min_max": [round(min(t_cs), 3), round(max(t_cs), 3)],
                           "beam_rounds": L - 1, "contrastive_rounds": L, "beam_ms_per_round": round(mb / (L - 1), 4),
                           "contrastive_ms_per_round": round(mc / L, 4),
                           "mean_caption_len": round(float(np.mean([len(t) for t, _ in res])), 2)}
    print(json.dumps(out))


def graph_us(fn, reps, start=None):
    """us per launch of fn(it), it = 0 .. TIMED - 1, as ONE hipGraph replay; start() (eager) precedes every replay"""
    if start is not None:
        start()
    for it in range(TIMED):   # (eager once: code objects loaded before the capture)
        fn(it)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for it in range(TIMED):
            fn(it)
    us = []
    for rep in range(reps + 1):   # (the first run is the warm-up)
        if start is not None:
            start()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            us.append(e0.elapsed_time(e1) * 1e3 / TIMED)
    return round(float(np.median(us)), 2)


def time_kernels(lib, reps):
    p, eng = engine(lib)
    S = eng.store
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    L = 32   # (> TIMED: the pick's rows never fill up)
    out = {"part": "kernels", "images": B, "vocab": V, "hidden": H, "reps": reps,
           "clock": "device events around one hipGraph replay of 20 launches (their gaps included), median of the runs"}
    rng = np.random.default_rng(1)
    for k in KS:
        M = B * k
        r = {"rows": M}
        # ---- the pick alone: every launch appends a vector, so the 20 timed launches see 1 .. 20 history vectors (eos = -1: no row ends)
        h2 = torch.randn(M, H, device="cuda")
        hist, h_sel = torch.zeros(B, L + 1, H, device="cuda"), torch.zeros(B, H, device="cuda")
        hist[:, 0] = torch.nn.functional.normalize(torch.randn(B, H, device="cuda"), dim=1)
        tv = torch.from_numpy(np.sort(rng.uniform(1e-4, 0.3, size=(B, k)).astype(np.float32), axis=1)[:, ::-1].copy()).cuda()
        ti = torch.from_numpy(np.stack([rng.permutation(np.arange(3, 53))[:k] for _ in range(B)]).astype(np.int32)).cuda()
        clen, done, seq, lp, parent = i32(B), i32(B), i32(B, L), f64(B), i32(M)
        pick = lambda it: lib.vc_contrastive_pick_f32(st(), B, k, H, L, P(h2), P(ti), P(tv), P(hist), P(clen), P(done), P(seq), P(lp), 0.6, -1, 1,
                                                      P(h_sel), P(parent), None, None)
        r["vc_contrastive_pick_f32_us"] = graph_us(pick, reps, clen.zero_)
        assert int(clen.min()) == TIMED and int(done.max()) == 0, "every timed launch must have run on every row"
        # ---- what differs between the rounds: logits, softmax + top-k over B rows (contrastive) and over B * k rows (beam search)
        for name, rows in (("contrastive", B), ("beam", M)):
            hh, logits, probs = torch.randn(rows, H, device="cuda"), torch.empty(rows, V, device="cuda"), torch.empty(rows, V, device="cuda")
            tvr, tir = torch.zeros(rows, k, device="cuda"), i32(rows, k)
            eng._need_ws(lib.vc_gemm_workspace_bytes(rows, V, H))
            gemm = lambda it=0: eng.gemm(0, 0, rows, V, H, hh, H, S.param("decoder/rnn_logits/kernel"), eng.Vp, logits, V,
                                         S.param("decoder/rnn_logits/bias"), tag=None)

            def softmax_topk(it=0):
                if k <= 8:
                    lib.vc_softmax_topk_rows_f32(st(), P(logits), rows, V, V, k, P(tvr), P(tir))
                else:
                    lib.vc_softmax_rows_f32(st(), P(logits), rows, V, V, P(probs), V)
                    lib.vc_topk_rows_f32(st(), P(probs), rows, V, V, k, P(tvr), P(tir))

            r["%s_logits_gemm_%d_rows_us" % (name, rows)] = graph_us(gemm, reps)
            r["%s_softmax_topk_%d_rows_us" % (name, rows)] = graph_us(softmax_topk, reps)
        # ---- the beam search's bookkeeping on full beams (sentences that never end: eos = -1), the state reset by the init
        Lb = TIMED + 8
        pcount, ccount, c_free, p_len, tok = i32(B), i32(B), i32(B), i32(M), i32(M)
        p_score, p_logprob, c_score, c_logprob, c_len, c_slot, c_sent = f64(M), f64(M), f64(M), f64(M), i32(M), i32(M), i32(B * (k + 1), Lb)
        sb = [i32(M, Lb), i32(M, Lb)]
        tvb = torch.from_numpy(np.sort(rng.uniform(1e-4, 0.3, size=(M, k)).astype(np.float32), axis=1)[:, ::-1].copy()).cuda()
        tib = torch.from_numpy(np.stack([rng.permutation(np.arange(3, 53))[:k] for _ in range(M)]).astype(np.int32)).cuda()
        c_in, c_out = torch.zeros(B, 8, device="cuda"), torch.zeros(M, 8, device="cuda")
        bstate = lambda it: (P(pcount), P(ccount), P(p_score), P(p_logprob), P(p_len), P(sb[it & 1]), P(sb[1 - (it & 1)]), P(c_score), P(c_logprob),
                             P(c_len), P(c_slot), P(c_free), P(c_sent), P(parent), P(tok))
        beam_update = lambda it: lib.vc_beam_update(st(), B, k, Lb, -1, 0.7, P(tvb), P(tib), *bstate(it))

        def beam_start():
            lib.vc_beam_init(st(), B, k, Lb, synth.BOS, 8, P(c_in), P(c_in), P(c_out), P(c_out), *bstate(0))
            for it in range(4):
                beam_update(it)

        r["vc_beam_update_us"] = graph_us(lambda it: beam_update(it + 4), reps, beam_start)
        assert int(pcount.min()) == k, "the timed rounds must run on full heaps"
        out["k_%d" % k] = r
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
