"""Stochastic beam search timing on one GPU at the generation benchmark's model (bench.py cfg5: GMM prior, gen_z_samples 10, V = 10 000,
default model sizes), beside the plain beam search of the same width:
  calls  : ms per batch of stochastic_beam_search(beam_size=10) and of beam_search(beam_size=10), at 32 images (320 rows) and 128
           images (1280 rows).  Host clock around a synchronised call, after warm-up, the two alternating; the median of --reps calls.
  kernels: us per launch, at 320 and 1280 rows x 10 000 columns, of vc_sbs_expand_f32 (kc = 11, Philox noise) beside the round's
           logits product (rows x 10 000 x 512) and beam search's softmax + top-10 of the same rows, and of vc_sbs_update beside
           vc_beam_update (beam 10, full beams).  Device events around a hipGraph replay of 20 launches, the median of --reps runs.
Prints one JSON line per part.
    python tools/experiments/sbs_time.py [--reps 9] [--part calls kernels]"""
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

V, N, H = 10000, 10, 512
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
    out = {"part": "calls", "beam": N, "vocab": V, "max_len": p.gen_max_len, "reps": reps,
           "clock": "host perf_counter around a synchronised call, median"}
    for B in (32, 128):
        rng = np.random.default_rng(0)
        feats = torch.from_numpy(np.maximum(rng.standard_normal((B, p.cnn_feature_size), dtype=np.float32), 0)).cuda()
        cv = np.zeros((B, 90), np.float32)
        eps = rng.standard_normal((p.gen_z_samples, B, p.latent_size), dtype=np.float32)
        plain = lambda: gen.beam_search(feats, cv, eps, synth.BOS, synth.EOS, beam_size=N, max_len=p.gen_max_len)
        sbs = lambda: gen.stochastic_beam_search(feats, cv, eps, synth.BOS, synth.EOS, beam_size=N, max_len=p.gen_max_len)

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res

        for _ in range(3):
            plain()
            sbs()
        t_plain, t_sbs = [], []
        for _ in range(reps):
            t_plain.append(clock(plain)[0])
            ms, res = clock(sbs)
            t_sbs.append(ms)
        out["images_%d" % B] = {"rows": B * N, "beam_search_ms": round(float(np.median(t_plain)), 3),
                                "stochastic_beam_search_ms": round(float(np.median(t_sbs)), 3),
                                "beam_search_ms_min_max": [round(min(t_plain), 3), round(max(t_plain), 3)],
                                "stochastic_beam_search_ms_min_max": [round(min(t_sbs), 3), round(max(t_sbs), 3)],
                                "distinct_captions_per_image": round(float(np.mean([len({tuple(c[0]) for c in r["captions"]}) for r in res])), 2),
                                "mean_caption_len": round(float(np.mean([len(c[0]) for r in res for c in r["captions"]])), 2)}
    print(json.dumps(out))


FILL, TIMED = 4, 20   # bookkeeping rounds that fill the beams, then the timed ones: sentences stay below 1 + FILL + TIMED + 1 words


def graph_us(fn, reps, start=None):
    """us per launch of fn(it), it = FILL .. FILL + TIMED - 1, as ONE hipGraph replay; start() (eager) precedes every replay"""
    launches = TIMED
    if start is not None:
        start()
    for it in range(FILL, FILL + TIMED):   # (eager once: code objects loaded before the capture)
        fn(it)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for it in range(FILL, FILL + TIMED):
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
            us.append(e0.elapsed_time(e1) * 1e3 / launches)
    return round(float(np.median(us)), 2)


def time_kernels(lib, reps):
    p, eng = engine(lib)
    S = eng.store
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    out = {"part": "kernels", "vocab": V, "beam": N, "kc": N + 1, "reps": reps,
           "clock": "device events around one hipGraph replay of 20 launches (their gaps included), median of the runs"}
    for B in (32, 128):
        M, kc, L = B * N, N + 1, 32   # (L > 1 + FILL + TIMED)
        h2 = torch.randn(M, H, device="cuda")
        logits, probs = torch.empty(M, V, device="cuda"), torch.empty(M, V, device="cuda")
        eng._need_ws(lib.vc_gemm_workspace_bytes(M, V, H))
        gemm = lambda it=0: eng.gemm(0, 0, M, V, H, h2, H, S.param("decoder/rnn_logits/kernel"), eng.Vp, logits, V, S.param("decoder/rnn_logits/bias"), tag=None)
        gemm()
        count, done = torch.full((B,), N, dtype=torch.int32, device="cuda"), i32(M)
        ck, cl, ci, rnd = f64(M, kc), torch.zeros(M, kc, device="cuda"), i32(M, kc), i32(1)
        expand = lambda it=0: lib.vc_sbs_expand_f32(st(), P(logits), M, N, V, V, P(count), P(done), kc, None, 0, P(rnd), 12345, 9 << 32, None, P(ck), P(cl), P(ci))
        tv, ti = torch.zeros(M, N, device="cuda"), i32(M, N)

        def softmax_topk(it=0):
            lib.vc_softmax_rows_f32(st(), P(logits), M, V, V, P(probs), V)
            lib.vc_topk_rows_f32(st(), P(probs), M, V, V, N, P(tv), P(ti))

        r = {"rows": M, "logits_gemm_us": graph_us(gemm, reps), "vc_sbs_expand_f32_us": graph_us(expand, reps),
             "softmax_plus_topk10_us": graph_us(softmax_topk, reps)}
        # the bookkeeping on full beams: one expansion's candidates, sentences that never end (eos = -1), the state reset by the init
        phi, G, kappa, p_len, p_done = f64(M), f64(M), f64(B), i32(M), i32(M)
        sent, parent, tok = [i32(M, L), i32(M, L)], i32(M), i32(M)
        c_in, c_out = torch.zeros(B, 8, device="cuda"), torch.zeros(M, 8, device="cuda")
        init = lambda: lib.vc_sbs_init(st(), B, N, L, synth.BOS, 8, P(c_in), P(c_in), P(c_out), P(c_out), P(count), P(phi), P(G), P(p_len), P(p_done),
                                       P(sent[0]), P(sent[1]), P(kappa), P(parent), P(tok), None)
        def update(it):
            lib.vc_sbs_update(st(), B, N, kc, L, synth.BOS, -1, P(ck), P(cl), P(ci), P(count), P(phi), P(G), P(p_len), P(p_done), P(sent[it & 1]),
                              P(sent[1 - (it & 1)]), P(kappa), P(parent), P(tok), None)

        def start():
            init()
            for it in range(FILL):
                update(it)

        r["vc_sbs_update_us"] = graph_us(update, reps, start)
        assert int(count.min()) == N and int(p_done.max()) == 0, "the timed rounds must run on full beams of live entries"
        count.fill_(N)
        pcount, ccount, c_free = i32(B), i32(B), i32(B)
        p_score, p_logprob, c_score, c_logprob, c_len, c_slot, c_sent = f64(M), f64(M), f64(M), f64(M), i32(M), i32(M), i32(B * (N + 1), L)
        sb = [i32(M, L), i32(M, L)]
        rng = np.random.default_rng(1)
        tvb = torch.from_numpy(np.sort(rng.uniform(1e-4, 0.3, size=(M, N)).astype(np.float32), axis=1)[:, ::-1].copy()).cuda()
        tib = torch.from_numpy(np.stack([rng.permutation(np.arange(3, 53))[:N] for _ in range(M)]).astype(np.int32)).cuda()
        bstate = lambda it: (P(pcount), P(ccount), P(p_score), P(p_logprob), P(p_len), P(sb[it & 1]), P(sb[1 - (it & 1)]), P(c_score), P(c_logprob),
                             P(c_len), P(c_slot), P(c_free), P(c_sent), P(parent), P(tok))
        beam_update = lambda it: lib.vc_beam_update(st(), B, N, L, synth.EOS, 0.7, P(tvb), P(tib), *bstate(it))

        def beam_start():
            lib.vc_beam_init(st(), B, N, L, synth.BOS, 8, P(c_in), P(c_in), P(c_out), P(c_out), *bstate(0))
            for it in range(FILL):
                beam_update(it)

        r["vc_beam_update_us"] = graph_us(beam_update, reps, beam_start)
        assert int(pcount.min()) == N, "the timed rounds must run on full heaps"
        out["rows_%d" % M] = r
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
