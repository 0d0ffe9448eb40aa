"""Typical / min-p / eta sampling timing on one GPU (DESIGN.md "Typical / min-p / eta sampling").
(a) vc_decode_pick_typical_f32 at the five settings of tests/typical_ref.py against vc_decode_pick_f32 in sampling mode and
    vc_decode_pick_trunc_f32 at top_p 0.9 on the same buffers: 640 and 4096 rows of V = 10 000 logits (N(0, 4^2)).  Each entry's
    `--launches` back-to-back launches are captured into one hipGraph (a Python launch costs more than a 640-row kernel runs); device
    events around a replay, the entries alternating inside a repetition, median over `--reps` after two warm-up repetitions;
    microseconds per launch and the mean number of words kept.
(b) diverse(method="sample", draws=20) on 32 images at full dimensions (V = 10 000, decoder_hidden 512, gen_z_samples 100, latent 150,
    Normal prior, random weights) with and without typical_p = 0.9: host clock around a synchronised call, alternating, median.
Prints one JSON line per measurement.
    python tools/experiments/typical_time.py [--rows 640 4096] [--reps 7] [--launches 50] [--skip-diverse]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi, spec  # noqa: E402
from vae_captioning_amd.engine import CaptionEngine  # noqa: E402
from vae_captioning_amd.generate import CaptionGenerator  # noqa: E402
from vae_captioning_amd.utils.parameters import Parameters  # noqa: E402

P = abi.ptr
SETTINGS = [(0.9, 0.0, 0.0, 1.0), (0.2, 0.0, 0.0, 1.0), (1.0, 0.05, 0.0, 0.8), (1.0, 0.0, 3e-3, 1.0), (0.9, 0.02, 1e-3, 0.7)]   # (tau, min_p, eta, t)


def kernel_times(lib, R, V, reps, launches):
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(R)
    x = torch.randn((R, V), device="cuda", generator=g) * 4.0
    u = torch.rand((R,), device="cuda", generator=g)
    i32 = dict(dtype=torch.int32, device="cuda")
    tok, done, seq, ln, kept = (torch.zeros(R, **i32) for _ in range(5))
    lp = torch.zeros(R, dtype=torch.float64, device="cuda")
    ent = torch.zeros(R, device="cuda")

    def plain():
        lib.vc_decode_pick_f32(st, P(x), R, V, V, 1.0, P(u), 1, None, -1, P(tok), P(done), P(seq), 1, P(ln), P(lp))

    def trunc():
        lib.vc_decode_pick_trunc_f32(st, P(x), R, V, V, 1.0, 0, 0.9, P(u), 1, None, -1, P(tok), P(done), P(seq), 1, P(ln), P(lp), P(kept))

    def typical(tau, m, eta, t):
        return lambda: lib.vc_decode_pick_typical_f32(st, P(x), R, V, V, t, tau, m, eta, P(u), 1, None, -1, P(tok), P(done), P(seq), 1, P(ln),
                                                      P(lp), P(kept), P(ent))

    fns = [("plain", plain), ("top_p 0.9", trunc)] + [("typical_p %g min_p %g eta %g t %g" % s, typical(*s)) for s in SETTINGS]
    ts, graphs, mean_kept = {name: [] for name, _ in fns}, {}, {}
    for name, fn in fns:
        fn()   # (eager once: the code object is loaded before the capture)
        torch.cuda.synchronize()
        mean_kept[name] = round(float(kept.float().mean()), 1) if name != "plain" else None
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            st = torch.cuda.current_stream().cuda_stream
            for _ in range(launches):
                fn()
    st = torch.cuda.current_stream().cuda_stream
    for rep in range(reps + 2):   # (two warm-up repetitions)
        for name, _ in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name].replay()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ts[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    base, nucleus = float(np.median(ts["plain"])), float(np.median(ts["top_p 0.9"]))
    for name, _ in fns:
        us = float(np.median(ts[name]))
        print(json.dumps({"rows": R, "V": V, "entry": name, "us_per_launch": round(us, 2), "min_us": round(min(ts[name]), 2),
                          "max_us": round(max(ts[name]), 2), "ratio_to_plain": round(us / base, 2), "ratio_to_top_p": round(us / nucleus, 2),
                          "mean_kept": mean_kept[name]}), flush=True)


def diverse_times(lib, reps):
    p = Parameters()
    p.mode, p.num_captions, p.prior = "inference", 1, "Normal"
    V, B, K = 10000, 32, 20
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(spec.init_caption_params(p, V, seed=3))
    gen = CaptionGenerator(eng)
    feats = np.maximum(np.random.default_rng(0).standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)
    runs = [("sample", dict()), ("sample typical_p 0.9", dict(typical_p=0.9)), ("sample top_p 0.9", dict(top_p=0.9))]
    ts, distinct = {n: [] for n, _ in runs}, {}
    for rep in range(reps + 2):
        for name, kw in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = gen.diverse(feats, draws=K, method="sample", **kw)
            torch.cuda.synchronize()
            if rep >= 2:
                ts[name].append((time.perf_counter() - t0) * 1e3)
            distinct[name] = float(np.mean([len(r) for r in res]))
    base = float(np.median(ts["sample"]))
    for name, _ in runs:
        ms = float(np.median(ts[name]))
        print(json.dumps({"images": B, "draws": K, "method": name, "diverse_ms": round(ms, 3), "min_ms": round(min(ts[name]), 3),
                          "max_ms": round(max(ts[name]), 3), "ratio_to_uncut": round(ms / base, 3),
                          "distinct_per_image": round(distinct[name], 2), "max_len": p.gen_max_len}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[640, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-diverse", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("typical_time.py measures on a GPU: none found")
    lib = abi.load()
    for R in a.rows:
        kernel_times(lib, R, 10000, a.reps, a.launches)
    if not a.skip_diverse:
        diverse_times(lib, a.reps)


if __name__ == "__main__":
    main()
