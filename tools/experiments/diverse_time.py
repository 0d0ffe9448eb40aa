"""Diverse captioning timing on one GPU: 32 images at full dimensions (V = 10 000, decoder_hidden 512, gen_z_samples 100,
latent 150), Normal prior, K = 20 and K = 100 latent draws per image.  Host clock around a synchronised call, after warm-up; the same
K done as K sequential greedy calls in the same process.  Prints one JSON line per K.
    python tools/experiments/diverse_time.py [--draws 20 100] [--reps 5] [--once K]
--once K: one warm call then one timed call of diverse(draws=K) only (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    lib = abi.load()
    p = Parameters()
    p.mode, p.num_captions, p.prior = "inference", 1, "Normal"
    V, B = 10000, 32
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(spec.init_caption_params(p, V, seed=3))
    gen = CaptionGenerator(eng)
    feats = np.maximum(np.random.default_rng(0).standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)

    def clock(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3, out

    if a.once:
        gen.diverse(feats, draws=a.once)
        torch.cuda.synchronize()
        ms, _ = clock(lambda: gen.diverse(feats, draws=a.once), 1)
        print(json.dumps({"draws": a.once, "ms": round(ms, 3)}))
        return
    for K in a.draws:
        for _ in range(2):
            gen.diverse(feats, draws=K)
            gen.greedy(feats)
        ms, res = clock(lambda: gen.diverse(feats, draws=K), a.reps)
        g_ms, _ = clock(lambda: [gen.greedy(feats) for _ in range(K)], max(1, a.reps // 2))
        distinct = float(np.mean([len(r) for r in res]))
        print(json.dumps({"images": B, "draws": K, "diverse_ms": round(ms, 3), "captions_per_s": round(B * K / ms * 1e3, 1),
                          "sequential_greedy_ms": round(g_ms, 3), "ratio": round(ms / g_ms, 3), "distinct_per_image": round(distinct, 2),
                          "max_len": p.gen_max_len}))


if __name__ == "__main__":
    main()
