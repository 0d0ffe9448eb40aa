"""Marginal decoding timing on one GPU: 32 images at full dimensions (V = 10 000, decoder_hidden 512, gen_z_samples 100, latent 150),
Normal prior.  Host clock around a synchronised call, median after warm-up, each pair in the same process and build:
  marginal_greedy(draws=20)                   beside  diverse(draws=20, method="greedy")   (the same rows and products; only the pick differs)
  marginal_beam_search(beam_size=5, draws=10) beside  beam_search(beam_size=5)
Prints one JSON line per pair.
    python tools/experiments/mixture_time.py [--reps 7] [--once]
--once: one warm call then one timed call of marginal_greedy(draws=20) only (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
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
        gen.marginal_greedy(feats, draws=20)
        torch.cuda.synchronize()
        ms, _ = clock(lambda: gen.marginal_greedy(feats, draws=20), 1)
        print(json.dumps({"draws": 20, "marginal_greedy_ms": round(ms, 3)}))
        return
    pairs = [("marginal_greedy", lambda: gen.marginal_greedy(feats, draws=20), "diverse_greedy", lambda: gen.diverse(feats, draws=20, method="greedy"),
              dict(draws=20, rows=B * 20)),
             ("marginal_beam_search", lambda: gen.marginal_beam_search(feats, beam_size=5, draws=10), "beam_search", lambda: gen.beam_search(feats, beam_size=5),
              dict(draws=10, beam_size=5, rows=B * 5 * 10, beam_search_rows=B * 5))]
    for name, fn, base_name, base, info in pairs:
        for _ in range(2):   # (the first call of a shape sizes and captures, the second replays)
            fn()
            base()
        ms, _ = clock(fn, a.reps)
        base_ms, _ = clock(base, a.reps)
        out = {"images": B, "max_len": p.gen_max_len, name + "_ms": round(ms, 3), base_name + "_ms": round(base_ms, 3), "ratio": round(ms / base_ms, 3)}
        out.update(info)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
