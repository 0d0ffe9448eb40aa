"""Posterior bounds timing on one GPU: 32 images x 5 captions x 16 tokens at full dimensions (V = 10 000, hidden 512, gen_z_samples 100,
latent 150), Normal prior, K = 20 and K = 100 draws per caption.  bound() and score() (the baseline: the same teacher forcing under
prior draws, existing code) alternate inside every repetition of one process; host clock around synchronised calls; the median of
`--reps` after two warm-ups and the spread (min .. max); then the phase breakdown of one bound() call (generate.PHASE_TIMES: the call
synchronises at its phase boundaries, so its phases add up to more than an untimed call).  Prints one JSON line per K.
    python tools/experiments/bound_time.py [--draws 20 100] [--reps 7] [--once bound|score] [--once_draws K]
--once: two warm calls then one timed call of that method only (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi, generate, spec  # noqa: E402
from vae_captioning_amd.engine import CaptionEngine  # noqa: E402
from vae_captioning_amd.generate import CaptionGenerator  # noqa: E402
from vae_captioning_amd.utils.parameters import Parameters  # noqa: E402

BOS, EOS = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", choices=["bound", "score"], default=None)
    ap.add_argument("--once_draws", type=int, default=20)
    a = ap.parse_args()
    lib = abi.load()
    p = Parameters()
    p.mode, p.num_captions, p.prior = "inference", 1, "Normal"
    V, B, NC, T = 10000, 32, 5, 16
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(spec.init_caption_params(p, V, seed=3))
    gen = CaptionGenerator(eng)
    rng = np.random.default_rng(0)
    feats = np.maximum(rng.standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)
    caps = [[rng.integers(3, V, size=T - 1).tolist() + [EOS] for _ in range(NC)] for _ in range(B)]
    calls = {"bound": lambda K: gen.bound(feats, caps, None, None, None, BOS, EOS, draws=K),
             "score": lambda K: gen.score(feats, caps, None, None, BOS, EOS, draws=K)}

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if a.once:
        for _ in range(2):
            calls[a.once](a.once_draws)
        print(json.dumps({"method": a.once, "draws": a.once_draws, "ms": round(clock(lambda: calls[a.once](a.once_draws)), 3)}))
        return
    for K in a.draws:
        for _ in range(2):
            calls["bound"](K)
            calls["score"](K)
        ts = {"bound": [], "score": []}
        for _ in range(a.reps):
            for name in ("bound", "score"):
                ts[name].append(clock(lambda: calls[name](K)))
        generate.PHASE_TIMES = {}
        calls["bound"](K)
        phases = {k: round(v * 1e3, 3) for k, v in generate.PHASE_TIMES.items() if k}
        generate.PHASE_TIMES = None
        med = {k: float(np.median(v)) for k, v in ts.items()}
        print(json.dumps({"images": B, "captions": B * NC, "tokens": T, "draws": K, "rows": B * NC * K, "reps": a.reps,
                          "bound_ms": round(med["bound"], 3), "bound_min_max_ms": [round(min(ts["bound"]), 3), round(max(ts["bound"]), 3)],
                          "score_ms": round(med["score"], 3), "score_min_max_ms": [round(min(ts["score"]), 3), round(max(ts["score"]), 3)],
                          "bound_over_score": round(med["bound"] / med["score"], 3), "bound_phases_ms": phases}))


if __name__ == "__main__":
    main()
