"""Unlikelihood training: what vc_softmax_xent_ul_f32 costs beside vc_softmax_xent_smooth_f32, on one GPU at the caption-only shape
(1344 caption rows, T = 20: logits [26 880, 10 000], 2.15 GB read + written per launch), gradient written in place, on the SAME
buffers in the SAME process.  The labels are caption-shaped: time-major [T, N] targets of synthetic captions of varying length with
their PAD tails (synth.make_batch), so that a row at step t has up to t candidates and the PAD rows have none.

Clock: a pair of HIP events around each launch, median of --reps after --warmup; the two entries alternate launch by launch, so both
see the same clocks and neighbours.  GB/s = algorithmic bytes (8 B per logit) / median.  One JSON line.
    python tools/experiments/unlikelihood_time.py [--reps 50] [--warmup 10] [--window 128]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=int, default=128)
    a = ap.parse_args()
    import numpy as np
    import torch
    from vae_captioning_amd import abi, synth
    if not torch.cuda.is_available():
        raise SystemExit("unlikelihood_time.py measures on the GPU: none found")
    lib, P = abi.load(), abi.ptr
    N, T, V = 1344, 20, 10000
    rows = N * T
    st = torch.cuda.current_stream().cuda_stream
    batch = synth.make_batch(np.random.default_rng(0), N, 1, T, V, variable_len=True, feature_size=4)
    labels_h = np.ascontiguousarray(batch["cap_enc"].T).astype(np.int32)          # [T, N]
    labels = torch.from_numpy(labels_h).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(rows, V, device="cuda", generator=g) * 3
    den, rl, ru, rm = (torch.zeros(n, device="cuda") for n in (1, rows, rows, rows))
    rc = torch.zeros(rows, device="cuda", dtype=torch.int32)
    lib.vc_count_nonzero_i32(st, P(labels), rows, P(den))
    # (in place: after the first launch the buffer holds gradients -- the kernels' memory work does not depend on the values)
    forms = {"smooth": lambda: lib.vc_softmax_xent_smooth_f32(st, P(logits), P(labels), rows, V, V, P(den), 1.0, 0.1, P(rl), 1),
             "ul": lambda: lib.vc_softmax_xent_ul_f32(st, P(logits), P(labels), rows, N, V, V, P(den), 1.0, 0.1, 1.0, a.window, P(rl), P(ru), P(rc), P(rm), 1)}
    for _ in range(a.warmup):
        for fn in forms.values():
            fn()
    ts = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    nbytes = 8.0 * rows * V
    live = int((labels_h != 0).sum())
    print(json.dumps({"rows": rows, "N": N, "T": T, "V": V, "window": a.window, "live_rows": live,
                      "mean_candidates_per_live_row": round(float(rc.sum().item()) / live, 3),
                      "smooth_ms": round(med["smooth"], 4), "ul_ms": round(med["ul"], 4),
                      "smooth_min_max_ms": [round(min(ts["smooth"]), 4), round(max(ts["smooth"]), 4)],
                      "ul_min_max_ms": [round(min(ts["ul"]), 4), round(max(ts["ul"]), 4)],
                      "ratio": round(med["ul"] / med["smooth"], 4), "smooth_GBps": round(nbytes / med["smooth"] / 1e6, 1),
                      "ul_GBps": round(nbytes / med["ul"] / 1e6, 1), "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
