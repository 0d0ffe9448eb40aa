"""Mutual-information timing on one GPU (DESIGN.md "Bounds", "Mutual information"): vc_gauss_mix_lse_f64 alone on tensors that are on the
device, and latent_mi.mutual_information as a whole (upload of the table, the Philox draws, the kernel, one copy-back, the host means),
at N = M = 25 000 and N = M = 4 096 posteriors with S = 10 draws of L = 150 dimensions; host clock around synchronised calls, the median
of `--reps` after two warm-ups and the spread (min .. max).  Then the numpy float64 reference (tests/latent_mi_ref.py) on this host at
N = M = `--ref_n` (1 024), scaled by N^2 to the two sizes: what the kernel replaces, not a target.
The float64 rate: a Gaussian term is one subtraction, one multiplication and one fused multiply-add = 4 floating-point operations in
3 instructions; FP64_VECTOR_PEAK is AMD's published figure for the Instinct MI355X (78.6 TFLOP/s FP64 vector, the product's data
sheet; it counts a fused multiply-add as two), so a kernel that issued nothing but these three instructions would reach 4 / 6 of it.
Prints one JSON line per size and one for the reference, and writes them to `--out` (profiles/mi_time.txt).
    python tools/experiments/mi_time.py [--sizes 25000 4096] [--samples 10] [--latent 150] [--reps 7] [--ref_n 1024] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi, latent_mi  # noqa: E402
from vae_captioning_amd.abi import ptr as P  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12   # FLOP/s, AMD Instinct MI355X data sheet: peak double precision (FP64) vector
FLOPS_PER_TERM = 4           # sub, mul, fma


def table(rng, n, L):
    """posteriors like a trained encoder's: means of unit spread, widths around 0.1"""
    return rng.standard_normal((n, L)).astype(np.float32), np.exp(rng.standard_normal((n, L)) * 0.5 - 2.5).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[25000, 4096])
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--latent", type=int, default=150)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref_n", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mi_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mi_time.py measures on the GPU: none visible")
    lib = abi.load()
    S, L = a.samples, a.latent
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def median(fn):
        for _ in range(2):
            fn()
        ts = [clock(fn) for _ in range(a.reps)]
        return float(np.median(ts)), [round(min(ts), 3), round(max(ts), 3)]

    for n in a.sizes:
        rng = np.random.default_rng(n)
        mean, std = table(rng, n, L)
        md, sd = torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()
        z = torch.empty((n, S, L), device="cuda")
        logw = torch.empty(n, dtype=torch.float64, device="cuda")
        lib.vc_posterior_latent_f32(st, n, 1, S, L, P(md), P(sd), None, None, 1.0, None, 1, latent_mi.MI_PHILOX_STREAM << 32, None, P(z), P(logw))
        out = torch.empty(n * S + n, dtype=torch.float64, device="cuda")
        k_ms, k_mm = median(lambda: lib.vc_gauss_mix_lse_f64(st, n, n, S, L, P(z), P(md), P(sd), P(out), P(out) + 8 * n * S))
        res = {}
        w_ms, w_mm = median(lambda: res.update(latent_mi.mutual_information(mean, std, S, seed=1, lib=lib)))
        terms = float(n) * n * S * L
        rate = terms * FLOPS_PER_TERM / (k_ms * 1e-3)
        lines.append({"N": n, "M": n, "S": S, "L": L, "reps": a.reps, "gauss_mix_lse_ms": round(k_ms, 3), "gauss_mix_lse_min_max_ms": k_mm,
                      "mutual_information_ms": round(w_ms, 3), "mutual_information_min_max_ms": w_mm, "gaussian_terms": terms,
                      "fp64_tflops": round(rate / 1e12, 3), "fp64_vector_peak_tflops": FP64_VECTOR_PEAK / 1e12,
                      "share_of_fp64_vector_peak": round(rate / FP64_VECTOR_PEAK, 4),
                      "share_of_fp64_issue_slots": round(terms * 3 / (k_ms * 1e-3) / (FP64_VECTOR_PEAK / 2), 4),
                      "mi": res["mi"], "mi_block": res["mi_block"], "mi_ceiling": res["mi_ceiling"]})
        print(json.dumps(lines[-1]), flush=True)
        del z, out, md, sd
    if a.ref_n > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import latent_mi_ref as ref
        n = a.ref_n
        rng = np.random.default_rng(n)
        mean, std = table(rng, n, L)
        zh = ref.draws(mean, std, rng.standard_normal((n, S, L)))
        t0 = time.perf_counter()
        ref.gauss_mix_lse(zh, mean, std)
        r_s = time.perf_counter() - t0
        lines.append({"numpy_reference_N": n, "S": S, "L": L, "seconds": round(r_s, 3),
                      "scaled_by_N2_seconds": {str(m): round(r_s * (float(m) / n) ** 2, 1) for m in a.sizes}})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
