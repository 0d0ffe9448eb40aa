"""Caption scoring timing on one GPU, full dimensions (V = 10 000, decoder_hidden 512, gen_z_samples 100, latent 150), Normal prior.
Medians of synchronised calls after warm-up; one JSON line per measurement.
    python tools/experiments/score_time.py [--part kernel score diverse] [--reps 7] [--once kernel|score]
kernel   vc_logits_logprob_f32 (fused: the logits never leave the chip) against the composition it replaces -- vc_gemm_f32 into a
         [R, Vp] buffer, then vc_softmax_xent_f32(write_grad = 0) -- at R = 51 200 and R = 10 240, HIP events round each; TFLOP/s of the
         fused pair, of the composition and of the product alone (2 R V H flops)
score    whole score() calls: 32 images x 5 captions of 16 tokens under K = 20 and K = 100 draws, host clock, and their phases
diverse  diverse(draws=20) with likelihood against marginal re-ranking
--once X: one warm call then one call only (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_captioning_amd import abi, generate, spec  # noqa: E402
from vae_captioning_amd.abi import ptr as P  # noqa: E402
from vae_captioning_amd.engine import CaptionEngine  # noqa: E402
from vae_captioning_amd.generate import CaptionGenerator  # noqa: E402
from vae_captioning_amd.utils.parameters import Parameters  # noqa: E402

V, H, B = 10000, 512, 32


def events(fn, reps):
    """median milliseconds of fn() between two HIP events on the current stream"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def clock(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def kernel_part(lib, reps, once):
    st = lambda: torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    W = torch.randn((H, V), device="cuda", generator=g) * (2.0 / np.sqrt(H))
    bias = torch.randn((V,), device="cuda", generator=g)
    den = torch.ones(1, device="cuda")
    for R in ((51200,) if once else (51200, 10240)):
        hs = torch.rand((R, H), device="cuda", generator=g) * 2 - 1
        lab = torch.randint(1, V, (R,), device="cuda", generator=g, dtype=torch.int32)
        lp, loss = torch.zeros(R, device="cuda"), torch.zeros(R, device="cuda")
        need = lib.vc_logits_logprob_workspace_bytes(R, V, H)
        ws = torch.empty(need // 4 + 4, device="cuda")
        gneed = lib.vc_gemm_workspace_bytes(R, V, H)
        gws = torch.empty(max(gneed, 16) // 4 + 4, device="cuda")
        fused = lambda: lib.vc_logits_logprob_f32(st(), R, V, H, P(hs), H, P(W), V, P(bias), P(lab), P(lp), P(ws), need)
        if once:
            fused()
            torch.cuda.synchronize()
            print(json.dumps({"rows": R, "fused_ms": round(events(fused, 1), 3)}))
            return
        logits = torch.empty((R, V), device="cuda")
        gemm = lambda: lib.vc_gemm_f32(st(), 0, 0, R, V, H, P(hs), H, P(W), V, P(logits), V, P(bias), 0, P(gws), gws.numel() * 4)

        def comp():
            gemm()
            lib.vc_softmax_xent_f32(st(), P(logits), P(lab), R, V, V, P(den), 1.0, P(loss), 0)

        for _ in range(3):
            fused(), comp()
        diff = float((lp + loss).abs().max())
        # interleaved: clock drift and thermal state hit both alike
        f_ms, c_ms, g_ms = [], [], []
        for _ in range(reps):
            f_ms.append(events(fused, 1)), c_ms.append(events(comp, 1)), g_ms.append(events(gemm, 1))
        f, c, gm = (float(np.median(x)) for x in (f_ms, c_ms, g_ms))
        tf = lambda ms: round(2.0 * R * V * H / ms / 1e9, 1)
        print(json.dumps({"rows": R, "V": V, "H": H, "fused_ms": round(f, 3), "gemm_then_xent_ms": round(c, 3), "gemm_alone_ms": round(gm, 3),
                          "fused_over_composition": round(f / c, 3), "fused_tflops": tf(f), "composition_tflops": tf(c), "gemm_tflops": tf(gm),
                          "fused_ms_min_max": [round(min(f_ms), 3), round(max(f_ms), 3)], "composition_ms_min_max": [round(min(c_ms), 3), round(max(c_ms), 3)],
                          "workspace_mb": round(need / 2 ** 20, 1), "logits_mb": round(R * V * 4 / 2 ** 20, 1), "max_abs_difference": diff}))
        del logits


def engine(lib):
    p = Parameters()
    p.mode, p.num_captions, p.prior = "inference", 1, "Normal"
    eng = CaptionEngine(p, V, lib=lib)
    eng.load_params(spec.init_caption_params(p, V, seed=3))
    feats = np.maximum(np.random.default_rng(0).standard_normal((B, p.cnn_feature_size)), 0).astype(np.float32)
    return p, CaptionGenerator(eng), feats


def score_part(lib, reps, once):
    p, gen, feats = engine(lib)
    rng = np.random.default_rng(1)
    caps = [[rng.integers(3, V, size=15).tolist() + [2] for _ in range(5)] for _ in range(B)]
    for K in ((20,) if once else (20, 100)):
        for _ in range(2):
            gen.score(feats, caps, draws=K)
        if once:
            ms, _ = clock(lambda: gen.score(feats, caps, draws=K), 1)
            print(json.dumps({"draws": K, "score_ms": round(ms, 3)}))
            return
        ms, res = clock(lambda: gen.score(feats, caps, draws=K), reps)
        generate.PHASE_TIMES = {}
        for _ in range(reps):
            gen.score(feats, caps, draws=K)
        ph = {k: round(v / reps * 1e3, 3) for k, v in generate.PHASE_TIMES.items() if k}
        generate.PHASE_TIMES = None
        rows = B * 5 * K
        print(json.dumps({"images": B, "captions_per_image": 5, "tokens": 16, "draws": K, "sequence_rows": rows, "row_steps": rows * 16,
                          "passes": -(-rows * 16 // gen.score_rows), "score_ms": round(ms, 3), "phases_ms_synchronised": ph,
                          "mean_marginal": round(float(np.mean([r["marginal"] for im in res for r in im])), 3)}))


def diverse_part(lib, reps):
    p, gen, feats = engine(lib)
    K = 20
    for mode in ("likelihood", "marginal"):
        for _ in range(2):
            gen.diverse(feats, draws=K, rerank=mode)
    out = {"images": B, "draws": K}
    for mode in ("likelihood", "marginal"):
        ms, res = clock(lambda: gen.diverse(feats, draws=K, rerank=mode), reps)
        out[mode + "_ms"] = round(ms, 3)
        out["distinct_per_image"] = round(float(np.mean([len(r) for r in res])), 2)
    out["rescoring_adds_ms"] = round(out["marginal_ms"] - out["likelihood_ms"], 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "score", "diverse"], choices=["kernel", "score", "diverse"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", default=None, choices=["kernel", "score"])
    a = ap.parse_args()
    lib = abi.load()
    if a.once:
        (kernel_part if a.once == "kernel" else score_part)(lib, 1, True)
        return
    if "kernel" in a.part:
        kernel_part(lib, a.reps, False)
    if "score" in a.part:
        score_part(lib, a.reps, False)
    if "diverse" in a.part:
        diverse_part(lib, a.reps)


if __name__ == "__main__":
    main()
