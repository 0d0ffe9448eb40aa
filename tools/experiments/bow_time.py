"""Bag-of-words auxiliary loss: what the head costs, on one GPU at the cfg2 shapes (1280 caption rows, T = 20, vocabulary 10 000,
embedding width of the shipped parameters).  Three parts, each a child process of this script under its own timeout; the script stops
at the first part that fails.  One JSON line per part.

  xent  vc_bow_xent_f32 beside vc_softmax_xent_f32 on the SAME [1280, 10 000] buffer, gradient written in place; the bag-of-words
        labels are caption-shaped ([T, N] targets of synthetic captions of varying length with their PAD tails)
  gemm  the head's three products: bow_logits = X @ W + b, dW = X^T @ dbow, d_in = dbow @ W^T
  step  the whole cfg2 training step (eager launches, device noise) with --bow_loss 1 against off

Clock: a pair of HIP events around each launch (xent, gemm) or each step (step), median of --reps after --warmup; the forms of a part
alternate launch by launch in the same process, so all see the same clocks and neighbours.  GB/s = algorithmic bytes / median.
    python tools/experiments/bow_time.py [--part all|xent|gemm|step] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TIMEOUTS = {"xent": 120, "gemm": 120, "step": 300}
N_ROWS, T_LEN, VOCAB = 1280, 20, 10000


def ab(forms, reps, warmup):
    """{name: median ms}, {name: (min, max)} of the launches in `forms` ({name: callable}), alternated launch by launch"""
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    ts = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in ts.items()}, {k: (float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def part_xent(a):
    import numpy as np
    import torch
    from vae_captioning_amd import abi, synth
    lib, P = abi.load(), abi.ptr
    N, T, V = N_ROWS, T_LEN, VOCAB
    st = torch.cuda.current_stream().cuda_stream
    batch = synth.make_batch(np.random.default_rng(0), N, 1, T, V, variable_len=True, feature_size=4)
    labels_h = np.ascontiguousarray(batch["cap_enc"].T).astype(np.int32)          # [T, N]
    labels = torch.from_numpy(labels_h).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(N, V, device="cuda", generator=g) * 3
    den, rl, rm = (torch.zeros(n, device="cuda") for n in (1, N, N))
    rw = torch.zeros(N, device="cuda", dtype=torch.int32)
    lib.vc_count_nonzero_i32(st, P(labels), T * N, P(den))
    # (in place: after the first launch the buffer holds gradients -- the kernels' memory work does not depend on the values; the plain
    # entry takes the captions' first words as its labels)
    forms = {"plain": lambda: lib.vc_softmax_xent_f32(st, P(logits), P(labels), N, V, V, P(den), 1.0, P(rl), 1),
             "bow": lambda: lib.vc_bow_xent_f32(st, P(logits), N, V, V, P(labels), T, N, P(den), 1.0, P(rl), P(rm), P(rw), 1)}
    med, rng = ab(forms, a.reps, a.warmup)
    nbytes = 8.0 * N * V
    print(json.dumps({"part": "xent", "rows": N, "V": V, "T": T, "mean_distinct_words": round(float(rw.sum().item()) / max(int((rw > 0).sum().item()), 1), 3),
                      "plain_ms": round(med["plain"], 4), "bow_ms": round(med["bow"], 4),
                      "plain_min_max_ms": [round(x, 4) for x in rng["plain"]], "bow_min_max_ms": [round(x, 4) for x in rng["bow"]],
                      "ratio": round(med["bow"] / med["plain"], 4), "plain_GBps": round(nbytes / med["plain"] / 1e6, 1),
                      "bow_GBps": round(nbytes / med["bow"] / 1e6, 1), "reps": a.reps}), flush=True)


def part_gemm(a):
    import torch
    from vae_captioning_amd import abi
    from vae_captioning_amd.utils.parameters import Parameters
    lib, P = abi.load(), abi.ptr
    N, V, E = N_ROWS, VOCAB, int(Parameters().embed_size)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(2)
    X, W, b = torch.randn(N, E, device="cuda", generator=g), torch.randn(E, V, device="cuda", generator=g) * 0.02, torch.zeros(V, device="cuda")
    Y, dW, dX = torch.zeros(N, V, device="cuda"), torch.zeros(E, V, device="cuda"), torch.zeros(N, E, device="cuda")
    dY = torch.randn(N, V, device="cuda", generator=g) * 1e-3
    nb = max(int(lib.vc_gemm_workspace_bytes(N, V, E)), int(lib.vc_gemm_workspace_bytes(E, V, N)), int(lib.vc_gemm_workspace_bytes(N, E, V)), 1 << 20)
    ws = torch.empty(nb // 4 + 16, device="cuda")
    gemm = lambda ta, tb, M, Nn, K, A, lda, B, ldb, C, ldc, bias: lib.vc_gemm_f32(st, ta, tb, M, Nn, K, P(A), lda, P(B), ldb, P(C), ldc, P(bias), 0, P(ws), ws.numel() * 4)
    forms = {"fwd": lambda: gemm(0, 0, N, V, E, X, E, W, V, Y, V, b),
             "dW": lambda: gemm(1, 0, E, V, N, X, E, dY, V, dW, V, None),
             "d_in": lambda: gemm(0, 1, N, E, V, dY, V, W, V, dX, E, None)}
    med, rng = ab(forms, a.reps, a.warmup)
    fl = 2.0 * N * V * E
    print(json.dumps({"part": "gemm", "rows": N, "V": V, "E": E, "fwd_ms": round(med["fwd"], 4), "dW_ms": round(med["dW"], 4), "d_in_ms": round(med["d_in"], 4),
                      "fwd_TFLOPs": round(fl / med["fwd"] / 1e9, 2), "dW_TFLOPs": round(fl / med["dW"] / 1e9, 2), "d_in_TFLOPs": round(fl / med["d_in"] / 1e9, 2),
                      "min_max_ms": {k: [round(x, 4) for x in v] for k, v in rng.items()}, "reps": a.reps}), flush=True)


def part_step(a):
    import numpy as np
    from vae_captioning_amd import abi, spec, synth
    from vae_captioning_amd.trainer import Trainer
    from vae_captioning_amd.utils.parameters import Parameters
    lib = abi.load()
    V, B, T = VOCAB, 256, T_LEN
    trs = {}
    for name, opts in (("off", {}), ("on", dict(bow_loss=1.0))):
        p = Parameters()
        p.batch_size, p.vocab_size = B, V
        for k, v in opts.items():
            setattr(p, k, v)
        tr = Trainer(p, V, lib=lib, seed=3)
        tr.load_state_dict(spec.init_caption_params(p, V, seed=1))
        tr.set_batch(synth.make_batch(np.random.default_rng(0), B, p.num_captions, T, V))
        trs[name] = tr
    med, rng = ab({k: tr.train_step for k, tr in trs.items()}, a.reps, a.warmup)
    print(json.dumps({"part": "step", "workload": "cfg2 shape: 256 images (1280 rows), T 20, V 10000, eager launches", "off_ms": round(med["off"], 3),
                      "on_ms": round(med["on"], 3), "off_min_max_ms": [round(x, 3) for x in rng["off"]], "on_min_max_ms": [round(x, 3) for x in rng["on"]],
                      "on_objective_stats": trs["on"].objective_stats(), "reps": a.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "xent", "gemm", "step"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.part != "all":
        import torch
        assert torch.cuda.is_available(), "bow_time.py measures on the GPU: no device, no numbers"
        {"xent": part_xent, "gemm": part_gemm, "step": part_step}[a.part](a)
        return
    for part in ("xent", "gemm", "step"):   # one child process per part, each under its own timeout; stop at the first failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                               timeout=TIMEOUTS[part])
        except subprocess.TimeoutExpired:
            sys.exit("bow_time: part %s ran into its %d s limit; stopping" % (part, TIMEOUTS[part]))
        if r.returncode != 0:
            sys.exit("bow_time: part %s failed with status %d; stopping" % (part, r.returncode))


if __name__ == "__main__":
    main()
