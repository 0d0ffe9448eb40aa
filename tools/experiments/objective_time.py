"""Training objective options: what each new kernel costs beside its plain form, on one GPU at the cfg2 shapes (1280 caption rows,
T = 20, vocabulary 10 000, latent 150, 100 z samples).  Three parts, each a child process of this script under its own timeout; the
script stops at the first part that fails.  One JSON line per part.

  xent  vc_softmax_xent_f32 vs vc_softmax_xent_smooth_f32 (eps 0.1) on the [25 600, 10 000] logits, gradient written in place
  kl    vc_kl_rows_f32 vs vc_kl_rows_fb_f32 and vc_latent_bwd_f32 vs vc_latent_bwd_fb_f32 at N = 1280, L = 150, S = 100
  step  the whole cfg2 training step (eager launches, device noise) with every option off and with every option on
        (--kl_free_bits 0.05 --kl_weight 0.5 --label_smoothing 0.1 --kl_cycle_steps 2000)

Clock: a pair of HIP events around each launch (xent, kl) or each step (step), median of --reps after --warmup; the two forms of a
pair alternate launch by launch in the same process, so both see the same clocks and neighbours.  GB/s = algorithmic bytes / median.
    python tools/experiments/objective_time.py [--part all|xent|kl|step] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TIMEOUTS = {"xent": 180, "kl": 120, "step": 300}


def ab(forms, reps, warmup):
    """{name: median ms} of the launches in `forms` ({name: callable}), alternated launch by launch"""
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
    from vae_captioning_amd import abi
    lib, P = abi.load(), abi.ptr
    rows, V = 1280 * 20, 10000
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(rows, V, device="cuda", generator=g) * 3
    labels = torch.randint(1, V, (rows,), device="cuda", dtype=torch.int32, generator=g)
    labels[::7] = 0
    den, rl = torch.zeros(1, device="cuda"), torch.zeros(rows, device="cuda")
    lib.vc_count_nonzero_i32(st, P(labels), rows, P(den))
    # (in place: after the first launch the buffer holds gradients -- the kernels' work does not depend on the values)
    forms = {"plain": lambda: lib.vc_softmax_xent_f32(st, P(logits), P(labels), rows, V, V, P(den), 1.0, P(rl), 1),
             "smooth": lambda: lib.vc_softmax_xent_smooth_f32(st, P(logits), P(labels), rows, V, V, P(den), 1.0, 0.1, P(rl), 1)}
    med, rng = ab(forms, a.reps, a.warmup)
    nbytes = 8.0 * rows * V
    print(json.dumps({"part": "xent", "rows": rows, "V": V, "plain_ms": round(med["plain"], 4), "smooth_ms": round(med["smooth"], 4),
                      "plain_min_max_ms": [round(x, 4) for x in rng["plain"]], "smooth_min_max_ms": [round(x, 4) for x in rng["smooth"]],
                      "ratio": round(med["smooth"] / med["plain"], 4), "plain_GBps": round(nbytes / med["plain"] / 1e6, 1),
                      "smooth_GBps": round(nbytes / med["smooth"] / 1e6, 1), "reps": a.reps}), flush=True)


def part_kl(a):
    import torch
    from vae_captioning_amd import abi
    lib, P = abi.load(), abi.ptr
    N, L, S = 1280, 150, 100
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    mean = torch.randn(N, L, device="cuda", generator=g) * 0.3
    std = torch.exp(torch.randn(N, L, device="cuda", generator=g) * 0.3)
    eps, dz = torch.randn(S, N, L, device="cuda", generator=g), torch.randn(S, N, L, device="cuda", generator=g)
    ann = torch.full((1,), 0.5, device="cuda")
    rk, raw, nf = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda", dtype=torch.int32)
    dm, ds = torch.zeros(N, L, device="cuda"), torch.zeros(N, L, device="cuda")
    out = {"part": "kl", "N": N, "L": L, "S": S, "reps": a.reps}
    for mode, tag in ((0, "normal"), (1, "ag")):
        mu = torch.randn(N, L, device="cuda", generator=g) * 0.1 if mode else None
        fwd = {"plain": lambda: lib.vc_kl_rows_f32(st, N, L, mode, P(mean), P(std), P(mu), P(rk)),
               "fb": lambda: lib.vc_kl_rows_fb_f32(st, N, L, mode, P(mean), P(std), P(mu), 0.05, P(rk), P(raw), P(nf))}
        bwd = {"plain": lambda: lib.vc_latent_bwd_f32(st, S, N, L, mode, 1 - mode, P(dz), P(eps), P(mean), P(std), P(mu), P(ann), 0.1 / N, P(dm), P(ds)),
               "fb": lambda: lib.vc_latent_bwd_fb_f32(st, S, N, L, mode, 1 - mode, P(dz), P(eps), P(mean), P(std), P(mu), P(ann), 0.1 / N, 0.05, P(dm), P(ds))}
        f, _ = ab(fwd, a.reps, a.warmup)
        b, _ = ab(bwd, a.reps, a.warmup)
        out[tag] = {"kl_rows_ms": round(f["plain"], 4), "kl_rows_fb_ms": round(f["fb"], 4), "latent_bwd_ms": round(b["plain"], 4),
                    "latent_bwd_fb_ms": round(b["fb"], 4), "latent_bwd_GBps": round(8.0 * S * N * L / b["plain"] / 1e6, 1),
                    "latent_bwd_fb_GBps": round(8.0 * S * N * L / b["fb"] / 1e6, 1)}
    print(json.dumps(out), flush=True)


def part_step(a):
    import numpy as np
    import torch
    from vae_captioning_amd import abi, spec, synth
    from vae_captioning_amd.trainer import Trainer
    from vae_captioning_amd.utils.parameters import Parameters
    lib = abi.load()
    V, B, T = 10000, 256, 20
    trs = {}
    for name, opts in (("off", {}), ("on", dict(kl_free_bits=0.05, kl_weight=0.5, label_smoothing=0.1, kl_cycle_steps=2000))):
        p = Parameters()
        p.batch_size, p.vocab_size = B, V
        for k, v in opts.items():
            setattr(p, k, v)
        tr = Trainer(p, V, lib=lib, seed=3)
        tr.load_state_dict(spec.init_caption_params(p, V, seed=1))
        tr.set_batch(synth.make_batch(np.random.default_rng(0), B, p.num_captions, T, V))
        trs[name] = tr
    med, rng = ab({k: tr.train_step for k, tr in trs.items()}, a.reps, a.warmup)
    stats = trs["on"].objective_stats()
    print(json.dumps({"part": "step", "workload": "cfg2 shape: 256 images (1280 rows), T 20, V 10000, eager launches", "off_ms": round(med["off"], 3),
                      "on_ms": round(med["on"], 3), "off_min_max_ms": [round(x, 3) for x in rng["off"]], "on_min_max_ms": [round(x, 3) for x in rng["on"]],
                      "on_objective_stats": stats, "reps": a.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "xent", "kl", "step"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.part != "all":
        import torch
        assert torch.cuda.is_available(), "objective_time.py measures on the GPU: no device, no numbers"
        {"xent": part_xent, "kl": part_kl, "step": part_step}[a.part](a)
        return
    for part in ("xent", "kl", "step"):   # one child process per part, each under its own timeout; stop at the first failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                               timeout=TIMEOUTS[part])
        except subprocess.TimeoutExpired:
            sys.exit("objective_time: part %s ran into its %d s limit; stopping" % (part, TIMEOUTS[part]))
        if r.returncode != 0:
            sys.exit("objective_time: part %s failed with status %d; stopping" % (part, r.returncode))


if __name__ == "__main__":
    main()
