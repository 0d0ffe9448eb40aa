"""Scheduled sampling (--sched_sampling, DESIGN.md "Scheduled sampling"): what the second decoder pass and the mix cost, on one GPU.
Three parts, each a child process of this script under its own timeout; the script stops at the first part that fails.  One JSON line
per part and workload.

  off     the eager training step with the mode off at cfg2 (256 images = 1280 caption rows, T 20, V 10 000, precomputed features) and
          cfg4 (64 images, VGG16 fine-tuned).  Uses nothing this feature added, so the same file runs on the parent commit: with
          --parent FILE (the output of that run) each line carries the parent's figures beside its own.
  on      the same two steps with the mode off and with --sched_sampling 0.25 --sched_schedule constant, alternating step by step in
          one process (both see the same clocks and neighbours)
  kernel  vc_sched_mix_f32 alone at the cfg2 shape ([25 600, 10 000] logits, T 20, N 1280) at rates 0.25 and 1.0, sampled and argmax
          pick; GB/s = 4 B x V x selected rows / median (the logits rows the call has to read)

Clock: a pair of HIP events around each step or launch, median of --reps after --warmup; min and max are the spread over the repetitions.
    python tools/experiments/sched_time.py [--part all|off|on|kernel] [--reps 30] [--warmup 5] [--parent FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TIMEOUTS = {"off": 300, "on": 420, "kernel": 120}
WORKLOADS = {"cfg2": dict(B=256, fine_tune=False), "cfg4": dict(B=64, fine_tune=True)}
V, T = 10000, 20


def ab(forms, reps, warmup):
    """{name: (median, min, max) ms} of the callables in `forms`, alternated call by call"""
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
    return {k: (round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)) for k, v in ts.items()}


def make_trainer(workload, **opts):
    import numpy as np
    from vae_captioning_amd import abi, spec, synth
    from vae_captioning_amd.trainer import Trainer
    from vae_captioning_amd.utils.parameters import Parameters
    w = WORKLOADS[workload]
    p = Parameters()
    p.batch_size, p.vocab_size, p.fine_tune = w["B"], V, w["fine_tune"]
    for k, v in opts.items():
        setattr(p, k, v)
    tr = Trainer(p, V, lib=abi.load(), seed=3)
    tr.load_state_dict({**spec.init_caption_params(p, V, seed=1), **(spec.init_vgg_params(seed=2) if p.fine_tune else {})})
    tr.set_batch(synth.make_batch(np.random.default_rng(0), w["B"], p.num_captions, T, V, images=bool(p.fine_tune)))
    return tr


def describe(workload):
    w = WORKLOADS[workload]
    return "%s shape: %d images (%d rows), T %d, V %d%s, eager launches" % (workload, w["B"], w["B"] * 5, T, V, ", VGG16 fine-tuned" if w["fine_tune"] else "")


def part_off(a):
    parent = {}
    if a.parent:
        for line in open(a.parent):
            if line.startswith("{"):
                d = json.loads(line)
                if d.get("part") == "off":
                    parent[d["workload"].split()[0]] = d
    for workload in WORKLOADS:
        tr = make_trainer(workload)
        med, lo, hi = ab({"off": tr.train_step}, a.reps, a.warmup)["off"]
        out = {"part": "off", "workload": describe(workload), "off_ms": med, "off_min_max_ms": [lo, hi], "reps": a.reps}
        if workload in parent:
            out["parent_off_ms"], out["parent_off_min_max_ms"] = parent[workload]["off_ms"], parent[workload]["off_min_max_ms"]
        print(json.dumps(out), flush=True)
        del tr


def part_on(a):
    for workload in WORKLOADS:
        trs = {"off": make_trainer(workload), "on": make_trainer(workload, sched_sampling=0.25, sched_schedule="constant")}
        r = ab({k: tr.train_step for k, tr in trs.items()}, a.reps, a.warmup)
        print(json.dumps({"part": "on", "workload": describe(workload), "off_ms": r["off"][0], "on_ms": r["on"][0], "off_min_max_ms": list(r["off"][1:]),
                          "on_min_max_ms": list(r["on"][1:]), "on_minus_off_ms": round(r["on"][0] - r["off"][0], 3), "on_sched_stats": trs["on"].sched_stats(),
                          "reps": a.reps}), flush=True)
        del trs


def part_kernel(a):
    import torch
    from vae_captioning_amd import abi
    lib, P = abi.load(), abi.ptr
    N = 1280
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(T * N, V, device="cuda", generator=g) * 3
    cap = torch.randint(3, V, (T, N), device="cuda", dtype=torch.int32, generator=g)
    lens = torch.full((N,), T, device="cuda", dtype=torch.int32)
    coin, u = torch.rand(T, N, device="cuda", generator=g), torch.rand(T, N, device="cuda", generator=g)
    step, out = torch.ones(1, device="cuda", dtype=torch.int32), torch.zeros(T, N, device="cuda", dtype=torch.int32)
    stats, rate_out = torch.zeros(2, device="cuda", dtype=torch.int32), torch.zeros(1, device="cuda")
    for rate in (0.25, 1.0):
        call = lambda uu: lib.vc_sched_mix_f32(st, P(logits), V, V, T, N, P(cap), P(lens), P(coin), uu, 1.0, P(step), 0, rate, 1, P(out), P(stats), P(rate_out))
        r = ab({"sample": lambda: call(P(u)), "argmax": lambda: call(None)}, a.reps, a.warmup)
        stats.zero_()
        call(P(u))
        eligible, selected = [int(x) for x in stats.cpu()]
        gb = 4.0 * V * selected / 1e6
        print(json.dumps({"part": "kernel", "T": T, "N": N, "V": V, "rate": rate, "eligible": eligible, "selected": selected,
                          "sample_ms": r["sample"][0], "sample_min_max_ms": list(r["sample"][1:]), "argmax_ms": r["argmax"][0],
                          "argmax_min_max_ms": list(r["argmax"][1:]), "sample_GBps": round(gb / max(r["sample"][0], 1e-6), 1),
                          "argmax_GBps": round(gb / max(r["argmax"][0], 1e-6), 1), "reps": a.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "off", "on", "kernel"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", default=None, help="output of this script's --part off on the parent commit: printed beside the off lines")
    a = ap.parse_args()
    if a.part != "all":
        import torch
        assert torch.cuda.is_available(), "sched_time.py measures on the GPU: no device, no numbers"
        {"off": part_off, "on": part_on, "kernel": part_kernel}[a.part](a)
        return
    for part in ("off", "on", "kernel"):   # one child process per part, each under its own timeout; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        if a.parent and part == "off":
            cmd += ["--parent", a.parent]
        try:
            r = subprocess.run(cmd, timeout=TIMEOUTS[part])
        except subprocess.TimeoutExpired:
            sys.exit("sched_time: part %s ran into its %d s limit; stopping" % (part, TIMEOUTS[part]))
        if r.returncode != 0:
            sys.exit("sched_time: part %s failed with status %d; stopping" % (part, r.returncode))


if __name__ == "__main__":
    main()
