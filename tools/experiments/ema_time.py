"""Weight averaging: what the average costs, folded into the Adam pass against a launch of its own, on one GPU.  Two parts, each a child
process of this script under its own timeout; the script stops at the first part that fails.  One JSON line per measurement.

  kernel  three forms on the same five buffers (p, g, m, v, ema), at the size of the caption store of cfg2 and of the two `part`s of the
          VGG16 store (conv: the 13 convolution layers, fc: fc1 + fc2):
            adam       vc_adam_f32 alone                          28 B per parameter
            adam+ema   vc_adam_f32, then vc_ema_update_f32        40 B per parameter (two launches inside one pair of events)
            fused      vc_adam_ema_f32                            36 B per parameter
  step    the eager Trainer step of cfg2 (256 images, precomputed features) and of cfg4 (64 images, --fine_tune) with --ema_decay 0.999
          against off

Clock: a pair of HIP events around each launch (kernel: around the form's one or two launches) or each step, median of --reps after
--warmup; the forms alternate launch by launch in the same process, so all see the same clocks and neighbours.  GB/s = algorithmic
bytes / median.  Between two launches of a form the other forms run over other buffers (each form has its own set), so whether a form's
buffers survive in the last-level cache depends on the total footprint, which is reported.
    python tools/experiments/ema_time.py [--part all|kernel|step] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TIMEOUTS = {"kernel": 240, "step": 420}
VOCAB, T_LEN = 10000, 20
LLC_BYTES = 256 << 20   # MI355X: 256 MB of last-level (Infinity) cache


def ab(forms, reps, warmup):
    """{name: median ms}, {name: (min, max)} of the calls in `forms` ({name: callable}), alternated call by call"""
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


def part_kernel(a):
    import numpy as np
    import torch
    from vae_captioning_amd import abi, spec
    from vae_captioning_amd.engine import _round, flat_offsets, internal_caption_variables
    from vae_captioning_amd.utils.parameters import Parameters
    lib, P = abi.load(), abi.ptr
    st = torch.cuda.current_stream().cuda_stream
    p = Parameters()
    n_cap = sum(_round(int(np.prod(s))) for _, s in internal_caption_variables(p, VOCAB))
    offs, n_vgg = flat_offsets(spec.vgg_variables())
    o_fc = offs["cnn/fc1/weights"][0]
    lr, step = torch.full((1,), 1e-5, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    omd = 1.0 - 0.999
    for name, n in (("caption store (cfg2)", n_cap), ("vgg16 conv part", o_fc), ("vgg16 fc part", n_vgg - o_fc)):
        g = torch.Generator(device="cuda").manual_seed(1)
        sets = {}
        for form in ("adam", "adam+ema", "fused"):   # a buffer set per form: every form updates parameters of its own from the same start
            sets[form] = dict(p=torch.randn(n, device="cuda", generator=g), g=torch.randn(n, device="cuda", generator=g) * 1e-3,
                              m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"), e=torch.zeros(n, device="cuda"))
        adam = lambda s: lib.vc_adam_f32(st, P(s["p"]), P(s["g"]), P(s["m"]), P(s["v"]), n, P(lr), None, 0.8, 0.999, 1e-8, 0.0)
        forms = {"adam": lambda: adam(sets["adam"]),
                 "adam+ema": lambda: (adam(sets["adam+ema"]), lib.vc_ema_update_f32(st, P(sets["adam+ema"]["e"]), P(sets["adam+ema"]["p"]), n, omd, P(step))),
                 "fused": lambda: (lambda s: lib.vc_adam_ema_f32(st, P(s["p"]), P(s["g"]), P(s["m"]), P(s["v"]), P(s["e"]), n, P(lr), None, 0.8, 0.999,
                                                                 1e-8, 0.0, omd, P(step)))(sets["fused"])}
        med, rng = ab(forms, a.reps, a.warmup)
        bpp = {"adam": 28.0, "adam+ema": 40.0, "fused": 36.0}
        print(json.dumps({"part": "kernel", "buffers": name, "n": n, "MB_per_buffer": round(4e-6 * n, 1),
                          "one_form_fits_last_level_cache": bool(5 * 4 * n <= LLC_BYTES), "all_forms_fit_last_level_cache": bool(3 * 5 * 4 * n <= LLC_BYTES),
                          "footprint_MB_all_forms": round(3 * 5 * 4e-6 * n, 1),
                          "ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": {k: [round(x, 4) for x in v] for k, v in rng.items()},
                          "GBps": {k: round(bpp[k] * n / med[k] / 1e6, 1) for k in med},
                          "fused_over_two_launch": round(med["fused"] / med["adam+ema"], 4), "ema_cost_fused_ms": round(med["fused"] - med["adam"], 4),
                          "ema_cost_two_launch_ms": round(med["adam+ema"] - med["adam"], 4), "reps": a.reps}), flush=True)
        del sets, forms
        torch.cuda.empty_cache()


def part_step(a):
    import numpy as np
    from vae_captioning_amd import abi, spec, synth
    from vae_captioning_amd.trainer import Trainer
    from vae_captioning_amd.utils.parameters import Parameters
    lib = abi.load()
    for workload, B, fine in (("cfg2 shape: 256 images (1280 rows), T 20, V 10000", 256, False),
                              ("cfg4 shape: 64 images (320 rows), --fine_tune, T 20, V 10000", 64, True)):
        trs = {}
        PV = spec.init_vgg_params(seed=2) if fine else {}
        for name, opts in (("off", {}), ("on", dict(ema_decay=0.999))):
            p = Parameters()
            p.batch_size, p.vocab_size, p.fine_tune = B, VOCAB, fine
            for k, v in opts.items():
                setattr(p, k, v)
            tr = Trainer(p, VOCAB, lib=lib, seed=3)
            tr.load_state_dict({**spec.init_caption_params(p, VOCAB, seed=1), **PV})
            tr.set_batch(synth.make_batch(np.random.default_rng(0), B, p.num_captions, T_LEN, VOCAB, images=fine))
            trs[name] = tr
        med, rng = ab({k: tr.train_step for k, tr in trs.items()}, a.reps, a.warmup)
        print(json.dumps({"part": "step", "workload": workload + ", eager launches", "off_ms": round(med["off"], 3), "on_ms": round(med["on"], 3),
                          "off_min_max_ms": [round(x, 3) for x in rng["off"]], "on_min_max_ms": [round(x, 3) for x in rng["on"]],
                          "averaged_parameters": int(sum(e.store.n for e in trs["on"]._ema_engines())),
                          "losses_equal": trs["off"].losses() == trs["on"].losses(), "reps": a.reps}), flush=True)
        del trs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "kernel", "step"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.part != "all":
        import torch
        assert torch.cuda.is_available(), "ema_time.py measures on the GPU: no device, no numbers"
        {"kernel": part_kernel, "step": part_step}[a.part](a)
        return
    for part in ("kernel", "step"):   # one child process per part, each under its own timeout; stop at the first failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                               timeout=TIMEOUTS[part])
        except subprocess.TimeoutExpired:
            sys.exit("ema_time: part %s ran into its %d s limit; stopping" % (part, TIMEOUTS[part]))
        if r.returncode != 0:
            sys.exit("ema_time: part %s failed with status %d; stopping" % (part, r.returncode))


if __name__ == "__main__":
    main()
