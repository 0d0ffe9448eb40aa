"""What a self-critical training step costs, beside the cross-entropy step it fine-tunes: one GPU, the cfg2 shapes (caption-only CVAE,
Normal prior, 256 images x 5 captions = 1280 rows, vocabulary 10 000, latent 150, 100 z samples, samples of at most gen_max_len = 30
tokens), eager launches, device noise.

  kernel  vc_softmax_xent_policy_f32 (entropy weight 0 and 0.01) beside vc_softmax_xent_f32 on [25 600, 10 000] logits, gradient in
        place: a pair of HIP events around each launch, the three forms alternating launch by launch, median of 2 x --reps
  xe    the XE training step of the same trainer on a T = 20 batch: a pair of HIP events around each step, median of --reps
  scst  Trainer.scst_step with baseline "average" and "greedy" (entropy weight 0.01), split into its phases on the HOST clock, each
        phase closed by a device synchronise (Trainer.scst_times): sample / greedy pass / reward (its host share -- token lists ->
        word rows -- beside it) / upload of the policy batch / policy forward + backward / optimiser; median over --reps steps of the
        per-step sums.  The phases are serial in a step (each needs the one before it), so their sum is the step.  --scst_rouge W..:
        one run per weight of the ROUGE-L term of the reward (0: CIDEr-D alone, the default; W > 0: scst.SumReward, CIDEr-D + W *
        ROUGE-L, one more launch and one more copy-back in the reward phase).

The weights are random, so samples rarely end before gen_max_len: the policy batch has T = 30 -- the most a step can cost at these
shapes.  One JSON line per part.  There is no target: the numbers are what was measured.
    python tools/scst_time.py [--reps 15] [--warmup 3] [--scst_rouge 0 0.5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scst_rouge", type=float, nargs="+", default=[0.0])
    a = ap.parse_args()
    import numpy as np
    import torch
    from vae_captioning_amd import abi, scst, spec, synth
    from vae_captioning_amd.trainer import Trainer
    from vae_captioning_amd.utils.parameters import Parameters
    assert torch.cuda.is_available(), "scst_time.py measures on the GPU: no device, no numbers"
    lib = abi.load()
    V, B, T = 10000, 256, 20
    rng = np.random.default_rng(0)
    corpus_batch = synth.make_batch(np.random.default_rng(11), 512, 5, 12, V, feature_size=8)
    corpus = [[[int(t) for t in r] for r in corpus_batch["cap_enc"][i * 5:(i + 1) * 5]] for i in range(512)]   # main.py's --synthetic index
    # ---- the loss kernel beside the cross-entropy kernel it stands next to: [25 600, 10 000] logits, gradient in place, launches alternating
    P, st = abi.ptr, torch.cuda.current_stream().cuda_stream
    rows, N = 1280 * T, 1280
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(rows, V, device="cuda", generator=g) * 3
    labels = torch.randint(1, V, (rows,), device="cuda", dtype=torch.int32, generator=g)
    labels[::7] = 0
    den, rl, re, adv = torch.zeros(1, device="cuda"), torch.zeros(rows, device="cuda"), torch.zeros(rows, device="cuda"), torch.randn(N, device="cuda", generator=g)
    lib.vc_count_nonzero_i32(st, P(labels), rows, P(den))
    forms = {"xent": lambda: lib.vc_softmax_xent_f32(st, P(logits), P(labels), rows, V, V, P(den), 1.0, P(rl), 1),
             "policy": lambda: lib.vc_softmax_xent_policy_f32(st, P(logits), P(labels), rows, V, V, P(adv), N, 1.0 / N, 0.0, P(rl), None, 1),
             "policy_entropy": lambda: lib.vc_softmax_xent_policy_f32(st, P(logits), P(labels), rows, V, V, P(adv), N, 1.0 / N, 0.01, P(rl), P(re), 1)}
    ts = {k: [] for k in forms}
    for i in range(a.warmup + 2 * a.reps):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ts[k].append(e0.elapsed_time(e1))
    print(json.dumps(dict({"part": "kernel", "rows": rows, "V": V, "reps": 2 * a.reps}, **{k + "_ms": round(float(np.median(v)), 4) for k, v in ts.items()},
                          **{k + "_GBps": round(8.0 * rows * V / (float(np.median(v)) * 1e-3) / 1e9, 1) for k, v in ts.items()})), flush=True)
    del logits
    xe_done = False
    for baseline, rouge_w in [(b, w) for b in ("average", "greedy") for w in a.scst_rouge]:
        p = Parameters()
        p.batch_size, p.vocab_size = B, V
        tr = Trainer(p, V, lib=lib, seed=3)
        tr.load_state_dict(spec.init_caption_params(p, V, seed=1))
        batch = synth.make_batch(rng, B, p.num_captions, T, V, variable_len=True)
        if not xe_done:   # the XE step beside it, once
            xe_done = True
            tr.set_batch(batch)
            ts = []
            for i in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.train_step()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ts = ts[a.warmup:]
            print(json.dumps({"part": "xe", "workload": "cfg2 shape: 256 images (1280 rows), T 20, V 10000, eager launches", "step_ms": round(float(np.median(ts)), 3),
                              "min_max_ms": [round(min(ts), 3), round(max(ts), 3)], "reps": a.reps}), flush=True)
        reward = scst.CiderReward(tr.cap, corpus, synth.BOS, synth.EOS, V)
        if rouge_w > 0:
            reward = scst.SumReward([(reward, 1.0), (scst.RougeReward(tr.cap, synth.BOS, synth.EOS), rouge_w)])
        tr.enable_scst(reward, synth.BOS, synth.EOS, baseline=baseline, beta=0.01)
        for _ in range(a.warmup):
            tr.scst_step(batch)
        rows, wall, host = [], [], []
        for _ in range(a.reps):
            tr.scst_times, reward.host_seconds = {}, 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = tr.scst_step(batch)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            rows.append(dict(tr.scst_times))
            host.append(reward.host_seconds)
        tr.scst_times = None
        med = lambda k: round(1e3 * float(np.median([r.get(k, 0.0) for r in rows])), 3)
        print(json.dumps({"part": "scst", "baseline": baseline, "scst_rouge": rouge_w, "workload": "cfg2 shape: 256 images x 5 samples, max_len 30, V 10000, entropy weight 0.01",
                          "step_ms": round(1e3 * float(np.median(wall)), 3), "min_max_ms": [round(1e3 * min(wall), 3), round(1e3 * max(wall), 3)],
                          "sample_ms": med("sample"), "greedy_ms": med("greedy"), "reward_ms": med("reward"),
                          "reward_host_ms": round(1e3 * float(np.median(host)), 3), "upload_ms": med("upload"),
                          "policy_fwd_bwd_ms": med("policy_fwd_bwd"), "optimiser_ms": med("optimiser"),
                          "policy_T": int(tr.cap.T), "stats": st, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
