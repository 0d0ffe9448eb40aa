#!/usr/bin/env python
"""Headline benchmark: captions/sec of one full training step (forward + backward +
optimisers) of the CVAE captioning trainer on synthetic data resident in HBM.

  python bench.py --gpus N --steps K --warmup W [--workload cfg4|cfg2|cfg3|cfg1] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times K steps and prints the result line, nothing more.  --full adds everything else the benchmark
reports: the CPU baseline legs, the roofline of the dominant kernel family (HIP events live in the timed region), cfg4's strong_n1
point, cfg1's greedy-decode leg and the data-parallel bucket waits / compute-only step.  --dump-outputs DIR writes what the last
timed step computed as DIR/<name>.npy (training: the losses and a fixed, seeded sample of every parameter after the update;
cfg5: the kept beams' token ids and scores), so that two builds can be compared output for output.

Workloads (BASELINE.json configs):
  cfg4 (default, the configuration the metric is quoted on): Normal CVAE + --fine_tune,
        224x224 images, VGG16 on device, 64 images (320 caption rows) PER GPU, T=20, V=10000
        -> global batch 512 on 8 GPUs (weak scaling).
  cfg2: Normal CVAE, precomputed 4096-d features, 256 images (1280 rows) per GPU.
  cfg3: AG-CVAE with cluster vectors, 256 images per GPU.   cfg1: LSTM baseline, 32 images.
A "step" = one pass of the whole hot path over one batch.  One process per GPU: under
torch.distributed.run the ranks read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the env; a bare
`python bench.py --gpus N` (N > 1, no WORLD_SIZE) starts the N ranks itself.  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense fp32
PEAK_HBM_GBS = 8000.0

WORKLOADS = {
    "cfg1": dict(B=32, prior="Normal", no_encoder=True, use_c_v=False, fine_tune=False),
    "cfg2": dict(B=256, prior="Normal", no_encoder=False, use_c_v=False, fine_tune=False),
    "cfg3": dict(B=256, prior="AG", no_encoder=False, use_c_v=True, fine_tune=False),
    "cfg4": dict(B=64, prior="Normal", no_encoder=False, use_c_v=False, fine_tune=True),
    # generation (not a training step): GMM prior, beam width 5, 10 z samples, 128 images per batch
    "cfg5": dict(B=128, prior="GMM", no_encoder=False, use_c_v=False, fine_tune=False, generate=True, beam=5, z=10),
}
T_LEN, VOCAB = 20, 10000


def make_params(w):
    from vae_captioning_amd.utils.parameters import Parameters
    p = Parameters()
    p.prior, p.no_encoder, p.use_c_v, p.fine_tune = w["prior"], w["no_encoder"], w["use_c_v"], w["fine_tune"]
    p.batch_size = w["B"]
    p.vocab_size = VOCAB
    if w.get("generate"):
        p.mode, p.gen_z_samples, p.beam_size = "inference", w["z"], w["beam"]
    return p


DUMP_SAMPLE = 1 << 16   # --dump-outputs: arrays above this many elements are written as a fixed, seeded sample of this many


def _dump_sample(name, t):
    """All of `t` (a torch tensor or numpy array) as a flat float32 array if it is small, else DUMP_SAMPLE elements at sorted indices
    drawn from a generator seeded by the name alone (the same elements whatever the build); large device tensors are gathered on
    the device, so the full array never crosses to the host."""
    import zlib
    n = int(np.prod(t.shape))
    if n <= DUMP_SAMPLE:
        idx = None
    else:
        idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(n, DUMP_SAMPLE, replace=False))
    if isinstance(t, np.ndarray):
        flat = t.reshape(-1)
        return (flat if idx is None else flat[idx]).astype(np.float32)
    import torch
    flat = t.detach().reshape(-1)
    if idx is not None:
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat.float().cpu().numpy()


def _dump_name(name):
    return name.replace("/", "__")


def dump_training_outputs(d, tr, losses):
    """What a caller of the timed training step receives after the last step: the four losses (kld, rec_loss, lower_bound,
    annealing) as losses.npy (float64), and every trainable variable after the update (Trainer.state_dict's names; VGG16's
    straight from the device) as param__<scope>__<name>.npy -- whole up to DUMP_SAMPLE elements, a seeded sample above."""
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "losses.npy"), np.array(losses, dtype=np.float64))
    params = dict(tr.cap.state_dict())
    if tr.vgg is not None:
        params.update({n: tr.vgg.store.param(n) for n in tr.vgg.store.names()})
    for name in sorted(params):
        np.save(os.path.join(d, "param__%s.npy" % _dump_name(name)), _dump_sample(name, params[name]))


def dump_beams(d, res, beam):
    """cfg5: the last call's kept beams per image, descending score -- beam_ids.npy [images, beam, longest] (token ids as float32,
    -1 past a caption's end and for beams an image did not keep) and beam_scores.npy [images, beam] (float64, NaN where no beam)."""
    os.makedirs(d, exist_ok=True)
    L = max([len(s) for r in res for s, _ in r] + [1])
    ids = np.full((len(res), beam, L), -1.0, np.float32)
    scores = np.full((len(res), beam), np.nan, np.float64)
    for b, r in enumerate(res):
        for k, (s, sc) in enumerate(r[:beam]):
            ids[b, k, :len(s)] = s
            scores[b, k] = sc
    np.save(os.path.join(d, "beam_ids.npy"), ids)
    np.save(os.path.join(d, "beam_scores.npy"), scores)


def conv_flops_per_image():
    """Algorithmic MACs of the 13 convolutions per image."""
    from vae_captioning_amd import spec
    H = 224
    macs = {}
    for name, ci, co in spec.VGG_CONV:
        macs[name] = H * H * 9 * ci * co
        if name in spec.VGG_POOL_AFTER:
            H //= 2
    return macs


def conv_algorithmic_bytes(images):
    """Algorithmic HBM bytes of one cfg4 step's 3x3 convolution calls (fp32), the denominator of roofline.traffic_over_algorithmic:
      forward        x [B,H,W,Ci] read + y [B,H,W,Co] written (+ the pooled copy [B,H/2,W/2,Co] behind conv1_2 / 2_2 / 3_3 / 4_3 / 5_3:
                     the fused max-pool writes it from the same kernel) + the layer's 9 Ci Co weights + Co biases
      data gradient  dy [B,H,W,Co] read + dx [B,H,W,Ci] written + the ReLU source: 1 bit per element of dx (the producer's forward
                     leaves mask bits: the Winograd forwards and, since round 4, conv1_1's); none behind a pool (MaxPoolGrad applies
                     it); no data gradient for conv1_1
      weight grad    x and dy read, 9 Ci Co + Co written
    Saved activations are the forward's y (counted once, as its write); Winograd-transformed tensors never touch HBM and do not count;
    transformed WEIGHTS (16 Ci Co, re-packed once per step) count as the 9 Ci Co they stand for."""
    from vae_captioning_amd import spec
    H = 224
    tot = 0.0
    prev_pool = True   # conv1_1's input is the image: no data gradient
    first = True
    for name, ci, co in spec.VGG_CONV:
        px = float(images) * H * H
        wts = 9.0 * ci * co + co
        cie = 4 if ci == 3 else ci   # conv1_1 reads the NHWC4 image
        pooled = name in spec.VGG_POOL_AFTER
        tot += 4 * (px * cie + px * co + (px / 4 * co if pooled else 0) + wts)          # forward
        if not first:
            mask = 0.0 if prev_pool else px * ci / 8.0 / 4.0                             # bits (in units of 4 bytes; conv1_2's come from conv1_1's forward)
            tot += 4 * (px * co + px * ci + mask + wts)                                  # data gradient
        tot += 4 * (px * cie + px * co + wts)                                           # weight gradient
        first = False
        prev_pool = pooled
        if pooled:
            H //= 2
    return tot


def cpu_baseline(workload, w, seed):
    """Own CPU restatement (numpy oracle, NOT TF1 -- the reference cannot run here), timed on
    the host cores on a bounded sample of the same workload.  Uses oracle/ as the thing timed
    only for this reported baseline."""
    from oracle import caption_model as cm, optim as oo, vgg as ov
    from vae_captioning_amd import spec, synth
    p = make_params(w)
    rng = np.random.default_rng(seed)
    # cfg1 at its own batch (32); cfg2 / cfg3 on a reduced batch and step count; cfg4 measured at 8 images
    # (and, separately, extrapolated linearly to the 512-image global batch -- marked as extrapolated)
    Bc, warm, nsteps = {"cfg1": (32, 1, 5), "cfg2": (32, 1, 4), "cfg3": (16, 1, 4), "cfg4": (8, 1, 2)}[workload]   # (one warm-up step: the first one pays for page faults and BLAS thread start-up)
    P = spec.init_caption_params(p, VOCAB, seed=1)
    batch = synth.make_batch(rng, Bc, p.num_captions, T_LEN, VOCAB, use_ci=spec.uses_ci(p), images=p.fine_tune)
    noise = synth.make_noise(rng, Bc * p.num_captions, T_LEN, p)
    if p.prior == "AG":
        from oracle import decode
        noise["c_means"] = decode.init_clusters(90, p.latent_size)
    PV = spec.init_vgg_params(seed=2) if p.fine_tune else None
    st, stv = {}, {}
    t0 = time.perf_counter()
    for s in range(warm + nsteps):
        if s == warm:
            t0 = time.perf_counter()
        if p.fine_tune:
            d1 = (rng.random((Bc, 4096)) < 0.5).astype(np.float32)
            d2 = (rng.random((Bc, 4096)) < 0.5).astype(np.float32)
            fc2, cache = ov.forward(PV, batch["images"], d1, d2, keep=0.5)
            batch["features"] = fc2
        out = cm.forward_backward(P, batch, noise, p, global_step=s)
        norm = oo.global_norm(out.grads, out.sparse)
        oo.adam_step(P, out.grads, st, p.learning_rate, s + 1, scale=float(oo.clip_scale(norm, 5.0)))
        if p.fine_tune:
            GV = ov.backward(PV, cache, out.dfeatures)
            oo.adam_step(PV, GV, stv, p.cnn_lr, s + 1, l2=p.weight_decay)
    dt = time.perf_counter() - t0
    try:
        import threadpoolctl
        nthreads = max([i.get("num_threads", 1) for i in threadpoolctl.threadpool_info()] + [1])
    except Exception:
        nthreads = os.cpu_count()
    out = dict(value=round(Bc * p.num_captions * nsteps / dt, 3), unit="captions/s", cores=int(nthreads), kind="port",
               host_cpus=os.cpu_count(),
               sample="%d steps (after %d warm-up) of %s at %d images (%d caption rows)/step, numpy oracle (own CPU restatement, not TF1), %.1f s"
                      % (nsteps, warm, workload, Bc, Bc * p.num_captions, dt))
    if workload == "cfg4":
        out["extrapolated"] = {"seconds_per_512_image_step": round(dt / nsteps * 512 / Bc, 1),
                               "note": "EXTRAPOLATED linearly from the measured %d-image step to the 512-image global batch" % Bc}
    return out


def _blas_threads():
    try:
        import threadpoolctl
        return int(max([i.get("num_threads", 1) for i in threadpoolctl.threadpool_info()] + [1]))
    except Exception:
        return int(os.cpu_count() or 1)


def cpu_baseline_generate(kind, p, feats, cv, eps, beam=5, images=8):
    """BASELINE.md section 3's generation legs on the host: the numpy oracle's per-image decode (own CPU restatement of
    vae_model/decoder.py:145-320, NOT TF1) on the first `images` images of the batch the GPU decodes -- cfg1: greedy, 32 images;
    cfg5: beam search, 8 images.  Returns (cpu_baseline dict, the oracle's outputs for a token-id comparison in the same run)."""
    from oracle import decode as od
    from vae_captioning_amd import spec, synth
    P = spec.init_caption_params(p, VOCAB, seed=1)
    t0 = time.perf_counter()
    outs = []
    for b in range(images):
        e = eps[:, b:b + 1] if eps is not None else None
        c = cv[b] if cv is not None else None
        if kind == "greedy":
            outs.append(od.greedy(P, p, feats[b], c, e, synth.BOS, synth.EOS, max_len=p.gen_max_len))
        else:
            outs.append(od.beam_search(P, p, feats[b], c, e, synth.BOS, synth.EOS, beam_size=beam, max_len=p.gen_max_len)[0])
    dt = time.perf_counter() - t0
    return dict(value=round(images / dt, 3), unit="captions/s", cores=_blas_threads(), kind="port", host_cpus=os.cpu_count(),
                sample="%s decode of %d images (max %d tokens%s), numpy oracle per image in fp32 (own CPU restatement, not TF1), %.1f s"
                       % (kind, images, p.gen_max_len, ", beam %d x %d z samples" % (beam, p.gen_z_samples) if kind == "beam" else "", dt)), outs


def main():
    # multi-process GPU work: the host driver only supports dmabuf IPC (without this RCCL's peer mappings fail with
    # "hipIpcGetMemHandle: invalid argument"); exported by the launch environment, defaulted here for bare invocations
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="cfg4", choices=sorted(WORKLOADS))
    ap.add_argument("--graph", type=int, default=0,
                    help="1: replay the step from a captured hipGraph (single GPU).  Default 0: eager launches, so the "
                         "dominant kernels can be bracketed by HIP events inside the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--strong-n1", type=int, default=1,
                    help="with --full, cfg4 at N = 1 (weak): after the timed region also run the 512-image GLOBAL batch on this one GPU (3 warm-up + 10 timed "
                         "steps, ~3 s) and report it as `strong_n1` -- SURVEY.md section 8d's single-GPU point of the strong-scaling curve")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--images-per-gpu", type=int, default=0, help="override the workload's images per GPU (sweeps; the default is BASELINE's)")
    ap.add_argument("--fresh-batch", type=int, default=0, metavar="K",
                    help="rotate K distinct host batches through Trainer.set_batch INSIDE the timed region (token upload, device index "
                         "build for the embedding gradient, image upload from pinned memory), i.e. the step main.py runs; 0 = one "
                         "HBM-resident batch (the headline figure: inputs resident when the timed region starts)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: the workload's images per GPU on every rank (global batch grows with N); strong: the GLOBAL batch is "
                         "fixed at 8 x the per-GPU figure (cfg4: 512 images) and divided over the ranks")
    ap.add_argument("--vocab", type=int, default=VOCAB, help="vocabulary size (secondary lines: 11313 = the reference's observed size)")
    ap.add_argument("--variable-len", action="store_true", help="caption lengths ~ clip(N(11,3), 6, 20) instead of all 20 (secondary line)")
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16x3"],
                    help="f32 (default, the reference's arithmetic: the headline line) or bf16x3: every dense product with operands split into "
                         "(hi, lo) bf16 pairs, three bf16 MFMAs per k-step, f32 accumulate (~1e-5 relative product error) -- a separately "
                         "reported line, never the default")
    ap.add_argument("--num-captions", type=int, default=0, help="captions per image (secondary line nc = 1; default: the reference's 5)")
    ap.add_argument("--full", action="store_true",
                    help="also run and report everything beyond the headline figure: CPU baselines (unless --no-cpu-baseline), the "
                         "roofline from HIP events in the timed region, strong_n1 (cfg4, unless --strong-n1 0), cfg1's greedy leg, the "
                         "data-parallel bucket waits and compute-only step")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed as DIR/<name>.npy (float32 / float64, a seeded sample "
                         "of large arrays; rank 0)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)

    import torch
    import torch.distributed as dist
    from vae_captioning_amd import abi, spec, synth
    from vae_captioning_amd.trainer import Trainer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with --nproc-per-node %d, or without a launcher)" % (args.gpus, world, args.gpus))
    # one process per GPU.  (VC_DIST_BACKEND=gloo lets two ranks share ONE GPU: used only by the
    # single-GPU test of the N > 1 code path, tests/test_gpu_cli.py.)
    backend = os.environ.get("VC_DIST_BACKEND", "nccl")
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    if local >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d wants GPU %d but this node shows %d (one process per GPU; --gpus %d needs %d GPUs)" % (
            rank, local, torch.cuda.device_count(), args.gpus, args.gpus))
    torch.cuda.set_device(local)
    lib = abi.load()  # raises if the HIP library is missing: no fallback
    lib.vc_device_check(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    w = dict(WORKLOADS[args.workload])
    if args.images_per_gpu:
        w["B"] = args.images_per_gpu
    if args.scaling == "strong":  # "1/2/4-GPU points ... at B=512 total (strong)"
        assert (8 * w["B"]) % world == 0
        w["B"] = 8 * w["B"] // world
    p = make_params(w)
    if args.num_captions:
        p.num_captions = args.num_captions
    # The CPU baseline leg (rank 0, N = 1) runs FIRST: the GPU's timed region is then the last thing the process does (a driver
    # that samples GPU activity over the whole run otherwise sees mostly the numpy baseline).
    cpu_base = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not w.get("generate"):
        cpu_base = cpu_baseline(args.workload, w, args.seed)
    vocab = args.vocab
    p.vocab_size = vocab
    if w.get("generate"):
        return bench_generation(args, torch, dist, lib, w, p, world, rank)
    rng = np.random.default_rng(args.seed + rank)
    B = w["B"]
    N = B * p.num_captions
    tr = Trainer(p, vocab, device="cuda", lib=lib, world=world, rank=rank, seed=args.seed, precision=args.precision)
    tr.load_state_dict({**spec.init_caption_params(p, vocab, seed=1), **(spec.init_vgg_params(seed=2) if p.fine_tune else {})})
    # (--fresh-batch: host batches carry uint8 pixels like the reference's HDF5 file; the resident headline batch is the float32 feed)
    mk = lambda: synth.make_batch(rng, B, p.num_captions, T_LEN, vocab, use_ci=spec.uses_ci(p), images=("u8" if args.fresh_batch else True) if p.fine_tune else False,
                                  variable_len=args.variable_len)
    batch = mk()
    fresh = [batch] + [mk() for _ in range(max(0, args.fresh_batch - 1))] if args.fresh_batch else None
    tr.set_batch(batch)  # inputs resident in HBM before the timed region; noise is generated on device

    from vae_captioning_amd.engine import KernelTimer
    use_graph = bool(args.graph) and world == 1
    for i in range(args.warmup):
        if fresh:
            tr.set_batch(fresh[i % len(fresh)])
        tr._step()
    timer = KernelTimer(all_gemms=tr.vgg is None) if args.full else None   # caption-only workloads: the dominant family is every dense product of the step
    if use_graph:
        tr.capture(warmup=0)
    elif timer is not None:  # HIP-event pairs around the dominant kernel launches, live in the timed region
        tr.cap.timer = timer
        if tr.vgg is not None:
            tr.vgg.timer = timer
    if world > 1 and args.full:
        tr.dp_stats = []
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if fresh:
            tr.set_batch(fresh[i % len(fresh)])
        tr.train_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    kld, rec, lb, ann = tr.losses()
    assert np.isfinite(rec) and np.isfinite(lb), "non-finite loss"
    if args.dump_outputs and rank == 0:   # before anything below runs another step
        dump_training_outputs(args.dump_outputs, tr, (kld, rec, lb, ann))
    dp_info = None
    if world > 1:  # per-bucket stall of the compute stream on the gradient all-reduce (ms per step, mean over the timed steps)
        from vae_captioning_amd import dp as dpm
        bk = dpm.gradient_buckets(tr.n_cap, tr.gall.numel(), tr.off_fc, tr.off_c3)
        dp_info = {"backend": backend, "rccl_world_size": dist.get_world_size(), "all_reduce_bytes_per_step": int(tr.gall.numel() * 4),
                   "collectives": ("libvaecap C ABI (vc_allreduce_sum_f32 / vc_allgather_f32 / vc_reducescatter_sum_f32), RCCL %d" % tr.comm.rccl_version)
                                  if tr.comm is not None else "torch.distributed (%s)" % backend,
                   "buckets_bytes": [int((b - a) * 4) for a, b in bk] if (tr.buckets and tr.vgg is not None) else [int(tr.gall.numel() * 4)]}
        if tr.dp_stats:
            torch.cuda.synchronize()
            waits = {}
            for i, nbytes, e0, e1 in tr.dp_stats:
                waits.setdefault(i, []).append(e0.elapsed_time(e1))
            dp_info["bucket_wait_ms"] = [round(float(np.mean(waits[i])), 4) for i in sorted(waits)]
    if world > 1 and args.full:
        # exposed communication = step - compute-only step (the same step with every collective muted), max over ranks like the step time
        tr.dp_stats = None
        restore = tr.mute_collectives()
        nco = max(5, args.steps // 5)
        for _ in range(2):
            tr.train_step()
        torch.cuda.synchronize()
        dist.barrier()
        t1 = time.perf_counter()
        for _ in range(nco):
            tr.train_step()
        torch.cuda.synchronize()
        tco = torch.tensor([time.perf_counter() - t1], device="cuda", dtype=torch.float64)
        restore()
        dist.all_reduce(tco, op=dist.ReduceOp.MAX)
        dp_info["compute_only_ms_per_step"] = round(1000 * float(tco.item()) / nco, 3)
        dp_info["exposed_comm_ms"] = round(1000 * dt / args.steps - dp_info["compute_only_ms_per_step"], 3)

    # ---- roofline of the dominant kernel family from the HIP events of the timed region
    roof = roofline_figures(args, tr, timer, B, use_graph) if args.full else None
    out = {
        "metric": "captions/sec training (224x224, seq20, vocab~10k)",
        "value": round(N * world * args.steps / dt, 2),
        "unit": "captions/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1000 * dt / args.steps, 3),
        "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f32" if args.precision == "f32" else ("bf16x3 split operands, f32 accumulate (dense products, LSTM recurrence products" + (", VGG16 weight gradients; forward / data-gradient convolutions f32 Winograd" if p.fine_tune else "") + "; element-wise work in f32)"),
        "data": "synthetic",
        "config": {"workload": "%s: %s" % (args.workload, json.dumps(w, sort_keys=True)), "images_per_gpu": B, "precision": args.precision,
                   "captions_per_image": p.num_captions, "caption_rows_per_gpu": N, "global_caption_rows": N * world,
                   "seq_len": T_LEN, "vocab": vocab, "variable_len": bool(args.variable_len), "gen_z_samples": p.gen_z_samples,
                   "hipgraph": use_graph, "parallelism": "dp%d" % world, "rccl_world_size": dist.get_world_size() if world > 1 else 1,
                   "inputs": ("%d host batches rotated through set_batch inside the timed region" % len(fresh)) if fresh
                             else "one batch resident in HBM"},
        "final_losses": {"rec_loss": round(rec, 5), "kld": round(kld, 5)},
    }
    if roof is not None:
        out["roofline"] = roof
    if dp_info:
        out["data_parallel"] = dp_info
    if cpu_base is not None:
        out["cpu_baseline"] = cpu_base
    if args.full and world == 1 and args.workload == "cfg1" and p.no_encoder:
        out["greedy_decode"] = greedy_leg(args, lib, w, p, vocab, tr, with_cpu=(rank == 0 and not args.no_cpu_baseline))
    if args.full and world == 1 and args.workload == "cfg4" and args.scaling == "weak" and args.strong_n1 and not args.images_per_gpu and not use_graph:
        del tr
        torch.cuda.empty_cache()
        out["strong_n1"] = strong_n1_point(args, lib, w, vocab)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def roofline_figures(args, tr, timer, B, use_graph):
    """--full: the roofline of the dominant kernel family from the HIP events of the timed region (graph replays carry none:
    one extra eager, instrumented pass), the HBM-bound kernels, and the traffic replayed from profiles/traffic_<workload>.json."""
    instrumented_pass = False
    if use_graph:  # events cannot be recorded inside a replayed graph: one extra eager, instrumented pass
        instrumented_pass = True
        tr.graph = None
        tr.cap.timer = timer
        if tr.vgg is not None:
            tr.vgg.timer = timer
        for _ in range(max(2, args.steps // 4)):
            tr._step()
    roof = roofline_from_timer(timer, tr.vgg is not None, B, precision=args.precision)
    roof["instrumented_pass"] = instrumented_pass
    roof["hbm_kernels"] = hbm_from_timer(timer)
    # HBM-side bytes per launch of the same kernels, from the rocprofv3 --pmc passes of this command
    # (profiles/, FETCH_SIZE x2 gfx950 correction + WRITE_SIZE); cannot be collected from inside the process.
    tj = os.path.join(ROOT, "profiles", "traffic_%s.json" % args.workload)
    if os.path.exists(tj):
        t = json.load(open(tj))
        # PMC bytes are per STEP (the launch count per step depends on VC_VGG_STREAMS: half-batch launches)
        roof["traffic"] = round(t["bytes_per_step"] * (max(2, args.steps // 4) if instrumented_pass else args.steps) / roof["launches"]) if "bytes_per_step" in t else t.get("bytes_per_launch")
        # NOT measured by this process: PMC counters need rocprofv3 around the command.  The figure is replayed from the tracked file.
        roof["traffic_source"] = "replayed from profiles/traffic_%s.json (rocprofv3 --pmc passes of this command, tools/collect_profiles.sh): %s" % (args.workload, t.get("source"))
        if roof.get("traffic") and tr.vgg is not None:
            # algorithmic bytes of one step's convolution calls (every call reads its input tensor and writes its
            # output tensor once, + the ReLU source of a data gradient, the pooled copy of a pooled forward, the 3x3 weights)
            alg = conv_algorithmic_bytes(B)
            nsteps_t = max(2, args.steps // 4) if instrumented_pass else args.steps
            roof["algorithmic_bytes_per_launch"] = round(alg * nsteps_t / roof["launches"])
            roof["traffic_over_algorithmic"] = round(roof["traffic"] / roof["algorithmic_bytes_per_launch"], 3)
    return roof


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU under torch.distributed.run,
    rendezvous on 127.0.0.1 at a free port) with the same arguments; rank 0's JSON line is the only thing on stdout, the exit code is
    the launcher's."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")
    sys.exit(subprocess.call(cmd, env=env))


def strong_n1_point(args, lib, w, vocab, steps=10, warmup=3):
    """The 512-image global batch of cfg4 on ONE GPU (the N = 1 point of the strong-scaling curve): a fresh
    Trainer at 8 x the per-GPU batch, `warmup` untimed + `steps` timed steps in the same process as the headline line."""
    import torch
    from vae_captioning_amd import spec, synth
    from vae_captioning_amd.trainer import Trainer
    w8 = dict(w)
    w8["B"] = 8 * w["B"]
    p = make_params(w8)
    rng = np.random.default_rng(args.seed + 512)
    tr = Trainer(p, vocab, device="cuda", lib=lib, seed=args.seed)
    tr.load_state_dict({**spec.init_caption_params(p, vocab, seed=1), **spec.init_vgg_params(seed=2)})
    tr.set_batch(synth.make_batch(rng, w8["B"], p.num_captions, T_LEN, vocab, use_ci=spec.uses_ci(p), images=True))
    for _ in range(warmup):
        tr.train_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kld, rec, lb, ann = tr.losses()
    assert np.isfinite(rec) and np.isfinite(lb), "non-finite loss"
    N = w8["B"] * p.num_captions
    return {"images": w8["B"], "caption_rows": N, "steps": steps, "warmup": warmup, "ms_per_step": round(1000 * dt / steps, 3),
            "value": round(N * steps / dt, 2), "unit": "captions/s",
            "note": "cfg4's 512-image GLOBAL batch on one GPU (strong scaling, N = 1); calls over the 2 GiB buffer range run as launches over image ranges"}


def bench_generation(args, torch, dist, lib, w, p, world, rank):
    """cfg5: beam-search caption generation throughput (captions = images per second); replicas only --
    images are independent, no collective."""
    from vae_captioning_amd import spec, synth
    from vae_captioning_amd.engine import CaptionEngine, KernelTimer
    from vae_captioning_amd.generate import CaptionGenerator
    rng = np.random.default_rng(args.seed + rank)
    eng = CaptionEngine(p, VOCAB, lib=lib, seed=args.seed)
    eng.load_params(spec.init_caption_params(p, VOCAB, seed=1))
    gen = CaptionGenerator(eng)
    B = w["B"]
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, 4096), dtype=np.float32), 0)).cuda()
    cv = np.zeros((B, 90), np.float32)
    eps = rng.standard_normal((p.gen_z_samples, B, p.latent_size), dtype=np.float32)   # injected noise: the CPU leg decodes the SAME captions
    cpu_base = cpu_ids = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:   # first, so that the GPU's timed region is the last thing the process does
        cpu_base, cpu_ids = cpu_baseline_generate("beam", p, feats.cpu().numpy(), cv, eps, beam=w["beam"], images=8)
    run = lambda: gen.beam_search(feats, cv, eps, synth.BOS, synth.EOS, beam_size=w["beam"], max_len=p.gen_max_len)
    for _ in range(args.warmup):
        run()
    if args.full:
        eng.timer = KernelTimer(all_gemms=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_beams(args.dump_outputs, res, w["beam"])
    roof = None
    if args.full:
        roof = roofline_from_timer(eng.timer, False)
        roof["instrumented_pass"] = False
        roof["note"] += ("; cfg5: decoder rounds replayed from hipGraphs carry no events -- the bracketed launches are each call's LAST round (run eagerly: "
                         "29 rounds = 7 replayed chunks of 4 + 1) of both image slices, whose logits products [320, 512] x [512, V] share the CUs with the "
                         "other slice's kernels (two streams), and the small products outside the rounds; every kernel's in-graph duration is in "
                         "profiles/r06_cfg5_kernel_stats.md")
    out = {"metric": "captions/sec generated (beam search)", "value": round(B * world * args.steps / dt, 2), "unit": "captions/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1000 * dt / args.steps, 3),
           "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "cfg5: %s" % json.dumps(w, sort_keys=True), "images_per_gpu": B, "beam_size": w["beam"],
                      "gen_z_samples": w["z"], "gen_max_len": p.gen_max_len, "vocab": VOCAB, "parallelism": "replicas%d" % world,
                      "mean_caption_len": round(float(np.mean([len(r[0][0]) for r in res])), 2)}}
    if roof is not None:
        out["roofline"] = roof
    if cpu_base is not None:
        # (random-init weights give near-uniform word distributions: a beam may legitimately differ where fp32 and the oracle's
        # arithmetic order disagree in the last bit; the parity tests use peaked weights -- this is a report, not a gate)
        cpu_base["beams_identical_to_gpu"] = "%d of %d images" % (sum([s for s, _ in res[b]] == cpu_ids[b] for b in range(len(cpu_ids))), len(cpu_ids))
        out["cpu_baseline"] = cpu_base
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def cpu_baseline_greedy(P, p, feats, gpu_ids):
    """cfg1's greedy leg on the host: the numpy oracle decodes the same images with the same parameters (per image, fp32)."""
    from oracle import decode as od
    from vae_captioning_amd import synth
    B = feats.shape[0]
    t0 = time.perf_counter()
    ref = [od.greedy(P, p, feats[b], None, None, synth.BOS, synth.EOS, max_len=p.gen_max_len) for b in range(B)]
    dc = time.perf_counter() - t0
    return dict(value=round(B / dc, 3), unit="captions/s", cores=_blas_threads(), kind="port", host_cpus=os.cpu_count(),
                sample="greedy decode of the same %d images with the same parameters, numpy oracle per image in fp32 "
                       "(own CPU restatement, not TF1), %.1f s" % (B, dc),
                token_ids_identical_to_gpu="%d of %d images" % (sum(a == b for a, b in zip(gpu_ids, ref)), B))


def greedy_leg(args, lib, w, p, vocab, tr, with_cpu):
    """cfg1's decode leg ("+ greedy decode of 32 images, max 30 tokens"): the trained-in-place parameters of
    the Trainer decode the batch's 32 images on the device (vae_model/decoder.py:145-201); reported beside the training line."""
    import torch
    from vae_captioning_amd import synth
    from vae_captioning_amd.generate import CaptionGenerator
    gen = CaptionGenerator(tr.cap)
    B = w["B"]
    rng = np.random.default_rng(args.seed + 77)
    feats = np.maximum(rng.standard_normal((B, 4096), dtype=np.float32), 0)
    fd = torch.from_numpy(feats).cuda()
    run = lambda: gen.greedy(fd, None, None, synth.BOS, synth.EOS, max_len=p.gen_max_len)
    for _ in range(3):
        ids = run()
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        ids = run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    out = {"images": B, "max_len": p.gen_max_len, "ms_per_batch": round(1000 * dt, 3), "value": round(B / dt, 1), "unit": "captions/s generated (greedy)",
           "mean_caption_len": round(float(np.mean([len(r) for r in ids])), 2)}
    if with_cpu:
        out["cpu_baseline"] = cpu_baseline_greedy(tr.state_dict(), p, feats, ids)
    return out


def hbm_from_timer(timer):
    """The HBM-bound kernels of the path (embedding gather, softmax cross-entropy, optimiser update, and cfg4's three fc1 products:
    a [64, 25088] x [25088, 4096] GEMM moves its 411 MB weight matrix -- or writes its gradient -- once per call): algorithmic bytes
    (fc1: weight matrix + both activations) / HIP-event duration, against the 8 TB/s HBM3E peak of
    MI355X_MICROARCH.md."""
    sm = timer.summary()
    out = {}
    # (fc1_gemm: the forward product, alone on the chip; fc1_gemm_bwd: its two backward products, which share the chip with the logits
    # layer's weight gradient on the weight-gradient stream since round 4 -- their event pairs include that)
    for tag in ("hbm_embedding_gather", "hbm_softmax_xent", "hbm_adam", "hbm_fc1_gemm", "hbm_fc1_gemm_bwd"):
        if tag in sm and sm[tag]["seconds"] > 0:
            gbs = sm[tag]["flops"] / sm[tag]["seconds"] / 1e9
            out[tag[4:]] = {"launches": sm[tag]["launches"], "avg_us": round(1e6 * sm[tag]["seconds"] / sm[tag]["launches"], 2),
                            "achieved_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / 8000.0, 3)}
    return out


def _cdiv(a, b):
    return (a + b - 1) // b


def wino_executed_ratio(images, wino4=True, with_wgrad=True):
    """Executed MFMA FLOPs / algorithmic FLOPs of one cfg4 step's 3x3 convolution calls when the Winograd kernels run (default):
    F(2x2,3x3) / F(3x3,2x2) multiply 16 times per 2x2 tile and channel pair where the direct form multiplies 36 times, F(4x4,3x3) 36
    times per 4x4 tile where the direct form multiplies 144 times; tile blocks that stick out of the image add padding work.  Forward /
    data gradient: F(4x4,3x3) on blocks of 16 x 16 pixels (csrc/conv_wino4.hip) where vc_conv3x3_wino4_preferred says so -- since round 4
    every VGG16 layer behind conv1_1 --, else F(2x2,3x3) on blocks of 16 tile slots whose halo patch fits 100 pixels
    (csrc/conv_wino.hip plan_wino2); weight gradient (conv_wino_wgrad.hip
    plan_wino_wgrad): F(3x3,2x2) on 4x8 / 4x7 / 2x14 tiles.  conv1_1 (3 input channels) stays on its direct HBM-bound kernels."""
    from vae_captioning_amd import abi, spec
    prefers4 = abi.load().vc_conv3x3_wino4_preferred   # the library's own rule (block coverage; csrc/conv_wino4.hip)
    slots, maxpix = 16, 100
    H = 224
    alg = ex = 0.0
    for name, ci, co in spec.VGG_CONV:
        th = tw = H // 2
        fl = 2.0 * images * H * H * 9 * ci * co
        if ci == 3:
            alg += (2 if with_wgrad else 1) * fl
            ex += (2 if with_wgrad else 1) * fl
        else:
            best = 0.0   # forward / data gradient: the block shape with the fewest empty slots
            for tbw in range(1, min(16, tw) + 1):
                tbh = min(slots // tbw, th)
                if tbh < 1 or (2 * tbh + 2) * (2 * tbw + 2) > maxpix:
                    continue
                best = max(best, tw * th / (_cdiv(tw, tbw) * _cdiv(th, tbh) * float(slots)))
            effw = max(tw * th / (_cdiv(tw, bw) * _cdiv(th, bh) * float(bh * bw)) for bh, bw in ((4, 8), (4, 7), (2, 14)))
            eff4 = H * H / (_cdiv(H, 4) ** 2 * 16.0) if _cdiv(images * _cdiv(H, 4) ** 2, 16) < images * _cdiv(H, 16) ** 2 else H * H / (_cdiv(H, 16) ** 2 * 256.0)   # linear tiles (csrc/conv_wino4.hip plan_wino4) / square blocks
            fd = (36.0 / 144.0) / eff4 if (wino4 and prefers4(images, H, H, ci, co)) else (16.0 / 36.0) / best
            alg += (3 if with_wgrad else 2) * fl
            ex += 2 * fl * fd + (fl * (16.0 / 36.0) / effw if with_wgrad else 0.0)
        if name in spec.VGG_POOL_AFTER:
            H //= 2
    return ex / alg


PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16, dense


def roofline_from_timer(timer, fine_tune, images=0, precision="f32"):
    """Dominant kernel family: cfg4 = the 3x3 convolution calls (forward, data gradient, weight gradient; a call = its main
    launch + split reduce); caption-only workloads = the [T*N, H] x [H, V] logits GEMM.
      achieved / frac                     = the FLOPs the MFMAs EXECUTE (Winograd: 16 multiplications where the direct form has 36, plus
                                            tile-block padding) / UNION of the calls' HIP-event intervals, over the dense fp32 MFMA peak:
                                            the matrix-pipe utilisation, a fraction of the roofline
      frac_serial                         = the same FLOPs / SUM of the calls' durations (equal to frac on one stream)
      effective_tflops / frac_algorithmic = ALGORITHMIC (direct-convolution) FLOPs / the same union time: may exceed
                                            the peak -- the Winograd kernels do the algorithm's work with 2.25x fewer multiplications (fp32)
    Both are recomputable from the tracked rocprofv3 summary of the same command (profiles/*_kernel_stats.md ends with the family's
    summed and union dispatch time, tools/rocpd_stats.py)."""
    # split-bf16 mode with VGG16 fine-tuning: the weight gradients run on the bf16 pipe (csrc/conv_wgrad_bx.hip) -- the f32 family is the
    # F(4x4,3x3) forward / data gradient alone, the weight gradient is priced separately below ("wgrad_bf16_pipe")
    bxw = bool(fine_tune) and precision == "bf16x3" and os.environ.get("VC_WGRAD_BX", "1") != "0" and os.environ.get("VC_CONV_WINO", "1") != "0"
    # caption-only workloads: EVERY dense product the step issues through vc_gemm_f32 (the logits trio, the Normal / AG / GMM heads --
    # cfg3's [N, 512] x [512, 27000] --, z_rnn, imf_emb / cv_emb, their data and weight gradients); the products inside vc_lstm_seq_*
    # (input projections, dW) are issued by the library and not bracketed.  The rocprofv3 family "GEMM" of profiles/*_kernel_stats.md
    # holds both, so its union is an upper bound of family_seconds_union.
    tags = (["conv_fwd", "conv_dgrad"] if bxw else ["conv_fwd", "conv_dgrad", "conv_wgrad"]) if fine_tune else ["logits_gemm", "gemm"]
    if not fine_tune and "gemm" not in timer.summary():
        tags = ["logits_gemm"]
    sm = timer.summary(family=tags)
    wg = timer.summary(family=["conv_wgrad"]) if bxw else None
    fl = sum(sm[t]["flops"] for t in tags)
    sec = sm["__union__"]
    ser = sum(sm[t]["seconds"] for t in tags)
    n = sum(sm[t]["launches"] for t in tags)
    ach = fl / sec / 1e12
    per = {t: dict(launches=sm[t]["launches"], avg_us=round(1e6 * sm[t]["seconds"] / sm[t]["launches"], 2),
                   tflops=round(sm[t]["flops"] / sm[t]["seconds"] / 1e12, 2)) for t in tags}
    wino = fine_tune and os.environ.get("VC_CONV_WINO", "1") != "0"
    ratio = wino_executed_ratio(images, with_wgrad=not bxw) if (wino and images) else 1.0
    if not fine_tune and precision == "bf16x3":
        # the logits product on the bf16 matrix pipe: three bf16 MFMAs per algorithmic MAC, priced against the dense bf16 peak
        return {"bound": "mfma", "kernel": "vc::gemm_bx_kernel (every dense product of the step issued through vc_gemm_f32: logits trio, heads, projections; split-bf16: hi.hi + hi.lo + lo.hi)",
                "achieved": round(3 * ach, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(3 * ach / PEAK_BF16_MFMA_TFLOPS, 4),
                "effective_tflops": round(ach, 2), "executed_over_algorithmic": 3.0,
                "family_flops": fl, "family_seconds_union": round(sec, 6), "family_seconds_serial": round(ser, 6),
                "traffic": None, "launches": n, "avg_launch_us": round(1e6 * sec / n, 2), "per_kernel": per, "streams": 1,
                "note": "achieved = 3 x algorithmic FLOPs of the dense products in the timed region (each MAC is three bf16 MFMA MACs) / "
                        "HIP-event time, against the dense bf16 MFMA peak; effective_tflops = the algorithmic rate (f32 MFMA peak: 157.3)"}
    if not fine_tune:
        kern = ("vc::gemm_kernel (every dense product the step issues through vc_gemm_f32: logits forward / data gradient / weight gradient, "
                "the latent heads, z_rnn, imf_emb / cv_emb and their gradients; per_kernel splits the logits forward from the rest)")
    elif wino:
        kern = ("vc::conv_wino4_kernel (Winograd F(4x4,3x3) forward / data gradient of conv1_2 ... conv5_3) / "
                "vc::wino_wgrad_kernel (F(3x3,2x2) weight gradient) (+ vc::conv1_fwd_kernel / vc::conv1_wgrad_kernel for conv1_1)")
    else:
        kern = "vc::conv_kernel<fwd|dgrad|wgrad> (NHWC implicit GEMM behind layout conversions: the checker path)"
    ex = ach * ratio
    extra = {}
    if bxw:
        kern = ("vc::conv_wino4_kernel (Winograd F(4x4,3x3) forward / data gradient of conv1_2 ... conv5_3, f32; + vc::conv1_fwd_kernel) -- the weight "
                "gradients of this mode run on the bf16 pipe: wgrad_bf16_pipe")
        w = wg["conv_wgrad"]
        extra["wgrad_bf16_pipe"] = {
            "kernel": "vc::wgrad_bx_kernel (direct, split-bf16: three bf16 MFMAs per algorithmic MAC; + vc::conv1_wgrad_kernel for conv1_1, f32)",
            "achieved": round(3 * w["flops"] / w["seconds"] / 1e12, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": round(3 * w["flops"] / w["seconds"] / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4), "effective_tflops": round(w["flops"] / w["seconds"] / 1e12, 2),
            "launches": w["launches"], "avg_launch_us": round(1e6 * w["seconds"] / w["launches"], 2),
            "note": "3 x algorithmic FLOPs of the weight-gradient calls / the SUM of their HIP-event durations (they run beside the data-gradient "
                    "chains on another stream: a call's duration includes what it loses to them); DESIGN.md section 4d: on real data the bf16 "
                    "pipe is power-limited to ~0.5 of this peak"}
    return {**extra, "bound": "mfma", "kernel": kern,
            # achieved / frac: the FLOPs the MFMAs EXECUTE per second against the dense fp32 MFMA peak (a fraction of the roofline, < 1)
            "achieved": round(ex, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(ex / PEAK_F32_MFMA_TFLOPS, 4),
            "frac_serial": round(fl * ratio / ser / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
            # the same time against the ALGORITHMIC (direct-convolution) FLOPs of SURVEY.md section 8d: what a direct kernel would have to sustain
            "effective_tflops": round(ach, 2), "frac_algorithmic": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
            "executed_over_algorithmic": round(ratio, 4),
            "family_flops": fl, "family_seconds_union": round(sec, 6), "family_seconds_serial": round(ser, 6),
            "traffic": None, "launches": n, "avg_launch_us": round(1e6 * sec / n, 2), "per_kernel": per,
            "streams": int(os.environ.get("VC_VGG_STREAMS", "3")) if fine_tune else 2,
            "note": ("achieved = algorithmic FLOPs (2 M N K) of every vc_gemm_f32 call the step issues (tags logits_gemm + gemm; the products inside "
                     "vc_lstm_seq_* are issued by the library and not bracketed) / union of the calls' HIP-event intervals, recorded on the stream each "
                     "call is launched on (the weight-gradient products run on a second stream); frac = achieved / the dense f32 MFMA peak") if not fine_tune else
                    "achieved = EXECUTED MFMA FLOPs of the family's calls in the timed region (Winograd, fp32: F(4x4,3x3) 36 multiplications per "
                    "4x4 tile and channel pair where the direct form has 144, F(2x2,3x3) / F(3x3,2x2) 16 per 2x2 tile where it has 36, + tile-block "
                    "padding; = algorithmic FLOPs x "
                    "executed_over_algorithmic) / union of the calls' HIP-event intervals (events recorded on the stream each call is "
                    "launched on); frac = achieved / peak = matrix-pipe utilisation.  effective_tflops / frac_algorithmic price the same "
                    "time against the direct-convolution FLOPs (> peak is possible: fewer multiplications, not a faster pipe)"}


if __name__ == "__main__":
    main()
