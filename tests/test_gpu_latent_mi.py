"""-m gpu: mutual information under the aggregated posterior -- vc_gauss_mix_lse_f64 (csrc/latent_mi.hip) against the float64 reference
tests/latent_mi_ref.py at every size where the kernel takes another path, its contracts (a caption's bits depend on the caption and the
table only, two calls agree, inputs and the memory behind the outputs stay), latent_mi.mutual_information against the reference and on
tables whose answer is known, and --bound_mi on the command line.

The kernel's sizes (csrc/latent_mi.hip): chunks of 64 posteriors, tiles of 32 latent dimensions, 16 rows per wave and 128 / S captions
per workgroup from S = 8 on, 8 rows per wave and 64 / S captions below, S <= 128.

Tolerance |dev - ref| <= 1e-9 * max(1, |ref|): every term and every sum is float64 on identical inputs; device and reference differ in
the order of the sums (at most L + M terms, a relative 2^-53 each), in one more rounding per term ((z - mean) * (1 / std) for
(z - mean) / std) and in a few ulp of exp / log: below 1e-12 at these sizes.  1e-9 leaves three orders of magnitude and is still far
below anything a float32 shortcut would give."""
import json
import math
import os

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, latent_mi, spec, synth
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.utils.parameters import Parameters

from . import latent_mi_ref as ref
from .test_gpu_score import _main

pytestmark = pytest.mark.gpu
TOL = 1e-9
SENTINEL = -7.25


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("%s: max |dev - ref| / max(1, |ref|) = %.3e" % (what, err.max() if err.size else 0.0))
    assert (err <= TOL).all(), (what, float(err.max()))


def _table(rng, M, L, std=None):
    mean = rng.standard_normal((M, L)).astype(np.float32)
    sd = np.exp(rng.uniform(math.log(1e-3), math.log(10.0), (M, L))).astype(np.float32) if std is None else np.full((M, L), std, np.float32)
    return mean, sd


def _draws(rng, N, S, mean, std, owner=None):
    """z [N, S, L]: caption n drawn from posterior owner[n] (n mod M when not given)"""
    own = np.arange(N) % mean.shape[0] if owner is None else np.asarray(owner)
    return ref.draws(mean[own], std[own], rng.standard_normal((N, S, mean.shape[1])))


def _run(lib, z, mean, std):
    """the C ABI on uploaded copies -> (lse_block [N, S], lse_full [N]); the inputs must come back unchanged and the float64 just past
    either output must keep its sentinel"""
    from .gpu_util import P, dev, host, stream
    N, S, L = z.shape
    zd, md, sd = dev(z), dev(mean), dev(std)
    blk = torch.full((N * S + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    full = torch.full((N + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    lib.vc_gauss_mix_lse_f64(stream(), N, mean.shape[0], S, L, P(zd), P(md), P(sd), P(blk), P(full))
    b, f = host(blk), host(full)
    assert b[-1] == SENTINEL and f[-1] == SENTINEL
    assert np.array_equal(host(zd), z) and np.array_equal(host(md), mean) and np.array_equal(host(sd), std)
    return b[:-1].reshape(N, S), f[:-1]


# ------------------------------------------------------------------ the kernel against the reference
SHAPES = [(1, 1, 1, 1), (3, 5, 2, 3), (5, 65, 3, 150), (7, 130, 10, 150), (70, 257, 1, 7), (4, 1000, 10, 20),
          # chunks of 64 posteriors, tiles of 32 dimensions
          (3, 63, 2, 31), (3, 64, 2, 32), (3, 128, 2, 33), (2, 129, 9, 64), (2, 3, 4, 65),
          # captions per workgroup: 64 / S below S = 8, 128 / S from there on (S = 1: 64; 7: 9; 8: 16; 10: 12; 42: 3; 43, 64: 2; 65..128: 1)
          (63, 3, 1, 2), (64, 3, 1, 2), (65, 3, 1, 2), (10, 4, 7, 5), (19, 4, 7, 5), (17, 4, 8, 5), (33, 4, 8, 5),
          (11, 70, 10, 9), (12, 70, 10, 9), (13, 70, 10, 9), (25, 6, 10, 3), (4, 5, 42, 3), (3, 5, 43, 3), (3, 5, 64, 3), (2, 5, 65, 3),
          (2, 66, 100, 40), (2, 5, 128, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gauss_mix_lse_matches_the_float64_reference(lib, shape):
    N, M, S, L = shape
    rng = np.random.default_rng(sum(shape))
    mean, std = _table(rng, M, L)
    z = _draws(rng, N, S, mean, std)
    blk, full = _run(lib, z, mean, std)
    want_b, want_f = ref.gauss_mix_lse(z, mean, std)
    _close(blk, want_b, "lse_block %s" % (shape,))
    _close(full, want_f, "lse_full %s" % (shape,))


@pytest.mark.parametrize("where", ["first", "last"])
def test_the_online_rescale_runs_in_both_directions(lib, where):
    """the posterior every draw comes from -- the sharpest of the table, so the largest term by far -- is the first m (every later
    term is added to a settled maximum) or the last one (the running sums are rescaled at the very end)"""
    N, M, S, L = 4, 1000, 10, 20
    rng = np.random.default_rng(1000)
    mean, std = _table(rng, M, L)
    top = 0 if where == "first" else M - 1
    std[top] = 1e-3
    z = _draws(rng, N, S, mean, std, owner=[top] * N)
    t = ref.terms(z[1], mean, std)
    assert (t.argmax(axis=1) == top).all() and t.sum(axis=0).argmax() == top
    assert (np.sort(t, axis=1)[:, -1] - np.sort(t, axis=1)[:, -2] > 20).all()      # nothing else comes near
    blk, full = _run(lib, z, mean, std)
    want_b, want_f = ref.gauss_mix_lse(z, mean, std)
    _close(blk, want_b, "lse_block, maximum %s" % where)
    _close(full, want_f, "lse_full, maximum %s" % where)


def test_sharp_posteriors_underflow_to_finite_values(lib):
    N, M, S, L = 5, 65, 3, 150
    rng = np.random.default_rng(4)
    mean, std = _table(rng, M, L, std=1e-4)
    z = _draws(rng, N, S, mean, std)
    t = ref.terms(z[0], mean, std)
    assert (np.exp(np.sort(t, axis=1)[:, -2] - t.max(axis=1)) == 0.0).all()         # every far term underflows once the max is out
    blk, full = _run(lib, z, mean, std)
    assert np.isfinite(blk).all() and np.isfinite(full).all()
    want_b, want_f = ref.gauss_mix_lse(z, mean, std)
    _close(blk, want_b, "lse_block, std 1e-4")
    _close(full, want_f, "lse_full, std 1e-4")


# ------------------------------------------------------------------ contracts
@pytest.mark.parametrize("shape", [(7, 130, 10, 150), (70, 9, 1, 7), (21, 40, 7, 33)], ids=lambda s: "x".join(map(str, s)))
def test_a_caption_s_bits_depend_on_the_caption_and_the_table_only(lib, shape):
    N, M, S, L = shape
    rng = np.random.default_rng(11)
    mean, std = _table(rng, M, L)
    z = _draws(rng, N, S, mean, std)
    blk, full = _run(lib, z, mean, std)
    blk2, full2 = _run(lib, z, mean, std)
    assert np.array_equal(_bits(blk), _bits(blk2)) and np.array_equal(_bits(full), _bits(full2))    # two calls: the same bits
    for c in sorted({0, N // 2, N - 1}):
        rest = np.delete(z, c, axis=0)
        alone = _run(lib, z[c:c + 1], mean, std)
        first = _run(lib, np.concatenate([z[c:c + 1], rest]), mean, std)
        last = _run(lib, np.concatenate([rest[:N // 2], z[c:c + 1]]), mean, std)                  # another N as well
        for name, (b, f), row in (("alone", alone, 0), ("first", first, 0), ("last", last, -1)):
            assert np.array_equal(_bits(b[row]), _bits(blk[c])) and _bits(f[row:][:1])[0] == _bits(full[c:c + 1])[0], (c, name)


def test_empty_calls_and_refusals(lib):
    from .gpu_util import P, stream, zeros
    a, d = zeros(256), zeros(256, dtype=torch.float64)
    st = stream()
    call = lambda N=2, M=4, S=2, L=3, z=P(a), mean=P(a), std=P(a), blk=P(d), full=P(d): lib.vc_gauss_mix_lse_f64(st, N, M, S, L, z, mean, std, blk, full)
    assert call(N=0) == 0
    assert call(N=0, M=0, S=0, L=0, z=None, mean=None, std=None, blk=None, full=None) == 0      # no pointer is looked at
    for bad in (dict(N=-1), dict(M=0), dict(M=-3), dict(S=0), dict(S=-1), dict(L=0), dict(L=-2), dict(S=129), dict(N=1 << 31),
                dict(M=1 << 31), dict(z=None), dict(mean=None), dict(std=None), dict(blk=None), dict(full=None),
                dict(z=None, mean=None, std=None, blk=None, full=None)):
        with pytest.raises(abi.VaecapError) as e:
            call(**bad)
        assert "invalid argument" in str(e.value), bad
    torch.cuda.synchronize()
    assert (d == 0).all() and (a == 0).all()                                                      # nothing was launched


# ------------------------------------------------------------------ mutual_information
def _sampled(lib, mean, std, eps):
    """z = mean + std * eps as the library forms it (vc_latent_sample_f32: the expression vc_posterior_latent_f32 shares, bit for bit)"""
    from .gpu_util import P, dev, host, stream
    N, S, L = eps.shape
    z = torch.zeros((N * S, L), device="cuda")
    lib.vc_latent_sample_f32(stream(), 1, N * S, L, P(dev(np.repeat(mean, S, axis=0))), P(dev(np.repeat(std, S, axis=0))),
                             P(dev(np.ascontiguousarray(eps, np.float32).reshape(N * S, L))), P(z))
    return host(z).reshape(N, S, L)


def _same(got, want):
    assert set(got) == set(want) == {"mi", "mi_block", "mi_ceiling", "captions"}
    assert got["captions"] == want["captions"] and got["mi_ceiling"] == want["mi_ceiling"]
    for k in ("mi", "mi_block"):
        print("%s: device %.12f, reference %.12f" % (k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= TOL * max(1.0, abs(want[k])), k


def test_mutual_information_matches_the_reference_with_injected_eps(lib):
    N, S, L = 64, 3, 10
    rng = np.random.default_rng(64)
    mean, std = _table(rng, N, L)
    eps = rng.standard_normal((N, S, L)).astype(np.float32)
    got = latent_mi.mutual_information(mean, std, S, eps=eps, lib=lib)
    _same(got, ref.mutual_information(mean, std, z=_sampled(lib, mean, std, eps)))
    blk, full = latent_mi.gauss_mix_lse(_sampled(lib, mean, std, eps), mean, std, lib=lib)       # the thin wrapper: the same numbers
    assert blk.shape == (N, S) and full.shape == (N,) and blk.dtype == full.dtype == np.float64
    assert latent_mi.summarise(blk, full, std) == got
    bt, ft = latent_mi.gauss_mix_lse(torch.from_numpy(_sampled(lib, mean, std, eps)).cuda(), torch.from_numpy(mean).cuda(),
                                     torch.from_numpy(std).cuda(), lib=lib)                      # device tensors in
    assert np.array_equal(_bits(bt), _bits(blk)) and np.array_equal(_bits(ft), _bits(full))


def test_mutual_information_draws_with_philox_on_its_own_stream(lib):
    from .gpu_util import P, host, stream
    N, S, L = 64, 3, 10
    rng = np.random.default_rng(65)
    mean, std = _table(rng, N, L)
    a, b, c = (latent_mi.mutual_information(mean, std, S, seed=s, lib=lib) for s in (5, 5, 6))
    assert a == b                                                                                 # the same seed: the same numbers
    assert a["mi"] != c["mi"] and a["mi_block"] != c["mi_block"]                                 # another seed: other draws
    eps = torch.zeros(N * S * L, device="cuda")                                                   # the library's draws of that stream
    lib.vc_philox_normal_f32(stream(), P(eps), N * S * L, 5, latent_mi.MI_PHILOX_STREAM << 32, None)
    _same(a, ref.mutual_information(mean, std, z=_sampled(lib, mean, std, host(eps).reshape(N, S, L))))
    assert latent_mi.MI_PHILOX_STREAM == 12                                                       # 1..11 are taken (bound() draws with 8)


def test_mutual_information_on_tables_whose_answer_is_known(lib):
    """identical rows: nothing to tell apart, |mi_block| < 0.1; rows 50 std apart: every draw names its caption, the estimate sits at
    its ceiling log N, mi_ceiling - mi_block < 0.1.  In both tables a draw's own posterior carries the mixture, so the estimate misses
    its value by 0.5 (mean_{n,s} sum_l eps^2 - L) exactly: a number of standard deviation sqrt(L / (2 N S)) = 0.044 at N = 256,
    S = 10, L = 10 that the injected eps fixes (0.029 for this generator seed; asserted below as a precondition on the inputs)."""
    N, S, L = 256, 10, 10
    rng = np.random.default_rng(2560)
    eps = rng.standard_normal((N, S, L)).astype(np.float32)
    assert abs(0.5 * ((eps.astype(np.float64) ** 2).sum(axis=2) - L).mean()) < 0.05
    std = np.full((N, L), 0.1, np.float32)
    same = latent_mi.mutual_information(np.full((N, L), 0.3, np.float32), std, S, eps=eps, lib=lib)
    apart = latent_mi.mutual_information((5.0 * np.arange(N, dtype=np.float32))[:, None] * np.ones((1, L), np.float32), std, S, eps=eps, lib=lib)
    print("identical rows: mi %.4f mi_block %.4f; rows 50 std apart: mi %.4f mi_block %.4f, ceiling %.4f"
          % (same["mi"], same["mi_block"], apart["mi"], apart["mi_block"], apart["mi_ceiling"]))
    assert same["captions"] == apart["captions"] == N and same["mi_ceiling"] == apart["mi_ceiling"] == math.log(N)
    assert abs(same["mi_block"]) < 0.1
    assert apart["mi_ceiling"] - apart["mi_block"] < 0.1


def test_mutual_information_refuses_what_it_cannot_compute(lib):
    mean, std = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    assert latent_mi.mutual_information(mean, std, 2, lib=lib)["captions"] == 4

    def put(a, v):
        a = a.copy()
        a[1, 2] = v
        return a

    for kw in (dict(std=put(std, 0.0)), dict(std=put(std, -1.0)), dict(std=put(std, np.inf)), dict(std=put(std, np.nan)),
               dict(mean=put(mean, np.nan)), dict(mean=put(mean, -np.inf)), dict(std=std[:3]), dict(std=std[:, :2]), dict(mean=mean[0], std=std[0]),
               dict(mean=np.zeros((4, 0), np.float32), std=np.zeros((4, 0), np.float32)), dict(samples=0), dict(samples=-2), dict(samples=129),
               dict(samples=1.5), dict(mean=np.zeros((0, 3), np.float32), std=np.ones((0, 3), np.float32)),
               dict(eps=np.zeros((4, 2, 2), np.float32)), dict(eps=np.zeros((3, 2, 3), np.float32))):
        args = dict(mean=mean, std=std, samples=2)
        args.update(kw)
        with pytest.raises(ValueError):
            latent_mi.mutual_information(args.pop("mean"), args.pop("std"), args.pop("samples"), lib=lib, **args)
    big = np.broadcast_to(np.ones((1, 1), np.float32), (latent_mi.MI_MAX_CAPTIONS + 1, 1))
    with pytest.raises(ValueError, match="0.4 GB"):
        latent_mi.mutual_information(big, big, 1, lib=lib)
    for kw in (dict(std=put(std, 0.0)), dict(mean=put(mean, np.nan)), dict(z=np.zeros((2, 2, 2), np.float32)), dict(std=std[:3]),
               dict(z=np.zeros((2, 129, 3), np.float32)), dict(z=np.full((2, 2, 3), np.inf, np.float32))):
        args = dict(z=np.zeros((2, 2, 3), np.float32), mean=mean, std=std)
        args.update(kw)
        with pytest.raises(ValueError):
            latent_mi.gauss_mix_lse(args["z"], args["mean"], args["std"], lib=lib)
    blk, full = latent_mi.gauss_mix_lse(np.zeros((0, 2, 3), np.float32), mean, std, lib=lib)
    assert blk.shape == (0, 2) and full.shape == (0,)


# ------------------------------------------------------------------ command line
def test_main_synthetic_inference_with_bound_mi(tmp_path, monkeypatch, lib):
    common = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10",
              "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "mi"]
    infer = common + ["--mode", "inference", "--sample_gen", "greedy", "--bound_draws", "2"]
    _main(tmp_path, common + ["--epochs", "1", "--max_steps", "1"])
    out = _main(tmp_path, infer + ["--gen_name", "mi", "--bound_mi", "16"])
    head = json.load(open(tmp_path / "val_mi_bound.json"))[0]
    assert set(head) == {"draws", "skipped_images", "active_units", "latent_size", "mi", "mi_block", "mi_captions", "mi_ceiling"}
    assert 1 <= head["mi_captions"] <= 16 and 0 <= head["mi_ceiling"] == math.log(head["mi_captions"])
    assert math.isfinite(head["mi"]) and math.isfinite(head["mi_block"])
    line = [ln for ln in out.splitlines() if ln.startswith("Mutual information")]
    assert len(line) == 1 and all(k in line[0] for k in ("mi %.6f" % head["mi"], "mi_block %.6f" % head["mi_block"],
                                                            "mi_ceiling %.6f" % head["mi_ceiling"], "mi_captions %d" % head["mi_captions"]))
    # the same captions through bound(): their posteriors, the same seed -> the same estimate
    monkeypatch.chdir(tmp_path)
    p = Parameters().parse_args(infer + ["--gen_name", "mi", "--bound_mi", "16"])
    from vae_captioning_amd.trainer import Trainer
    tr = Trainer(p, p.vocab_size, seed=p.seed)
    tr.load_state_dict(spec.init_caption_params(p, p.vocab_size, seed=p.seed))
    tr.restore("./checkpoints/mi.ckpt.npz")
    gen = CaptionGenerator(tr.cap)
    from vae_captioning_amd.ops.inference import human_captions
    rng = np.random.default_rng(p.seed + 5)                                        # main.py's two synthetic validation batches
    mean, std = [], []
    for _ in range(2):
        b = synth.make_batch(rng, p.batch_size, 1, 20, p.vocab_size, use_ci=spec.uses_ci(p), images=False)
        res = gen.bound(b["features"], human_captions((b["cap_dec"], b["cap_enc"]), b["lengths"]), None, None, None, synth.BOS, synth.EOS,
                        draws=2, return_latents="stats")
        mean += [r["mean"] for rs in res for r in rs]
        std += [r["std"] for rs in res for r in rs]
    assert len(mean) == 8 == head["mi_captions"]
    want = latent_mi.mutual_information(np.stack(mean[:16]), np.stack(std[:16]), p.gen_z_samples, seed=p.seed, lib=lib)
    assert head["mi"] == want["mi"] and head["mi_block"] == want["mi_block"] and head["mi_ceiling"] == want["mi_ceiling"]
    # without the flag: today's header
    _main(tmp_path, infer + ["--gen_name", "off"])
    assert set(json.load(open(tmp_path / "val_off_bound.json"))[0]) == {"draws", "skipped_images", "active_units", "latent_size"}
    assert os.path.exists(tmp_path / "val_off.json")
