"""-m gpu: the posterior at inference -- the three kernels of csrc/bound.hip against numpy and against the kernels whose expressions they
share, CaptionGenerator.encode against the oracle's posterior, CaptionGenerator.bound against the fp64 checker tests/bound_ref.py, its
independence of batch and passes, the unchanged bits of score() / diverse(rerank="marginal"), the refusals and the command line."""
import json
import math
import re

import numpy as np
import pytest
import torch

from vae_captioning_amd import abi, spec
from vae_captioning_amd.generate import SCORE_MAX_TOKENS, CaptionGenerator

from . import bound_ref as ref
from .test_gpu_diverse import _eps
from .test_gpu_generate import setup
from .test_gpu_score import SUMS, _main

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
PRIORS = [dict(prior="Normal"), dict(prior="AG", use_c_v=True), dict(prior="GMM")]
IDS = lambda k: "-".join("%s=%s" % i for i in k.items())
SHAPES = [(1, 1, 1, 1), (3, 4, 3, 7), (5, 20, 10, 150), (2, 256, 1, 64)]   # (C, K, S, L); S*L = 21: rows start inside Philox quads
SEED, OFFSET = (977 << 32) + 12345, 8 << 32
# encode() against the fp64 oracle, relative to each tensor's maximum: 4 x the largest error observed over the cases of
# test_encode_matches_the_oracle_s_posterior (5.0e-7: the std of the AG model; DESIGN.md "Bounds"); the issue's cap is 1e-4, a tenth
# of the 1e-3 the project holds KL to
ENC_TOL = 2.0e-6


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------ vc_posterior_latent_f32
def _inputs(rng, C, K, S, L, with_pm):
    mean = (rng.standard_normal((C, L)) * 0.1).astype(np.float32)
    std = np.exp(rng.standard_normal((C, L)) * 0.5 - 2.5).astype(np.float32)
    pm = img = None
    if with_pm:   # fewer prior-mean rows than captions: captions share them
        n_img = max(1, (C + 1) // 2)
        pm, img = (rng.standard_normal((n_img, L)) * 0.05).astype(np.float32), (np.arange(C) % n_img).astype(np.int32)
    return mean, std, pm, img


def _latent(lib, K, S, L, mean, std, pm, img, sp, eps=None, seed=0, offset=0, step=None):
    from .gpu_util import P, dev, host, stream
    rows = mean.shape[0] * K
    z = torch.full((rows, S, L), 7.0, device="cuda")
    lw = torch.full((rows,), 7.0, dtype=torch.float64, device="cuda")
    lib.vc_posterior_latent_f32(stream(), rows, K, S, L, P(dev(mean)), P(dev(std)), P(dev(pm)) if pm is not None else None,
                                P(dev(img)) if img is not None else None, sp, P(dev(eps)) if eps is not None else None, seed, offset,
                                P(step), P(z), P(lw))
    return host(z), host(lw)


def _sample(lib, mean_rows, std_rows, eps):
    """vc_latent_sample_f32 on [n, L] rows: the expression z = mean + std * eps as the training step computes it"""
    from .gpu_util import P, dev, host, stream
    n, L = mean_rows.shape
    z = torch.zeros((n, L), device="cuda")
    lib.vc_latent_sample_f32(stream(), 1, n, L, P(dev(mean_rows)), P(dev(std_rows)), P(dev(np.ascontiguousarray(eps).reshape(n, L))), P(z))
    return host(z)


def _philox(lib, n, seed, offset, step):
    from .gpu_util import P, host, stream
    out = torch.zeros((n,), device="cuda")
    lib.vc_philox_normal_f32(stream(), P(out), n, seed, offset, P(step))
    return host(out)


def _check_logw(got, z, eps, std, pm, img, sp, K):
    """logw against the float64 formula on the kernel's own f32 z: only the summation order differs, so the error is a few float64
    roundings of the terms' magnitudes -- 1e-12 of sum |terms| (the four terms of every element) leaves three decimal digits"""
    for r in range(z.shape[0]):
        c = r // K
        pmr = pm[img[c]].astype(np.float64) if pm is not None else np.zeros(std.shape[1])
        z64, e64, s64 = z[r].astype(np.float64), eps[r].astype(np.float64), std[c].astype(np.float64)
        parts = [-0.5 * ((z64 - pmr) / float(np.float32(sp))) ** 2, np.full_like(z64, -math.log(float(np.float32(sp)))), 0.5 * e64 ** 2,
                 np.broadcast_to(np.log(s64), z64.shape)]
        want = math.fsum(np.concatenate([p.ravel() for p in parts]).tolist())
        scale = sum(float(np.abs(p).sum()) for p in parts)
        assert abs(got[r] - want) <= 1e-12 * scale, (r, got[r], want, scale)


@pytest.mark.parametrize("with_pm", [False, True], ids=["pm-null", "pm-shared"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_posterior_latent_matches_numpy_with_injected_eps(lib, shape, with_pm):
    C, K, S, L = shape
    rng = np.random.default_rng(sum(shape) + with_pm)
    mean, std, pm, img = _inputs(rng, C, K, S, L, with_pm)
    eps = rng.standard_normal((C * K, S, L)).astype(np.float32)
    z, lw = _latent(lib, K, S, L, mean, std, pm, img, 0.1, eps)
    want = _sample(lib, np.repeat(mean, K * S, axis=0), np.repeat(std, K * S, axis=0), eps).reshape(z.shape)
    assert np.array_equal(_bits(z), _bits(want))
    np.testing.assert_allclose(z, np.repeat(mean, K, 0)[:, None] + np.repeat(std, K, 0)[:, None] * eps, rtol=1e-6, atol=1e-7)   # (the expression itself)
    _check_logw(lw, z, eps, std, pm, img, 0.1, K)


@pytest.mark.parametrize("shape", SHAPES[1:3], ids=lambda s: "x".join(map(str, s)))
def test_posterior_latent_philox_draws_are_the_library_s_and_a_row_depends_on_the_row_only(lib, shape):
    C, K, S, L = shape
    rng = np.random.default_rng(7)
    mean, std, pm, img = _inputs(rng, C, K, S, L, True)
    step = torch.tensor([3], dtype=torch.int32, device="cuda")
    rows = C * K
    z, lw = _latent(lib, K, S, L, mean, std, pm, img, 0.1, None, SEED, OFFSET, step)
    eps = _philox(lib, rows * S * L, SEED, OFFSET, step).reshape(rows, S, L)
    want = _sample(lib, np.repeat(mean, K * S, axis=0), np.repeat(std, K * S, axis=0), eps).reshape(z.shape)
    assert np.array_equal(_bits(z), _bits(want))
    _check_logw(lw, z, eps, std, pm, img, 0.1, K)
    # a row run alone (as row 0 of a call of its own, its eps injected): the same z and logw bits
    odd = [r for r in range(rows) if (r * S * L) % 4]
    for r in sorted(set([0, rows - 1] + odd[:2] + odd[-1:])):
        c = r // K
        z1, lw1 = _latent(lib, 1, S, L, mean[c:c + 1], std[c:c + 1], pm[img[c]:img[c] + 1], np.zeros(1, np.int32), 0.1, eps[r:r + 1])
        assert np.array_equal(_bits(z1[0]), _bits(z[r])) and _bits(lw1)[0] == _bits(lw)[r], r
    if (S * L) % 4:
        assert odd


@pytest.mark.parametrize("inject", [True, False], ids=["eps", "philox"])
def test_posterior_latent_with_the_prior_as_proposal_is_diverse_s_draw_with_unit_weights(lib, inject):
    from .gpu_util import P, dev, host, stream
    C, K, S, L, sp = 3, 4, 3, 7, 0.1
    rows = C * K
    rng = np.random.default_rng(5)
    step = torch.tensor([2], dtype=torch.int32, device="cuda")
    eps = rng.standard_normal((rows, S, L)).astype(np.float32) if inject else None
    mean, std = np.zeros((C, L), np.float32), np.full((C, L), sp, np.float32)
    z, lw = _latent(lib, K, S, L, mean, std, None, None, sp, eps, SEED, OFFSET, step)
    zd = torch.zeros((rows, S, L), device="cuda")
    lib.vc_diverse_latent_f32(stream(), rows, K, S, L, None, sp, P(dev(eps)) if inject else None, SEED, OFFSET, P(step), P(zd))
    assert np.array_equal(_bits(z), _bits(host(zd)))
    if not inject:
        eps = _philox(lib, rows * S * L, SEED, OFFSET, step).reshape(rows, S, L)
    bound = 2.0 ** -22 * (eps.astype(np.float64) ** 2).sum(axis=(1, 2))   # the rounding of sigma_p * eps is the only error
    print("prior as proposal: max |logw| / (2^-22 sum eps^2) = %.3f" % (np.abs(lw) / bound).max())
    assert (np.abs(lw) <= bound).all()


def test_bound_entries_refuse_bad_arguments(lib):
    from .gpu_util import P, stream, zeros
    a, d, i = zeros(64), zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.int32, device="cuda")
    st = stream()
    lat = lambda rows=4, K=2, S=2, L=2, z=P(a), lw=P(d): lib.vc_posterior_latent_f32(st, rows, K, S, L, P(a), P(a), None, None, 0.1, None, 0, 0, None, z, lw)
    red = lambda T=2, C=2, K=2, lp=P(d), out=P(d): lib.vc_bound_reduce_f64(st, P(a), T, C, K, P(i), P(d), lp, out)
    klr = lambda C=2, S=2, L=2, kl=P(d): lib.vc_gauss_kl_rows_f64(st, C, S, L, P(a), P(a), None, None, 0.1, kl)
    for bad in (lambda: lat(K=0), lambda: lat(rows=514, K=257), lambda: lat(S=0), lambda: lat(L=0), lambda: lat(rows=-2), lambda: lat(z=None),
                lambda: lat(lw=None), lambda: lat(rows=3), lambda: red(K=0), lambda: red(K=257), lambda: red(T=-1), lambda: red(C=-1),
                lambda: red(lp=None), lambda: red(out=None), lambda: klr(C=-1), lambda: klr(S=0), lambda: klr(L=0), lambda: klr(kl=None)):
        with pytest.raises(abi.VaecapError) as e:
            bad()
        assert "invalid argument" in str(e.value)
    lat(rows=0), red(C=0), klr(C=0)   # empty calls are no-ops


# ------------------------------------------------------------------ vc_bound_reduce_f64, vc_gauss_kl_rows_f64
def test_bound_reduce_matches_numpy_float64_and_keeps_score_reduce_s_sums(lib):
    from .gpu_util import P, dev, host, stream
    rng = np.random.default_rng(9)
    for T, C, K in ((5, 3, 1), (9, 4, 3), (6, 2, 256)):
        lp = -rng.random((T, C * K)).astype(np.float32) * 40
        ln = rng.integers(1, T + 1, size=C).astype(np.int32)
        ln[0] = 0                                               # a zero-length caption: rec_k = 0
        lw = -rng.random(C * K) * 800 - 5.0
        if K > 1:                                               # a_k spread over 800 nats (sums of lp span < 400): exp underflows without the max shift
            lw.reshape(C, K)[:, 0], lw.reshape(C, K)[:, -1] = -5.0, -1205.0
        f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")
        logprob, out, lp0, marg = f64(C * K), f64(C * 5), f64(C * K), f64(C)
        lib.vc_bound_reduce_f64(stream(), P(dev(lp)), T, C, K, P(dev(ln)), P(dev(lw)), P(logprob), P(out))
        lib.vc_score_reduce_f64(stream(), P(dev(lp)), T, C, K, P(dev(ln)), P(lp0), P(marg))
        assert np.array_equal(_bits(host(logprob)), _bits(host(lp0)))
        got, sums = host(out).reshape(C, 5), host(logprob).reshape(C, K)
        assert (sums[0] == 0).all()
        for c in range(C):
            a = sums[c] + lw[c * K:(c + 1) * K]
            if K > 1:
                assert a.max() - a.min() > 800
            want = ref.reduce(sums[c], lw[c * K:(c + 1) * K])
            np.testing.assert_allclose(got[c], [want[k] for k in ("elbo", "iwae", "rec", "kl_mc", "ess")], rtol=1e-13, atol=1e-13)
            assert got[c, 1] >= got[c, 0] and 1.0 <= got[c, 4] <= K
            if K == 1:
                assert got[c, 1] == got[c, 0] and got[c, 4] == 1.0


@pytest.mark.parametrize("with_pm", [False, True], ids=["pm-null", "pm-shared"])
def test_gauss_kl_rows_matches_numpy_float64(lib, with_pm):
    from .gpu_util import P, dev, host, stream
    for C, S, L in ((1, 1, 1), (4, 3, 150), (3, 100, 7)):
        rng = np.random.default_rng(C + S + L)
        mean, std, pm, img = _inputs(rng, C, 1, S, L, with_pm)
        kl = torch.full((C,), 7.0, dtype=torch.float64, device="cuda")
        lib.vc_gauss_kl_rows_f64(stream(), C, S, L, P(dev(mean)), P(dev(std)), P(dev(pm)) if with_pm else None, P(dev(img)) if with_pm else None,
                                 0.1, P(kl))
        want = [ref.kl(mean[c], std[c], pm[img[c]] if with_pm else None, np.float32(0.1), S) for c in range(C)]
        np.testing.assert_allclose(host(kl), want, rtol=1e-13, atol=1e-13)
    # q == p: zero
    sp = np.float32(0.1)
    lib.vc_gauss_kl_rows_f64(stream(), 1, 4, 10, P(dev(np.zeros((1, 10), np.float32))), P(dev(np.full((1, 10), sp, np.float32))), None, None, float(sp), P(kl))
    assert abs(host(kl)[0]) <= 1e-13


# ------------------------------------------------------------------ encode() and bound() against the fp64 checker
COUNTS = [0, 1, 3, 1, 3, 0]   # captions per image of setup()'s six (the AG model's last image has no cluster vector: no captions)


def _captions(rng, V, counts=COUNTS):
    """ragged caption counts and lengths 1..12 (both ends present), some with <BOS>, most with <EOS>"""
    lens = [1, 12] + rng.integers(1, 13, size=sum(counts)).tolist()
    caps, j = [], 0
    for n in counts:
        row = []
        for _ in range(n):
            t = rng.integers(3, V, size=lens[j]).tolist()
            if lens[j] > 1 and j % 3:
                t[-1] = EOS
            row.append(([BOS] + t) if j % 2 else t)
            j += 1
        caps.append(row)
    return caps


def _strip(t):
    return t[1:] if t and t[0] == BOS else t


def _model(lib, kw, seed=19):
    p, eng, gen, P64, feats, cv, _, cm = setup(lib, seed, **kw)
    c = cv if spec.uses_ci(p) else None
    return p, eng, gen, P64, feats, cv, c, cm


def _gmm(rng, p, n):
    return rng.integers(0, 90, size=n).astype(np.int32) if p.prior == "GMM" else None


@pytest.mark.parametrize("kw", PRIORS, ids=IDS)
def test_encode_matches_the_oracle_s_posterior(lib, kw):
    p, eng, gen, P64, feats, cv, c, cm = _model(lib, kw)
    rng = np.random.default_rng(21)
    caps = _captions(rng, eng.V)
    gmm = _gmm(rng, p, sum(COUNTS))
    got = gen.encode(feats, caps, c, gmm, BOS)
    assert [len(g) for g in got] == COUNTS
    gm, gs, wm, ws, j = [], [], [], [], 0
    for b, cl in enumerate(caps):
        for t, (m, s) in zip(cl, got[b]):
            assert m.dtype == np.float32 and s.dtype == np.float32 and m.shape == s.shape == (p.latent_size,)
            tm, ts = ref.posterior(P64, p, feats[b], cv[b], _strip(t), BOS, None if gmm is None else gmm[j], cm)
            gm.append(m), gs.append(s), wm.append(tm), ws.append(ts)
            j += 1
    gm, gs, wm, ws = (np.array(a, np.float64) for a in (gm, gs, wm, ws))
    em, es = np.abs(gm - wm).max() / np.abs(wm).max(), np.abs(gs - ws).max() / np.abs(ws).max()
    print("%s: encode() vs fp64 oracle, relative to the tensor's maximum: mean %.3e, std %.3e" % (IDS(kw), em, es))
    assert (gs > 0).all()
    assert em <= ENC_TOL and es <= ENC_TOL


def _flat_eps(rng, p, K, C):
    return rng.standard_normal((K, p.gen_z_samples, C, p.latent_size)).astype(np.float32)


@pytest.mark.parametrize("kw", PRIORS, ids=IDS)
def test_bound_matches_the_checker_end_to_end(lib, kw):
    p, eng, gen, P64, feats, cv, c, cm = _model(lib, kw)
    rng = np.random.default_rng(22)
    counts = [0, 1, 2, 0, 1, 0]
    caps = _captions(rng, eng.V, counts)
    C, K = sum(counts), 4
    gmm, eps = _gmm(rng, p, C), _flat_eps(rng, p, K, C)
    got = gen.bound(feats, caps, c, eps, gmm, BOS, EOS, draws=K, return_latents=True)
    pm = gen.prior_mean(cv) if p.prior == "AG" else None
    assert [len(g) for g in got] == counts
    j = 0
    for b, cl in enumerate(caps):
        for t, g in zip(cl, got[b]):
            t = _strip(t)
            assert g["tokens"] == len(t) and g["z"].shape == (K, p.gen_z_samples, p.latent_size) and g["z"].dtype == np.float32
            assert g["logprob"].dtype == np.float64 and g["logprob"].shape == g["logw"].shape == (K,)
            e = eps[:, :, j]
            want = ref.bound(P64, p, feats[b], cv[b], t, BOS, e, None if pm is None else pm[b], mean=g["mean"], std=g["std"], z=g["z"])
            np.testing.assert_allclose(g["logprob"], want["logprob"], **SUMS)
            np.testing.assert_allclose(g["logw"], want["logw"], rtol=1e-12, atol=0)
            np.testing.assert_allclose(g["kl"], want["kl"], rtol=1e-12, atol=0)
            own = ref.reduce(g["logprob"], g["logw"])   # the device's reduction of its own per-draw terms
            for k in ("elbo", "iwae", "rec", "kl_mc", "ess"):
                np.testing.assert_allclose(g[k], own[k], rtol=1e-12, atol=0, err_msg=k)
            assert g["iwae"] >= g["elbo"] - 1e-12 and 1.0 <= g["ess"] <= K
            # z is the definition's: mean + std * eps on the returned f32 statistics
            np.testing.assert_allclose(g["z"], g["mean"][None, None] + g["std"][None, None] * e, rtol=1e-6, atol=1e-7)
            j += 1
    one = gen.bound(feats, caps, c, eps[:1], gmm, BOS, EOS, draws=1)
    for row in one:
        for g in row:
            assert abs(g["iwae"] - g["elbo"]) <= 1e-14 * max(1.0, abs(g["elbo"])) and g["ess"] == 1.0 and "z" not in g


def _same_record(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def test_a_caption_s_record_does_not_depend_on_the_batch_or_on_the_passes(lib, monkeypatch):
    p, eng, gen, P64, feats, cv, c, cm = _model(lib, dict(prior="Normal"))
    rng = np.random.default_rng(23)
    counts = [1, 3, 2]
    feats = feats[:3]
    caps = _captions(rng, eng.V, counts)
    K = 4
    eps = _flat_eps(rng, p, K, sum(counts))
    whole = gen.bound(feats, caps, None, eps, None, BOS, EOS, draws=K, return_latents=True)
    alone = gen.bound(feats[1:2], caps[1:2], None, eps[:, :, 1:4], None, BOS, EOS, draws=K, return_latents=True)
    for a, w in zip(alone[0], whole[1]):
        _same_record(a, w)
    g = CaptionGenerator(eng)
    passes = []
    one = CaptionGenerator._bound_pass
    # (patched on the class: see tests/test_gpu_score.py)
    monkeypatch.setattr(CaptionGenerator, "_bound_pass", lambda self, *a: (passes.append(a[0].shape[0]), one(self, *a))[1])
    g.bound_rows = 1                                         # every image exceeds it alone: three passes
    cut = g.bound(feats, caps, None, eps, None, BOS, EOS, draws=K, return_latents=True)
    assert passes == [1, 1, 1]
    for rc, rw in zip(cut, whole):
        assert len(rc) == len(rw)
        for a, w in zip(rc, rw):
            _same_record(a, w)


# ------------------------------------------------------------------ score() and diverse(rerank="marginal") are what they were
@pytest.mark.parametrize("kw", [dict(prior="Normal"), dict(prior="AG", use_c_v=True)], ids=IDS)
def test_score_and_marginal_reranking_keep_the_bits_of_the_image_parent_mapping(lib, kw):
    """The teacher forcing behind score() takes row c*K + k's state from row b*K + k of the image states.  The same call on states
    expanded by that mapping by hand, every caption presented as an image of its own (its parent rows are then its own rows), must
    give the same bits: a row's result depends on the row alone."""
    p, eng, gen, P64, feats, cv, c, cm = _model(lib, kw, seed=31)
    B, K, T = 3, 4, 12
    rng = np.random.default_rng(24)
    feats, c = feats[:B], (c[:B] if c is not None else None)
    eps = _eps(rng, p, K, B)
    caps = [[_strip(t) for t in cl] for cl in _captions(rng, eng.V, [1, 3, 2])]
    caps[1][1] = []                                          # an empty caption among them

    def by_hand(cap_lists):
        c0, h0 = gen._diverse_init(feats, c, eps, K)
        parent = torch.tensor([b * K + k for b, cl in enumerate(cap_lists) for _ in cl for k in range(K)], device="cuda")
        return gen._score_states(c0[parent].contiguous(), h0[parent].contiguous(), K, [[t] for cl in cap_lists for t in cl], BOS)

    got = gen.score(feats, caps, c, eps, BOS, EOS, draws=K)
    lp, marg = by_hand(caps)
    flat = [r for row in got for r in row]
    assert len(flat) == lp.shape[0] == 6
    for j, r in enumerate(flat):
        assert np.array_equal(_bits(r["logprob"]), _bits(lp[j])) and r["marginal"] == float(marg[j])
    res = gen.diverse(feats, c, eps, BOS, EOS, draws=K, max_len=T, rerank="marginal")
    dcaps = [[list(e[0]) for e in r] for r in res]
    _, marg = by_hand(dcaps)
    assert [e[3] for r in res for e in r] == marg.tolist()


# ------------------------------------------------------------------ refusals
def test_encode_and_bound_refuse_what_they_cannot_compute(lib):
    p, eng, gen, P64, feats, cv, c, cm = _model(lib, dict(prior="Normal"))
    V = eng.V
    ok = [[[5, 6, EOS]]] + [[] for _ in range(5)]
    assert len(gen.encode(feats, ok)[0]) == 1
    for bad in ([[[5, V, EOS]]], [[[5, -1]]], [[[]]], [[[BOS]]], [[[3] * (SCORE_MAX_TOKENS + 1)]]):
        for call in (gen.encode, gen.bound):
            with pytest.raises(ValueError):
                call(feats, bad + [[] for _ in range(5)])
    with pytest.raises(ValueError):
        gen.encode(feats, ok[:5])                            # not one list per image
    for kwargs in (dict(draws=0), dict(draws=257), dict(draws=2, eps=np.zeros((2, p.gen_z_samples, 2, p.latent_size), np.float32))):
        with pytest.raises(ValueError):
            gen.bound(feats, ok, **kwargs)
    _, _, nogen, _, _, _, _, _ = _model(lib, dict(no_encoder=True))
    for call in (nogen.encode, nogen.bound):
        with pytest.raises(ValueError, match="no_encoder"):
            call(feats, ok)
    # GMM: the component of every caption has to be given, in 0..89
    p, eng, gen, P64, feats, cv, c, cm = _model(lib, dict(prior="GMM"))
    for gmm in (None, [90], [-1], [3, 4], [1.5]):
        with pytest.raises(ValueError):
            gen.encode(feats, ok, c, gmm)
    assert len(gen.bound(feats, ok, c, None, [89], draws=2)[0]) == 1
    with pytest.raises(ValueError):
        gen.encode(feats, ok, None, [3])                     # no cluster vectors
    # AG / GMM: setup()'s last image has an empty cluster vector -- with captions it raises, with none it passes
    for kw in (dict(prior="AG", use_c_v=True), dict(prior="GMM")):
        p, eng, gen, P64, feats, cv, c, cm = _model(lib, kw)
        gmm = [7] if p.prior == "GMM" else None
        last = [[] for _ in range(5)] + [[[5, 6, EOS]]]
        for call in (gen.encode, gen.bound):
            with pytest.raises(ValueError, match="cluster vector"):
                call(feats, last, c, gmm_idx=gmm)
        assert [len(r) for r in gen.encode(feats, ok, c, gmm)] == [1, 0, 0, 0, 0, 0]
        assert [len(r) for r in gen.bound(feats, ok, c, gmm_idx=gmm, draws=2)] == [1, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------ command line
def test_main_synthetic_inference_with_bound_draws(tmp_path):
    common = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10",
              "--gen_z_samples", "4", "--bs", "4", "--ckpt_format", "npz", "--checkpoint", "bd"]
    _main(tmp_path, common + ["--epochs", "1", "--max_steps", "1"])
    out = _main(tmp_path, common + ["--mode", "inference", "--sample_gen", "greedy", "--gen_name", "bd", "--bound_draws", "4", "--score_draws", "4"])
    recs = json.load(open(tmp_path / "val_bd_bound.json"))
    assert recs[0]["draws"] == 4 and recs[0]["skipped_images"] == 0 and 0 <= recs[0]["active_units"] <= recs[0]["latent_size"] == 10
    caps = [c for r in recs[1:] for c in r["captions"]]
    assert len(recs) == 9 and len(caps) == 8
    for c in caps:
        assert c["tokens"] == 20 and c["iwae"] >= c["elbo"] - 1e-9 and 1.0 <= c["ess"] <= 4.0 and c["kl"] > 0
    n = sum(c["tokens"] for c in caps)
    for name, key in (("importance-weighted bound", "iwae"), ("ELBO", "elbo")):
        ppl = float(re.search(r"Perplexity bound of the human captions from the %s, 4 posterior draws: (\S+)" % name, out).group(1))
        want = math.exp(-sum(c[key] for c in caps) / n)
        assert abs(ppl - want) <= 1e-12 * want and 1.0 < ppl < float("inf")
    for line in ("Mean KL(q || p) per caption:", "Mean effective sample size / draws:", "Active latent units: %d of 10" % recs[0]["active_units"]):
        assert line in out
    assert (tmp_path / "val_bd_scores.json").exists() and (tmp_path / "val_bd.json").exists()
