"""-m gpu: the kernels that close a training step -- csrc/optim.hip, the latent and loss-scalar kernels of csrc/loss.hip, the reductions
of csrc/elementwise.hip -- through the C ABI, at the sizes where each of their loops changes branch, against float64 / oracle references
(tests/step_tail_ref.py, oracle/optim.py, oracle/ops.py).

Rules of every case:
  * outputs, partial buffers and workspaces enter filled with NaN (`poisoned`): an element the kernel leaves unwritten fails the case;
  * every output buffer is followed by GUARD sentinel floats that must come back bit-unchanged (`logical` checks it); inputs are followed
    by NaN (`padded_in`), and the padding columns of a pitched input hold NaN: a read past the logical end poisons the result;
  * grid-dependent sizes come from vc_adam_blocks / vc_sumsq_blocks / vc_colsum_workspace_bytes, and a case that depends on the 2048-block
    cap asserts it, so a changed cap fails the case instead of emptying it.

Tolerances are the ones of tests/test_gpu_ops.py for the same kernels (assert_close: max error relative to max|ref|): Adam 2e-6, SGD /
Momentum / tile / segment sum 1e-6, norms, column sums and latent gradients 1e-5, the latent sample 1e-6.  Where this file sets its own, the
reasoning stands at the assertion."""
import functools

import numpy as np
import pytest

from oracle import ops as O
from oracle import optim as OO
from vae_captioning_amd.abi import VaecapError

from . import step_tail_ref as R
from .gpu_util import P, assert_close, dev, host, stream

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64
SENTINEL = f32(-24680.5)
NAN = f32(np.nan)
SWEEP = 2048 * 256   # elements of one grid sweep of the capped 256-thread launches (grid_for)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def guarded(a):
    """upload `a` (flattened) followed by GUARD sentinel floats; the logical part is t[:a.size]"""
    a = np.ascontiguousarray(a, f32).ravel()
    return dev(np.concatenate([a, np.full(GUARD, SENTINEL, f32)]))


def poisoned(n):
    return guarded(np.full(n, NAN, f32))


def padded_in(a, dtype=f32, pad=np.nan):
    """an INPUT: `a` (flattened) followed by GUARD poison values"""
    a = np.ascontiguousarray(a, dtype).ravel()
    return dev(np.concatenate([a, np.full(GUARD, pad).astype(dtype)]))


def raw(t, n, what):
    """host copy of the logical part after checking the guard band (NaN allowed: for buffers that must be UNCHANGED)"""
    h = host(t).ravel()
    assert h.size == n + GUARD, what
    assert np.array_equal(bits(h[n:]), bits(np.full(GUARD, SENTINEL, f32))), "%s: guard band overwritten" % what
    return h[:n]


def logical(t, n, what):
    out = raw(t, n, what)
    assert not np.isnan(out).any(), "%s: %d of %d elements unwritten or NaN" % (what, int(np.isnan(out).sum()), n)
    return out


def scalar(v):
    return dev(np.array([v], f32))


# ============================================================================= 1. Adam
# n = 4 * n4 + r.  stride = 2048 * 256 float4 groups per sweep; the paired loop `i + stride < n4` runs once n4 > S4.
S4 = SWEEP
ADAM_N4_R = [(S4 - 1, 3),        # the largest launch without pairing (n / 4 + 1 == S4: exactly 2048 blocks)
             (S4 + 1, 0),        # exactly one thread pairs
             (2 * S4, 0),        # every thread pairs once, no remainder group
             (2 * S4 + 37, 1),   # 37 threads take the remainder branch after one paired iteration
             (3 * S4 - 5, 2),
             (4 * S4 + 3, 3)]    # two paired iterations
ADAM_CAPPED = [4 * n4 + r for n4, r in ADAM_N4_R]
ADAM_IDLE_BLOCK = 4 * 768 + 1   # n / 4 == 3 * 256: the fourth block has no element at all and still owes its partial, a zero
ADAM_N = ADAM_CAPPED + [1, 3, 4, 5, 1023, ADAM_IDLE_BLOCK]
assert {r for _, r in ADAM_N4_R} == {0, 1, 2, 3}
B1, B2, EPS, L2 = 0.8, 0.999, 1e-8, 4e-5
ADAM_LR, ADAM_T, ADAM_SCALE = 0.3, 1, 0.5   # lr_t = 0.3 * sqrt(1 - 0.999) / (1 - 0.8) = 0.047


@functools.lru_cache(maxsize=None)
def _adam_inputs():
    """(p, g, m, v) of the largest case; Adam is elementwise, so every smaller case is a prefix (and any sub-range a slice)."""
    rng = np.random.default_rng(101)
    n = max(ADAM_N)
    p = rng.standard_normal(n, dtype=f32)
    g = rng.standard_normal(n, dtype=f32) * f32(0.05)
    m = rng.standard_normal(n, dtype=f32) * f32(0.05)            # non-zero
    v = (rng.random(n, dtype=f32) + f32(0.25)) * f32(0.01)       # positive
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v


@functools.lru_cache(maxsize=None)
def _adam_ref(scaled):
    """oracle.optim.adam_step, one step, on the whole input -> (p, m, v); computed once per `scaled` and never modified."""
    p, g, m, v = _adam_inputs()
    Pn, st = {"w": p.copy()}, {"m/w": m.copy(), "v/w": v.copy()}
    OO.adam_step(Pn, {"w": g}, st, ADAM_LR, ADAM_T, B1, B2, EPS, scale=ADAM_SCALE if scaled else 1.0, l2=L2)
    out = (Pn["w"], st["m/w"], st["v/w"])
    for a in out:
        a.setflags(write=False)
    # one update moves a parameter by ~ lr_t * m / sqrt(v) ~ 0.02 and m by ~ 0.2 * |g - m| ~ 0.01: thousands of times the tolerances
    # (2e-6 * max|p| ~ 1e-5, 2e-6 * max|m| ~ 5e-7), so an element that is skipped or updated twice fails
    assert np.median(np.abs(out[0] - p)) > 1000 * 2e-6 * np.abs(out[0]).max()
    assert np.median(np.abs(out[1] - m)) > 1000 * 2e-6 * np.abs(out[1]).max()
    return out


def _sumsq64(a):
    return float((np.asarray(a, np.float64) ** 2).sum())


@pytest.mark.parametrize("scaled", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_and_adam_sumsq(lib, n, scaled):
    if n in ADAM_CAPPED:
        assert lib.vc_adam_blocks(n) == 2048, "the grid cap moved: this size no longer reaches the branch it was chosen for"
    if n == ADAM_IDLE_BLOCK:
        assert lib.vc_adam_blocks(n) == (n // 4) // 256 + 1
    p0, g, m0, v0 = (a[:n] for a in _adam_inputs())
    refs = [a[:n] for a in _adam_ref(scaled)]
    lr = scalar(R.adam_lr_t(ADAM_LR, ADAM_T, B1, B2))
    sc = P(scalar(ADAM_SCALE)) if scaled else None
    tg = padded_in(g)
    for sumsq in (False, True):
        tp, tm, tv = guarded(p0), guarded(m0), guarded(v0)
        if sumsq:
            nb = lib.vc_adam_blocks(n)
            part = poisoned(nb)
            lib.vc_adam_sumsq_f32(stream(), P(tp), P(tg), P(tm), P(tv), n, P(lr), sc, B1, B2, EPS, L2, P(part))
        else:
            lib.vc_adam_f32(stream(), P(tp), P(tg), P(tm), P(tv), n, P(lr), sc, B1, B2, EPS, L2)
        for name, t, ref in zip("pmv", (tp, tm, tv), refs):
            what = "adam%s n=%d %s" % ("_sumsq" if sumsq else "", n, name)
            assert_close(logical(t, n, what), ref, 2e-6, msg=what)
        if sumsq:
            parts = logical(part, nb, "adam_sumsq partials n=%d" % n)
            assert np.isfinite(parts).all()
            np.testing.assert_allclose(parts.astype(np.float64).sum(), _sumsq64(refs[0]), rtol=1e-5)


def test_adam_sumsq_on_adjacent_subranges_of_a_flat_store(lib):
    """trainer.apply_gradients: two adjacent 16-byte-aligned sub-ranges of one flat store, each with its own range of partials."""
    lead, nA, nB, trail = 1000, 4 * (S4 + 9), 70003, 501
    total = lead + nA + nB + trail
    nbA, nbB = lib.vc_adam_blocks(nA), lib.vc_adam_blocks(nB)
    assert nbA == 2048 and nbB < 2048 and (lead * 4) % 16 == 0 and ((lead + nA) * 4) % 16 == 0
    p0, g, m0, v0 = (a[:total] for a in _adam_inputs())
    refs = [a[:total] for a in _adam_ref(False)]
    lr = scalar(R.adam_lr_t(ADAM_LR, ADAM_T, B1, B2))
    tp, tg, tm, tv = guarded(p0), padded_in(g), guarded(m0), guarded(v0)
    part = poisoned(nbA + nbB)
    for lo, n, po in ((lead, nA, 0), (lead + nA, nB, nbA)):
        lib.vc_adam_sumsq_f32(stream(), tp.data_ptr() + lo * 4, tg.data_ptr() + lo * 4, tm.data_ptr() + lo * 4, tv.data_ptr() + lo * 4,
                              n, P(lr), None, B1, B2, EPS, L2, part.data_ptr() + po * 4)
    inside = slice(lead, lead + nA + nB)
    for name, t, a0, ref in zip("pmv", (tp, tm, tv), (p0, m0, v0), refs):
        h = logical(t, total, "sub-range " + name)
        assert_close(h[inside], ref[inside], 2e-6, msg="sub-range " + name)
        assert np.array_equal(bits(h[:lead]), bits(a0[:lead])), "%s: elements before the first range changed" % name
        assert np.array_equal(bits(h[lead + nA + nB:]), bits(a0[lead + nA + nB:])), "%s: elements after the second range changed" % name
    parts = logical(part, nbA + nbB, "sub-range partials").astype(np.float64)
    np.testing.assert_allclose(parts[:nbA].sum(), _sumsq64(refs[0][lead:lead + nA]), rtol=1e-5)
    np.testing.assert_allclose(parts[nbA:].sum(), _sumsq64(refs[0][lead + nA:lead + nA + nB]), rtol=1e-5)


def test_adam_rejects_a_pointer_offset_by_four_bytes(lib):
    n = 1023
    p0, g, m0, v0 = (a[:n + 1] for a in _adam_inputs())
    lr = scalar(0.05)
    tp, tg, tm, tv = guarded(p0), guarded(g), guarded(m0), guarded(v0)
    part = poisoned(lib.vc_adam_blocks(n))
    for which in range(4):
        ptrs = [t.data_ptr() for t in (tp, tg, tm, tv)]
        ptrs[which] += 4
        with pytest.raises(VaecapError):
            lib.vc_adam_f32(stream(), *ptrs, n, P(lr), None, B1, B2, EPS, L2)
        with pytest.raises(VaecapError):
            lib.vc_adam_sumsq_f32(stream(), *ptrs, n, P(lr), None, B1, B2, EPS, L2, P(part))
    for t, a0 in ((tp, p0), (tg, g), (tm, m0), (tv, v0)):
        assert np.array_equal(bits(raw(t, n + 1, "rejected call")), bits(a0)), "a rejected call changed a buffer"
    assert np.isnan(raw(part, lib.vc_adam_blocks(n), "rejected call partials")).all()


# ============================================================================= 2. sum of squares + clip scale
@pytest.mark.parametrize("n", [0, 1, 3, 5, "sweeps"])
def test_sumsq_partial_then_clip_finalize(lib, n):
    nb = lib.vc_sumsq_blocks()
    if n == "sweeps":   # two whole sweeps of the nb x 256 float4 grid, a partly filled third one and a scalar tail
        n = 2 * nb * 256 * 4 + 4 * 300 + 3
    x = np.random.default_rng(7).standard_normal(n, dtype=f32) * f32(0.05)
    part = poisoned(nb)
    lib.vc_sumsq_partial_f32(stream(), P(padded_in(x)), n, P(part))
    parts = logical(part, nb, "sumsq partials n=%d" % n)
    assert np.isfinite(parts).all()
    ref = _sumsq64(x)
    if n == 0:
        assert np.all(parts == 0)
    np.testing.assert_allclose(parts.astype(np.float64).sum(), ref, rtol=1e-5)
    ns = poisoned(2)
    clip = 0.5 * float(np.sqrt(ref)) if n else 5.0   # norm > clip
    lib.vc_clip_finalize_f32(stream(), P(part), nb, clip, P(ns))
    norm, scale = logical(ns, 2, "norm, scale")
    np.testing.assert_allclose(norm, np.sqrt(ref), rtol=1e-5)
    if n:
        np.testing.assert_allclose(scale, OO.clip_scale(np.sqrt(ref), clip), rtol=1e-5)
        assert scale < 1.0
    else:
        assert norm == 0.0 and scale == 1.0


@pytest.mark.parametrize("regime", ["above", "below", "zero"])
@pytest.mark.parametrize("n_partial", [1, 255, 256, 257, 3 * 512 + 7])
def test_clip_finalize_partial_counts_and_norm_regimes(lib, n_partial, regime):
    clip = 5.0
    part = np.random.default_rng(n_partial).random(n_partial) + 0.5
    target = {"above": 20.0, "below": 1.25, "zero": 0.0}[regime]   # the norm
    part = (part * (target ** 2 / part.sum())).astype(f32)
    ns = poisoned(2)
    lib.vc_clip_finalize_f32(stream(), P(padded_in(part)), n_partial, clip, P(ns))
    norm, scale = logical(ns, 2, "norm, scale")
    ref = np.sqrt(part.astype(np.float64).sum())
    if regime == "zero":
        assert norm == 0.0 and scale == 1.0
        return
    np.testing.assert_allclose(norm, ref, rtol=1e-5)
    np.testing.assert_allclose(scale, OO.clip_scale(norm, clip), rtol=1e-6)   # the scale of the norm the kernel found
    if regime == "above":
        np.testing.assert_allclose(scale, OO.clip_scale(ref, clip), rtol=1e-5)
        assert scale < 0.3
    else:
        np.testing.assert_allclose(scale, OO.clip_scale(ref, clip), rtol=1e-6)   # clip * (1 / clip): no dependence on the norm


# ============================================================================= 3. SGD, Momentum
SGD_E = 150
SGD_N = SWEEP + 1000 * SGD_E + 3   # one full grid sweep plus a partial one; the last row of width E is partial


def test_sgd_beyond_one_grid_sweep(lib):
    n = SGD_N
    rng = np.random.default_rng(51)
    p0, g = rng.standard_normal(n, dtype=f32), rng.standard_normal(n, dtype=f32)
    tp = guarded(p0)
    lib.vc_sgd_f32(stream(), P(tp), P(padded_in(g)), n, P(scalar(0.1)), P(scalar(0.5)), L2)
    Pn = {"w": p0.copy()}
    OO.sgd_step(Pn, {"w": g}, 0.1, scale=0.5, l2=L2)
    assert np.median(np.abs(Pn["w"] - p0)) > 1000 * 1e-6 * np.abs(p0).max()
    assert_close(logical(tp, n, "sgd"), Pn["w"], 1e-6, msg="sgd")


@pytest.mark.parametrize("masked", [True, False], ids=["row_mask", "dense"])
def test_momentum_two_steps_beyond_one_grid_sweep(lib, masked):
    n, E = SGD_N, SGD_E
    rng = np.random.default_rng(52)
    p0, a0 = rng.standard_normal(n, dtype=f32), rng.standard_normal(n, dtype=f32) * f32(0.1)
    gs = [rng.standard_normal(n, dtype=f32) for _ in range(2)]
    rows = (n + E - 1) // E
    touched = rng.random(rows) < 0.3
    touched[[0, 2]] = False
    touched[[1, 3, SWEEP // E, rows - 1]] = True   # rows that straddle a workgroup boundary, the sweep boundary, and the partial last row
    assert any((r * E) // 256 != (r * E + E - 1) // 256 for r in np.flatnonzero(touched))
    assert (SWEEP // E) * E < SWEEP < (SWEEP // E + 1) * E
    elem = R.masked_rows(touched, n, E)
    tp, ta = guarded(p0), guarded(a0)
    tmask = P(padded_in(touched.astype(f32))) if masked else None
    Pn, st = {"e": p0.copy()}, {"a/e": a0.copy()}
    for g in gs:
        lib.vc_momentum_f32(stream(), P(tp), P(padded_in(g)), P(ta), n, P(scalar(0.1)), P(scalar(0.5)), 0.9, L2, tmask, E if masked else 0)
        OO.momentum_step(Pn, {"e": g}, st, 0.1, momentum=0.9, scale=0.5, touched={"e": elem} if masked else None, l2=L2)
    hp, ha = logical(tp, n, "momentum p"), logical(ta, n, "momentum accum")
    assert_close(hp, Pn["e"], 1e-6, msg="momentum p")
    assert_close(ha, st["a/e"], 1e-6, msg="momentum accum")
    if masked:
        assert np.array_equal(bits(hp[~elem]), bits(p0[~elem])), "an untouched row of p changed"
        assert np.array_equal(bits(ha[~elem]), bits(a0[~elem])), "an untouched row of accum changed"


# ============================================================================= 4. latent backward
def _latent_inputs(S, N, L, seed):
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((N, L), dtype=f32) * f32(0.3)
    std = np.exp(rng.standard_normal((N, L), dtype=f32) * f32(0.3)).astype(f32)
    mu_p = rng.standard_normal((N, L), dtype=f32) * f32(0.1)
    eps = rng.standard_normal((S or 5, N, L), dtype=f32)   # S == 0: five samples stand behind the sums the kernel receives
    dz = rng.standard_normal((S or 5, N, L), dtype=f32)
    return mean, std, mu_p, eps, dz


def _latent_bwd_case(lib, S, N, L, mode):
    mean, std, mu_p, eps, dz = _latent_inputs(S, N, L, 400 + 10 * S + mode)
    m64, s64, mu64 = (a.astype(np.float64) for a in (mean, std, mu_p))
    sm, ss = O.sample_z_bwd(dz.astype(np.float64), eps.astype(np.float64))
    if S == 0:   # dmean / dstd enter holding the (float32) sums and are updated in place
        sm, ss = sm.astype(f32), ss.astype(f32)
    tmean, tstd, tmu = padded_in(mean), padded_in(std), padded_in(mu_p)
    tdz, teps = (padded_in(dz), padded_in(eps)) if S else (None, None)
    for out_logstd in (0, 1):
        for ann in (0.37, None):
            a = 1.0 if ann is None else ann
            if mode == 0:
                km, ks = O.kl_normal_bwd(m64, s64, a / 10)
                kl_scale = 0.1 / N
            else:   # c_i = I, cluster means = mu_p: c_i @ means == mu_p
                km, ks = O.kl_ag_bwd(m64, s64, np.eye(N), mu64, np.full(N, a / 10))
                kl_scale = 0.1
            dm_ref, ds_ref = sm.astype(np.float64) + km, ss.astype(np.float64) + ks
            if out_logstd:
                ds_ref = ds_ref * s64
            dm, ds = (guarded(sm), guarded(ss)) if S == 0 else (poisoned(N * L), poisoned(N * L))
            lib.vc_latent_bwd_f32(stream(), S, N, L, mode, out_logstd, P(tdz), P(teps), P(tmean), P(tstd), P(tmu),
                                  None if ann is None else P(scalar(ann)), kl_scale, P(dm), P(ds))
            what = "S=%d NL=%d mode=%d logstd=%d ann=%s" % (S, N * L, mode, out_logstd, ann)
            assert_close(logical(dm, N * L, "dmean " + what), dm_ref.ravel(), 1e-5, msg="dmean " + what)
            assert_close(logical(ds, N * L, "dstd " + what), ds_ref.ravel(), 1e-5, msg="dstd " + what)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("S", [0, 1, 7, 8, 9, 16, 23, 100])
def test_latent_bwd_sample_counts(lib, S, mode):
    _latent_bwd_case(lib, S, 7, 150, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_latent_bwd_beyond_one_grid_sweep(lib, mode):
    N, L = 3500, 150
    assert N * L > SWEEP
    _latent_bwd_case(lib, 9, N, L, mode)


# ============================================================================= 5. data-parallel shard forms of the latent sample
MIXED_CASES = [(3, 5, 4, 150), (2, 7, 5, 37), (4, 6, 1, 150), (1, 50, 7, 150), (2, 1750, 2, 150)]


@pytest.mark.parametrize("case", MIXED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_latent_shard_sample_and_sums(lib, case):
    W, N, S, L = case
    Ng, nq = W * N, N * S
    if case == (2, 1750, 2, 150):
        assert nq * L > SWEEP and Ng * L > SWEEP   # both kernels stride the grid
    rng = np.random.default_rng(600 + W)
    mean = rng.standard_normal((Ng, L), dtype=f32) * f32(0.3)
    std = np.exp(rng.standard_normal((Ng, L), dtype=f32) * f32(0.3)).astype(f32)
    eps = rng.standard_normal((S, Ng, L), dtype=f32)
    dz = rng.standard_normal((S, Ng, L), dtype=f32)
    fe, fd = eps.reshape(S * Ng, L), dz.reshape(S * Ng, L)
    tmean, tstd = padded_in(mean), padded_in(std)
    # every rank reads ITS rows of the global noise / gradient through a pointer into the global device tensors
    teps, tdz = padded_in(eps), padded_in(dz)
    dm_sum, ds_sum = np.zeros((Ng, L)), np.zeros((Ng, L))
    zs = []
    for r in range(W):
        q0 = r * nq
        off = q0 * L * 4
        what = "%s rank %d" % (case, r)
        z = poisoned(nq * L)
        lib.vc_latent_sample_mixed_f32(stream(), Ng, L, q0, nq, P(tmean), P(tstd), teps.data_ptr() + off, P(z))
        hz = logical(z, nq * L, "z " + what).reshape(nq, L)
        assert_close(hz, R.sample_mixed(mean, std, fe[q0:q0 + nq], q0), 1e-6, msg="z " + what)
        zs.append(hz)
        pm, ps = poisoned(Ng * L), poisoned(Ng * L)
        lib.vc_latent_sums_mixed_f32(stream(), Ng, L, q0, nq, tdz.data_ptr() + off, teps.data_ptr() + off, P(pm), P(ps))
        hm, hs = logical(pm, Ng * L, "dmean_part " + what).reshape(Ng, L), logical(ps, Ng * L, "dstd_part " + what).reshape(Ng, L)
        rm, rs = R.sums_mixed(fd[q0:q0 + nq], fe[q0:q0 + nq], Ng, q0)
        assert_close(hm, rm, 1e-6, msg="dmean_part " + what)
        assert_close(hs, rs, 1e-6, msg="dstd_part " + what)
        occurs = np.zeros(Ng, bool)
        occurs[(q0 + np.arange(nq)) % Ng] = True
        if case == (4, 6, 1, 150):
            assert occurs.sum() == N and np.array_equal(np.flatnonzero(occurs), np.arange(q0, q0 + nq))
        assert np.all(hm[~occurs] == 0.0) and np.all(hs[~occurs] == 0.0), "a global row outside the rank's range is not exactly zero"
        dm_sum += hm
        ds_sum += hs
    dm_ref, ds_ref = O.sample_z_bwd(dz.astype(np.float64), eps.astype(np.float64))
    assert_close(dm_sum, dm_ref, 1e-5, msg="sum of the ranks' dmean partials")
    assert_close(ds_sum, ds_ref, 1e-5, msg="sum of the ranks' dstd partials")
    zg = np.concatenate(zs).reshape(S, Ng, L)
    assert_close(zg, O.sample_z_fwd(mean.astype(np.float64), std.astype(np.float64), eps.astype(np.float64)), 1e-6, msg="ranks' z, concatenated")
    if W == 1:   # Ng = N, q0 = 0, nq = S * N: the single-rank kernel
        z1 = poisoned(S * N * L)
        lib.vc_latent_sample_f32(stream(), S, N, L, P(tmean), P(tstd), P(teps), P(z1))
        assert_close(logical(z1, S * N * L, "vc_latent_sample_f32").reshape(S, N, L), zg, 1e-6, msg="shard form against vc_latent_sample_f32")


# ============================================================================= 6. reductions and small ops
COLSUM_CASES = [(3, 1, 1804),        # the gathered label counts: rows = world, cols = 1, ld = 2*N*L + 4 (scalar path, one chunk)
                (1, 3, 3),
                (63, 64, 64),        # rows < 64: rows / 64 == 0 chunks, clamped to one
                (64, 65, 65),        # a second column block of one column, scalar path
                (65, 150, 152),
                (5000, 300, 304),    # the vector path with a padded pitch
                (16385, 64, 64),     # narrow matrix: the chunks > 256 clamp
                (20000, 4100, 4100), # 65 column blocks: chunks capped by 2048 / 65 workgroups
                (0, 8, 8)]


def _colsum_case(lib, rows, cols, ld, offset=0):
    """offset: floats by which the base pointer is moved off its 16-byte alignment"""
    rng = np.random.default_rng(31 + rows + cols)
    # values ~ 1 +- 0.5: column sums do not cancel, so max|ref| is the scale of the terms that were added
    data = rng.standard_normal((rows, cols), dtype=f32)
    data *= f32(0.5)
    data += f32(1.0)
    buf = np.full(offset + max(rows, 1) * ld + GUARD, NAN, f32)   # pitch padding, the offset and the tail hold NaN
    if rows:
        buf[offset:offset + rows * ld].reshape(rows, ld)[:, :cols] = data
    tx = dev(buf)
    px = tx.data_ptr() + offset * 4
    ref = data.sum(0, dtype=np.float64)
    nbytes = lib.vc_colsum_workspace_bytes(rows, cols)
    assert nbytes % (4 * cols) == 0
    chunks = nbytes // (4 * cols)
    if rows < 64:
        assert chunks == 1
    if (rows, cols) == (16385, 64):
        assert chunks == 256, "the narrow-matrix clamp moved: this case no longer reaches it"
    if (rows, cols) == (20000, 4100):
        assert chunks == 2048 // 65
    o0 = rng.standard_normal(cols, dtype=f32)
    what = "colsum %dx%d ld=%d offset=%d" % (rows, cols, ld, offset)
    for accumulate in (0, 1):
        out = guarded(o0) if accumulate else poisoned(cols)
        ws = poisoned(nbytes // 4)
        lib.vc_colsum_f32(stream(), px, rows, cols, ld, P(out), accumulate, P(ws), nbytes)
        logical(ws, nbytes // 4, what + " workspace")
        assert_close(logical(out, cols, what), ref + (o0 if accumulate else 0), 1e-5, msg="%s accumulate=%d" % (what, accumulate))
    out, ws = poisoned(cols), poisoned(nbytes // 4)
    with pytest.raises(VaecapError, match="workspace"):
        lib.vc_colsum_f32(stream(), px, rows, cols, ld, P(out), 0, P(ws), nbytes - 4)
    assert np.isnan(raw(out, cols, what + " after the rejected call")).all(), "a rejected call wrote the output"


@pytest.mark.parametrize("case", COLSUM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_colsum_shapes(lib, case):
    _colsum_case(lib, *case)


def test_colsum_misaligned_base_takes_the_scalar_path(lib):
    _colsum_case(lib, 5000, 300, 301, offset=1)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 48000])
def test_reduce_sum_and_count_nonzero(lib, n, accumulate):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n, dtype=f32)
    scale, o0 = -0.37, f32(2.5)
    out = guarded([o0]) if accumulate else poisoned(1)
    lib.vc_reduce_sum_f32(stream(), P(padded_in(x)), n, scale, P(out), accumulate)
    ref = float(f32(scale)) * x.astype(np.float64).sum() + (float(o0) if accumulate else 0.0)
    # one workgroup: <= ceil(n / 1024) serial additions per thread, then a 10-level tree: the error is below
    # (n / 1024 + 11) * 2^-24 * sum|x| <= 58 * 2^-24 * sum|x| = 3.5e-6 * sum|x| at n = 48000; 1e-5 is the suite's bound for sums
    tol = 1e-5 * (abs(scale) * np.abs(x).astype(np.float64).sum() + (abs(float(o0)) if accumulate else 0.0))
    got = float(logical(out, 1, "reduce_sum n=%d" % n)[0])
    assert abs(got - ref) <= tol, (got, ref, tol)
    if accumulate:
        return
    ids = rng.integers(-3, 4, size=n).astype(np.int32)   # negative ids count as non-zero
    ids[0] = -1 if n % 2 else 0
    cnt = poisoned(1)
    lib.vc_count_nonzero_i32(stream(), P(padded_in(ids, np.int32, pad=7)), n, P(cnt))
    assert logical(cnt, 1, "count_nonzero")[0] == float((ids != 0).sum())   # exact (counts < 2^24)


@pytest.mark.parametrize("n", [1, SWEEP + 5])
def test_axpy_and_fill(lib, n):
    rng = np.random.default_rng(n)
    x, y0 = rng.standard_normal(n, dtype=f32), rng.standard_normal(n, dtype=f32)
    y = guarded(y0)
    lib.vc_axpy_f32(stream(), -1.75, P(padded_in(x)), n, P(y))
    # y + a * x in one or two roundings (fused or not): the error of an element is at most 2 * 2^-24 * (|y| + |a x|) = 1.2e-7 of the
    # terms that were added, so the bound is 1e-6 relative to max(|y| + |a x|), not to max|ref| (the largest terms may cancel)
    ref = y0.astype(np.float64) - 1.75 * x.astype(np.float64)
    assert_close(logical(y, n, "axpy"), ref, 1e-6, atol_scale=float((np.abs(y0) + 1.75 * np.abs(x)).max()), msg="axpy n=%d" % n)
    t = poisoned(n)
    lib.vc_fill_f32(stream(), P(t), n, 0.7)
    assert np.array_equal(bits(logical(t, n, "fill")), bits(np.full(n, 0.7, f32)))


@pytest.mark.parametrize("B", [3, 3500])
def test_tile_rows_and_segment_sum(lib, B):
    nc, E = 5, 150
    if B == 3500:
        assert B * E > SWEEP
    rng = np.random.default_rng(B)
    f = rng.standard_normal((B, E), dtype=f32)
    t = poisoned(B * nc * E)
    lib.vc_tile_rows_f32(stream(), P(padded_in(f)), B, nc, E, P(t))
    assert np.array_equal(bits(logical(t, B * nc * E, "tile_rows").reshape(B * nc, E)), bits(np.repeat(f, nc, axis=0)))
    g = rng.standard_normal((B * nc, E), dtype=f32)
    ref = g.astype(np.float64).reshape(B, nc, E).sum(1)
    x0 = rng.standard_normal((B, E), dtype=f32)
    tg = padded_in(g)
    for accumulate in (0, 1):
        s = guarded(x0) if accumulate else poisoned(B * E)
        lib.vc_segment_sum_rows_f32(stream(), P(tg), B, nc, E, P(s), accumulate)
        assert_close(logical(s, B * E, "segment sum").reshape(B, E), ref + (x0 if accumulate else 0), 1e-6,
                     msg="segment sum B=%d accumulate=%d" % (B, accumulate))


@pytest.mark.parametrize("combo", ["all", "no_reg", "no_kl", "no_ann"])
def test_loss_finalize(lib, combo):
    ce_num, ce_den, reg, reg_scale, kl_sum, inv_n, ann = 913.25, 217.0, 8123.5, 2e-5, 345.75, 1.0 / 35, 0.37
    use_reg, use_kl, use_ann = combo != "no_reg", combo != "no_kl", combo != "no_ann"
    out = poisoned(4)
    lib.vc_loss_finalize_f32(stream(), P(scalar(ce_num)), P(scalar(ce_den)), P(scalar(reg)) if use_reg else None, reg_scale,
                             P(scalar(kl_sum)) if use_kl else None, inv_n, P(scalar(ann)) if use_ann else None, P(out))
    got = logical(out, 4, "loss scalars " + combo)
    ref = R.loss_scalars(ce_num, ce_den, reg if use_reg else None, reg_scale, kl_sum if use_kl else None, inv_n, ann if use_ann else None)
    # positive terms, at most six float32 roundings per scalar: 6 * 2^-24 = 3.6e-7 relative
    np.testing.assert_allclose(got, ref, rtol=1e-6)
    if not use_kl:
        assert got[2] == got[0] and got[1] == 0.0
    if not use_ann:
        assert got[3] == 1.0
    else:
        assert got[3] == f32(ann)


@pytest.mark.parametrize("decay_steps,ann_on", [(100, 1), (0, 0)])
@pytest.mark.parametrize("gs", [0, 1, 2, 99, 100, 20000])
def test_step_update(lib, gs, decay_steps, ann_on):
    lr, cnn_lr, ann_param = 5e-4, 1e-5, 2.0
    step = dev(np.array([gs], np.int32))
    s = poisoned(5)
    lib.vc_step_update(stream(), P(step), P(s), lr, cnn_lr, B1, B2, ann_param, ann_on, decay_steps)
    got = logical(s, 5, "step scalars").astype(np.float64)
    assert host(step)[0] == gs + 1
    ref = R.step_scalars(gs, lr, cnn_lr, B1, B2, ann_param, ann_on, decay_steps)
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-4)
    if not ann_on:
        assert got[1] == 1.0
    # (the reference rounded to the output's format: 0.5^200 is below the float32 range)
    np.testing.assert_allclose(got[2], f32(ref[2]), rtol=1e-6)
    np.testing.assert_allclose(got[4], f32(ref[4]), rtol=1e-6)
    # lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t): powf returns b^t to within 2 ulp <= 2^-22 ABSOLUTE (b^t < 1), and 1 - b^t cancels at small
    # t, so the relative error of each difference is 2^-22 / (1 - b^t) (the square root halves the first; kept whole); the subtraction, the
    # square root, the division and the product add one rounding of 2^-24 each, bounded by 4 * 2^-23
    t = gs + 1
    b1, b2 = float(f32(B1)), float(f32(B2))
    bound = 2.0 ** -22 / (1 - b2 ** t) + 2.0 ** -22 / (1 - b1 ** t) + 4 * 2.0 ** -23
    for k in (0, 3):
        assert abs(got[k] - ref[k]) <= ref[k] * bound, (k, got[k], ref[k], bound)
