"""CPU: the float64 reference of stochastic beam search (tests/sbs_ref.py) -- its identities, the statistics of what it samples, the
importance weights, and the proof that the parity cases tests/test_gpu_sbs.py runs on the device are safe to compare exactly."""
import functools

import numpy as np
import pytest

from . import sbs_ref as R


def table_search(tables, B, n, rng):
    """B independent searches of width n over the table model, as ONE batch of B images"""
    L = R.T_LEN + 1
    logits = lambda st: R.table_logits(tables, st["sent"].reshape(B * n, L), st["len"].reshape(-1))
    return R.search(logits, lambda it: rng.gumbel(size=(B * n, R.T_V)), B, n, R.T_V, L, R.T_BOS, R.T_EOS)


@functools.lru_cache(maxsize=None)
def table_runs(seed):
    tables = R.table_model()
    caps, p = R.table_captions(tables)
    st = table_search(tables, 4096, 2, np.random.default_rng(seed))
    return R.results(st, R.T_EOS), caps, p


def test_the_table_model_has_forty_captions():
    caps, p = R.table_captions(R.table_model())
    assert len(caps) == len(set(caps)) == 40 and abs(p.sum() - 1.0) < 1e-12
    assert abs(R.inclusion_n2(p).sum() - 2.0) < 1e-12


def test_the_maximum_of_the_conditioned_children_is_the_parent():
    rng = np.random.default_rng(0)
    for _ in range(200):
        V = int(rng.integers(2, 50))
        Gt = rng.normal(0, 3, V) + rng.gumbel(size=V)
        G_i = float(rng.normal(0, 5))
        Gp = R.conditioned(G_i, Gt, Gt.max())
        assert Gp.max() == G_i and int(np.argmax(Gp)) == int(np.argmax(Gt)) and not np.isnan(Gp).any()
        assert (np.argsort(-Gp) == np.argsort(-Gt)).all()   # monotone
        # the unstable form, where it can be evaluated
        plain = -np.log(np.exp(-G_i) - np.exp(-Gt.max()) + np.exp(-Gt))
        np.testing.assert_allclose(Gp, plain, rtol=1e-6, atol=1e-6)
    assert R.conditioned(1.5, np.array([-np.inf, 2.0]), 2.0).tolist() == [-np.inf, 1.5]


def test_width_one_is_ancestral_sampling_by_gumbel_max():
    tables = R.table_model()
    rng = np.random.default_rng(3)
    noise = rng.gumbel(size=(R.T_LEN, 64, R.T_V))
    L = R.T_LEN + 1
    st = R.search(lambda s: R.table_logits(tables, s["sent"].reshape(64, L), s["len"].reshape(-1)), lambda it: noise[it], 64, 1, R.T_V, L,
                  R.T_BOS, R.T_EOS)
    for b, (kappa, caps) in enumerate(R.results(st, R.T_EOS)):
        (words, phi, G, ended, w, nw), = caps
        want, lp = [], 0.0
        while len(want) < R.T_LEN and (not want or want[-1] != R.T_EOS):
            l = R.lsm64(tables[len(want)][tuple(want)])
            v = int(np.argmax(l + noise[len(want), b]))
            lp += l[v]
            want.append(v)
        assert words == want and G == 0.0 and abs(phi - lp) < 1e-12 and nw == 1.0 and kappa < 0.0


def test_a_beam_as_wide_as_the_support_enumerates_it():
    tables = R.table_model()
    caps, p = R.table_captions(tables)
    for n in (40, 45):
        st = table_search(tables, 3, n, np.random.default_rng(n))
        for kappa, got in R.results(st, R.T_EOS):
            assert kappa == -np.inf and sorted(tuple(c[0]) for c in got) == sorted(caps)
            for c in got:
                np.testing.assert_allclose(c[4], p[caps.index(tuple(c[0]))], rtol=1e-12)   # q = 1: the weight is the probability
            np.testing.assert_allclose(sum(c[5] for c in got), 1.0, rtol=1e-12)


def test_weights():
    w, nw = R.sbs_weights([-1.0, -2.0], -np.inf)
    np.testing.assert_allclose(w, np.exp([-1.0, -2.0]))
    w, nw = R.sbs_weights([-1.0, -30.0], -3.0)
    q = 1.0 - np.exp(-np.exp(np.array([-1.0, -30.0]) + 3.0))
    np.testing.assert_allclose(w[0], np.exp(-1.0) / q[0], rtol=1e-12)   # (1 - exp(-x) cancels for the tiny x of the second: expm1 does not)
    np.testing.assert_allclose(nw.sum(), 1.0)
    np.testing.assert_allclose(w[1], np.exp(-3.0), rtol=1e-6)   # an improbable caption weighs exp(kappa)
    from vae_captioning_amd.generate import sbs_weights
    for a, b in zip(sbs_weights([-1.0, -30.0], -3.0), (w, nw)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_reference_samples_without_replacement(seed):
    """4096 searches of width 2 per seed over the 40 captions: the first-ranked caption is distributed as p (chi-square, 39 degrees of
    freedom, below its 99.9 % point 72.05); every caption's inclusion count is within 4.5 standard deviations of exact sampling
    without replacement; the weighted estimate of E[len] agrees with the enumeration within 4.5 of ITS standard errors"""
    res, caps, p = table_runs(seed)
    chi2, worst, est = R.table_stats(res, caps, p)
    print("seed %d: chi-square %.1f, largest inclusion deviation %.2f sd" % (seed, chi2, worst))
    assert chi2 < 72.05 and worst < 4.5
    exact = float(sum(pc * len(c) for c, pc in zip(caps, p)))
    se = est.std(ddof=1) / np.sqrt(est.size)
    print("E[len]: exact %.5f, estimate %.5f +- %.5f" % (exact, est.mean(), se))
    assert abs(est.mean() - exact) < 4.5 * se


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_committed_parity_cases_are_safe(name):
    """every case of tests/test_gpu_sbs.py: the float32-lsm and float64 references select the same candidates in every round, every
    taken G' is at least 1e-3 above the best untaken one, and the orders inside the beam and inside a row have their margins"""
    safe, facts = R.case_margins(name)
    assert safe, facts
    B, n, V, L, rounds, bias, seed = R.CASES[name]
    if name == "finished-carried-then-evicted":
        assert facts["carried"] > 0 and facts["evicted"] > 0, facts
    if name == "longer-than-a-wave":
        assert facts["finished"] == 0 and rounds > 64
    if name == "kc-is-V":
        assert min(n + 1, V) == V   # every word of the vocabulary is a candidate
    assert R.find_seed(name, tries=seed + 1, want=lambda f: name != "finished-carried-then-evicted" or (f["carried"] > 0 and f["evicted"] > 0))[0] == seed
