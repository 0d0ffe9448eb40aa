"""CPU: pins tests/step_tail_ref.py (the references of tests/test_gpu_step_tail.py) to the oracle.

The shard forms of the latent sample are DEFINED by the single-rank operation on the global tensors: the ranks' samples, concatenated in
rank order, are the global sample, and the ranks' partial sums add up to the global gradient.  The step scalars are pinned to the float32
expressions of oracle/optim.py."""
import numpy as np
import pytest

from oracle import ops as O
from oracle import optim as OO

from . import step_tail_ref as R

# (W ranks, N rows per rank, S samples, L): (3, 5, 4) has q0 % Ng != 0 and nq % Ng != 0; (4, 6, 1) has nq < Ng (rows that do not occur)
CASES = [(3, 5, 4, 150), (4, 6, 1, 150), (2, 7, 5, 37), (1, 50, 7, 150), (5, 3, 3, 4), (2, 1, 1, 1), (3, 4, 6, 20)]


def _global(W, N, S, L, seed):
    rng = np.random.default_rng(seed)
    Ng = W * N
    mean = rng.standard_normal((Ng, L))
    std = np.exp(0.3 * rng.standard_normal((Ng, L)))
    eps = rng.standard_normal((S, Ng, L))
    dz = rng.standard_normal((S, Ng, L))
    return mean, std, eps, dz


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_rank_samples_concatenate_to_the_global_sample(case):
    W, N, S, L = case
    Ng, nq = W * N, N * S
    mean, std, eps, _ = _global(W, N, S, L, 5)
    flat = eps.reshape(S * Ng, L)
    z = np.concatenate([R.sample_mixed(mean, std, flat[r * nq:(r + 1) * nq], r * nq) for r in range(W)])
    assert z.shape == (S * Ng, L)
    np.testing.assert_array_equal(z.reshape(S, Ng, L), O.sample_z_fwd(mean, std, eps))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_rank_partial_sums_add_up_to_the_global_gradient(case):
    W, N, S, L = case
    Ng, nq = W * N, N * S
    _, _, eps, dz = _global(W, N, S, L, 6)
    fe, fd = eps.reshape(S * Ng, L), dz.reshape(S * Ng, L)
    dm, ds = np.zeros((Ng, L)), np.zeros((Ng, L))
    for r in range(W):
        pm, ps = R.sums_mixed(fd[r * nq:(r + 1) * nq], fe[r * nq:(r + 1) * nq], Ng, r * nq)
        occurs = np.zeros(Ng, bool)
        occurs[(r * nq + np.arange(nq)) % Ng] = True
        assert np.all(pm[~occurs] == 0) and np.all(ps[~occurs] == 0)   # rows this rank does not hold: zeros
        dm += pm
        ds += ps
    dm_ref, ds_ref = O.sample_z_bwd(dz, eps)
    # the same float64 terms in another order: a few ulp of the S-term sums
    np.testing.assert_allclose(dm, dm_ref, rtol=0, atol=1e-13 * S)
    np.testing.assert_allclose(ds, ds_ref, rtol=0, atol=1e-12 * S)


def test_the_named_cases_reach_the_first_row_branches():
    W, N, S = 3, 5, 4
    assert any((r * N * S) % (W * N) != 0 for r in range(W)) and (N * S) % (W * N) != 0
    W, N, S = 4, 6, 1
    assert N * S < W * N


@pytest.mark.parametrize("gs", [0, 1, 2, 99, 100, 20000])
def test_step_scalars_agree_with_the_oracle_expressions(gs):
    lr, cnn_lr, b1, b2 = 5e-4, 1e-5, 0.8, 0.999
    s = R.step_scalars(gs, lr, cnn_lr, b1, b2, 2.0, 1, 100)
    # the oracle evaluates lr_t in float32: 1 - b2^t carries a rounding of 2^-24 relative to b2^t ~ 1, amplified by 1 / (1 - b2^t)
    t = gs + 1
    tol = 2.0 ** -23 / (1 - 0.999 ** t) + 2.0 ** -23 / (1 - 0.8 ** t) + 8 * 2.0 ** -24
    assert abs(float(R.adam_lr_t(lr, t, b1, b2)) - s[0]) <= tol * s[0]
    assert abs(float(R.adam_lr_t(cnn_lr, t, b1, b2)) - s[3]) <= tol * s[3]
    np.testing.assert_allclose(s[1], (np.tanh((gs - 2000.0) / 1000) + 1) / 2, rtol=1e-12)
    np.testing.assert_allclose(s[2], float(np.float32(lr)) * 0.5 ** (gs // 100), rtol=1e-12)
    np.testing.assert_allclose(s[4], float(np.float32(cnn_lr)) * 0.5 ** (gs // 100), rtol=1e-12)
    assert R.step_scalars(gs, lr, cnn_lr, b1, b2, 2.0, 0, 0)[1] == 1.0
    assert R.step_scalars(gs, lr, cnn_lr, b1, b2, 2.0, 0, 0)[2] == float(np.float32(lr))


def test_decayed_lr_of_the_oracle_is_the_staircase():
    # oracle.optim.decayed_lr at its own decay_steps
    ds = int(150000 / (32 + 0.001) * 5)
    for gs in (0, ds - 1, ds, 3 * ds + 7):
        np.testing.assert_allclose(R.step_scalars(gs, 5e-4, 1e-5, 0.8, 0.999, 2.0, 1, ds)[2], float(OO.decayed_lr(5e-4, gs)), rtol=1e-6)


def test_loss_scalars_and_row_mask():
    s = R.loss_scalars(6.0, 3.0, reg=2.0, reg_scale=0.5, kl_sum=40.0, inv_n=0.25, ann=0.5)
    np.testing.assert_allclose(s, [3.0, 10.0, 3.5, 0.5])
    s = R.loss_scalars(6.0, 3.0)
    np.testing.assert_allclose(s, [2.0, 0.0, 2.0, 1.0])
    m = R.masked_rows([1, 0, 1], 7, 3)
    np.testing.assert_array_equal(m, [True] * 3 + [False] * 3 + [True])
