"""CPU: unlikelihood training -- the float64 reference against itself (hand-derived gradient vs torch autograd), the candidate-set
rules on hand-written label grids, the flags, and the behaviour case's seed."""
import pickle

import numpy as np
import pytest
import torch

from vae_captioning_amd.utils.parameters import Parameters

from . import unlikelihood_ref as R

NEW_DEFAULTS = dict(unlikelihood=0.0, ul_window=128)


# ------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize("window", [1, 2, 128])
@pytest.mark.parametrize("eps,alpha", [(0.0, 0.5), (0.1, 2.0)])
def test_hand_derived_gradient_is_autograd(eps, alpha, window):
    buf, labels = R.ul_case(203, 204, 0)
    x = buf[:, :203].astype(np.float64)
    x[3, 1] += 40.0     # row 3 = (t = 1, n = 0): label V - 1, sole candidate word 1 -- pushed into the clamp
    c = R.ul_rows(x, labels, eps, alpha, window, gscale=3.0)
    assert c["min_om"] <= R.CLAMP    # the clamped branch is in the case
    xt = torch.tensor(x, requires_grad=True)
    R.torch_row_loss(xt, labels, eps, alpha, window, gscale=3.0).backward()
    g = xt.grad.numpy()
    assert np.abs(c["dlogits"] - g).max() <= 1e-9 * np.abs(g).max()
    # the clamped candidate has no term of its own (and R = 0: it was the only one): its gradient is the softmax part alone
    k = 3.0 / float((labels > 0).sum())
    p = np.exp(x[3] - x[3].max()); p /= p.sum()
    assert abs(c["dlogits"][3, 1] - k * (p[1] - eps / 203)) <= 1e-12
    assert c["row_ul"][3] == pytest.approx(-np.log(R.CLAMP), rel=1e-12)


def test_reference_without_candidates_is_the_smoothed_loss():
    from .objective_ref import smooth_xent
    buf, labels = R.ul_case(203, 204, 0)
    x = buf[:, :203]
    y = labels.reshape(-1)
    c = R.ul_rows(x, labels, 0.1, 1e-30, 128, gscale=2.0)
    loss, d = smooth_xent(x, y, 0.1, 2.0)
    np.testing.assert_allclose(c["row_loss"], loss, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(c["dlogits"], d, rtol=1e-9, atol=1e-15)


# ------------------------------------------------------------------------------------------------ candidate sets
def _sets(labels, V, window):
    T, N = np.asarray(labels).shape
    s = R.candidate_sets(labels, V, window)
    return [[list(s[t * N + n]) for n in range(N)] for t in range(T)]


def test_candidate_rules_on_hand_written_grids():
    V = 50
    g = np.array([[5, 7], [6, 7], [5, 8], [9, 0], [5, 49], [0, 50], [3, -2], [4, 9]], np.int32)   # [T = 8, N = 2]
    s = _sets(g, V, 128)
    assert s[0] == [[], []]                                   # t = 0
    assert s[1] == [[5], []]                                  # an earlier word equal to the label is excluded
    assert s[2] == [[6], [7]]                                 # ... and so is the label's own earlier occurrence; 7 twice -> once
    assert s[3] == [[5, 6], []]                               # a PAD row has no candidates
    assert s[4] == [[6, 9], [7, 8]]                           # PAD (0) is never a candidate
    assert s[5] == [[], []]                                   # label 0 and label >= V: not live
    assert s[6] == [[5, 6, 9], []]                            # negative label: not live
    assert s[7] == [[3, 5, 6, 9], [7, 8, 49]]                 # values <= 0 and >= V are never candidates; V - 1 is
    w2 = _sets(g, V, 2)
    assert w2[4] == [[9], [8]] and w2[7] == [[3], []] and w2[2] == [[6], [7]]
    w1 = _sets(g, V, 1)
    assert w1[1] == [[5], []] and w1[2] == [[6], [7]] and w1[7] == [[3], []]
    M = R.candidate_mask(g, V, 128)
    assert M.shape == (16, V) and M.sum() == sum(len(c) for row in s for c in row)


def test_the_kernel_grid_holds_every_case_it_promises():
    V = 203
    buf, labels = R.ul_case(V, 204, 0)
    s = _sets(labels, V, 128)
    assert all(s[0][n] == [] for n in range(3))                                # t = 0
    assert (labels[:4, 0] == 1).sum() == 3 and s[4][0] == [1, V - 1]           # a word three times, once in the set; columns 1 and V - 1
    assert labels[2, 0] == 1 and 1 not in s[2][0]                              # earlier word equal to the label
    assert labels[6, 0] == 0 and (labels[5:, 1] == 0).all()                    # PAD tails
    assert s[3][1] == [20, 21, 22] and labels[3, 1] // 4 == 20 // 4            # candidates in the label's float4, several in one
    assert R.ul_rows(buf[:, :V], labels, 0.0, 1.0, 128)["min_om"] >= R.MIN_OM


# ------------------------------------------------------------------------------------------------ flags
def test_flags_parse_and_default_to_off():
    p = Parameters().parse_args([])
    for k, v in NEW_DEFAULTS.items():
        assert getattr(p, k) == v and k in vars(p), k
    p = Parameters().parse_args("--unlikelihood 0.5 --ul_window 4".split())
    assert (p.unlikelihood, p.ul_window) == (0.5, 4)
    for extra in ("--no_encoder", "--fine_tune", "--sched_sampling 0.5", "--label_smoothing 0.1 --kl_free_bits 0.05", "--prior GMM", "--prior AG --c_v",
                  "--ul_window 1", "--ul_window 128"):
        p = Parameters().parse_args(["--unlikelihood", "1"] + extra.split())
        assert p.unlikelihood == 1.0


@pytest.mark.parametrize("argv", [
    "--unlikelihood -0.1", "--unlikelihood inf", "--unlikelihood nan", "--unlikelihood 1 --ul_window 0", "--unlikelihood 1 --ul_window 129",
    "--ul_window 4", "--unlikelihood 0 --ul_window 4", "--unlikelihood 1 --scst",
], ids=lambda a: a.replace(" ", "_"))
def test_parse_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        Parameters().parse_args(argv.split())
    assert e.value.code == 2
    assert "--" in capsys.readouterr().err


def test_defaults_leave_parameters_as_they_were():
    """every attribute but the two new ones parses to what it parsed to before, and an old pickle loads with the feature off"""
    p = Parameters().parse_args([])
    q = Parameters().parse_args("--unlikelihood 1 --ul_window 7".split())
    assert {k: v for k, v in vars(p).items() if k not in NEW_DEFAULTS} == {k: v for k, v in vars(q).items() if k not in NEW_DEFAULTS}
    old = Parameters()
    assert not any(k in vars(old) for k in NEW_DEFAULTS)
    old = pickle.loads(pickle.dumps(old))
    for k, v in NEW_DEFAULTS.items():
        assert getattr(old, k) == v, k


# ------------------------------------------------------------------------------------------------ behaviour case
def test_behaviour_seed_separates_the_two_runs_in_the_reference():
    """the seed of the behaviour test (tests/test_gpu_unlikelihood.py) was chosen with the reference alone: after the same steps from
    the same start, the probability on already-said words differs by at least 10 % between alpha = 1 and alpha = 0"""
    from .test_gpu_engine import make_case, small_params
    b = R.BEHAVIOUR
    mass = {}
    for alpha in (1.0, 0.0):
        p = small_params(prior=b["prior"], unlikelihood=alpha)
        P0, batch, noise = make_case(p, b["V"], b["B"], b["T"], seed=b["seed"])
        _, Pend = R.reference_steps(p, P0, batch, noise, b["steps"], grads=False)
        mass[alpha] = R.reference_repeat_mass(p, Pend, batch, noise)
    print("reference repeat_mass after %d steps: alpha=1 %.6g, alpha=0 %.6g" % (b["steps"], mass[1.0], mass[0.0]))
    assert mass[1.0] < mass[0.0]
    assert (mass[0.0] - mass[1.0]) / mass[0.0] >= 0.10, mass
