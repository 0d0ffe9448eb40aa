"""CPU: scheduled sampling's host side -- the flags and their parse errors, objective.sched_rate against the float64 reference
(tests/sched_ref.py) on a step grid, the reference mix at its edges, and the C-ABI entry's declaration and argument errors (argument
validation happens before any device work, so it is testable without a GPU)."""
import ctypes
import pickle

import numpy as np
import pytest

from vae_captioning_amd import abi, objective
from vae_captioning_amd.utils.parameters import Parameters

from . import sched_ref as R

NEW_DEFAULTS = dict(sched_sampling=0.0, sched_schedule="linear", sched_ramp_steps=10000, sched_pick="sample", sched_temperature=1.0)


# ------------------------------------------------------------------------------------------------ flags
def test_flags_parse_and_default_to_off():
    p = Parameters().parse_args([])
    for k, v in NEW_DEFAULTS.items():
        assert getattr(p, k) == v and k in vars(p), k   # materialised on the instance (--save_params pickles vars(p))
    assert pickle.loads(pickle.dumps(p)).sched_sampling == 0.0
    p = Parameters().parse_args("--sched_sampling 0.25 --sched_schedule sigmoid --sched_ramp_steps 500 --sched_pick argmax".split())
    assert (p.sched_sampling, p.sched_schedule, p.sched_ramp_steps, p.sched_pick, p.sched_temperature) == (0.25, "sigmoid", 500, "argmax", 1.0)
    p = Parameters().parse_args("--sched_sampling 1 --sched_schedule constant --sched_temperature 0.7".split())
    assert (p.sched_sampling, p.sched_schedule, p.sched_temperature) == (1.0, "constant", 0.7)


@pytest.mark.parametrize("argv", [
    "--sched_sampling 0.3 --no_encoder",
    "--sched_sampling 0.3 --prior GMM",
    "--sched_sampling 0.3 --prior AG --c_v",
    "--sched_sampling 0.3 --fine_tune",
    "--sched_sampling 0.3 --kl_free_bits 0.05 --kl_weight 0.5 --kl_cycle_steps 100 --label_smoothing 0.1 --word_drop 0.2",
    "--sched_sampling 0.3 --restore --ann_param 2",
], ids=lambda a: a.replace(" ", "_"))
def test_accepted_combinations(argv):
    assert Parameters().parse_args(argv.split()).sched_sampling == 0.3


@pytest.mark.parametrize("argv", [
    "--sched_sampling -0.1", "--sched_sampling 1.5", "--sched_sampling nan",
    "--sched_schedule linear", "--sched_ramp_steps 100", "--sched_pick argmax", "--sched_temperature 0.5",   # subsidiary flags alone
    "--sched_sampling 0 --sched_schedule constant",
    "--sched_sampling 0.3 --sched_schedule cosine",
    "--sched_sampling 0.3 --sched_ramp_steps 0",
    "--sched_sampling 0.3 --sched_pick beam",
    "--sched_sampling 0.3 --sched_temperature 0", "--sched_sampling 0.3 --sched_temperature -1", "--sched_sampling 0.3 --sched_temperature inf",
    "--sched_sampling 0.3 --scst",
    "--sched_sampling 0.3 --mode inference",
], ids=lambda a: a.replace(" ", "_"))
def test_parse_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        Parameters().parse_args(argv.split())
    assert e.value.code == 2
    assert "--" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("ramp", [1, 2, 100, 10000])
@pytest.mark.parametrize("rate_max", [0.0, 0.25, 1.0])
def test_sched_rate_equals_the_reference(rate_max, ramp):
    grid = [0, 1, 2, ramp - 1, ramp, ramp + 1, 3 * ramp, 10 * ramp, 1000 * ramp, 10 ** 9]
    for sch in R.SCHEDULES:
        for s in grid:
            got, ref = objective.sched_rate(s, sch, rate_max, ramp), R.sched_rate(s, sch, rate_max, ramp)
            assert got == pytest.approx(ref, rel=1e-12, abs=1e-15), (sch, s)
            assert objective.sched_rate(s, R.SCHEDULES.index(sch), rate_max, ramp) == got   # by index, as the C ABI takes it
            assert 0.0 <= got <= rate_max
    assert objective.sched_rate(0, "linear", rate_max, ramp) == 0.0
    assert objective.sched_rate(ramp, "linear", rate_max, ramp) == rate_max
    assert objective.sched_rate(10 ** 9, "sigmoid", rate_max, ramp) == rate_max        # far behind the ramp: no overflow, the full rate
    assert objective.sched_rate(0, "sigmoid", rate_max, ramp) == pytest.approx(rate_max / (ramp + 1.0), rel=1e-12)
    for bad in (0, -5, 12345):   # the constant schedule ignores the ramp
        assert objective.sched_rate(7, "constant", rate_max, bad) == rate_max


def test_sched_rate_rises_monotonically_and_rejects_bad_arguments():
    for sch in ("linear", "sigmoid"):
        r = [objective.sched_rate(s, sch, 0.8, 50) for s in range(0, 2000, 7)]
        assert all(b >= a for a, b in zip(r, r[1:])) and r[0] < 0.02 and r[-1] == pytest.approx(0.8)
    for args in ((0, "cosine", 0.5, 10), (0, "linear", 1.5, 10), (0, "linear", 0.5, 0), (0, "sigmoid", 0.5, -1)):
        with pytest.raises(ValueError):
            objective.sched_rate(*args)


# ------------------------------------------------------------------------------------------------ the reference mix
def _case(T=7, N=6, V=37, seed=0):
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, 2, T, 4, T - 1][:N], np.int32)
    cap = np.zeros((T, N), np.int32)
    for n in range(N):
        cap[:lens[n], n] = np.concatenate([[1], rng.integers(3, V, size=T)])[:lens[n]]
    logits = (3 * rng.standard_normal((T * N, V))).astype(np.float32)
    return cap, lens, logits, rng.random((T, N), dtype=np.float32), rng.random((T, N), dtype=np.float32)


@pytest.mark.parametrize("argmax", [False, True])
def test_reference_mix_edges(argmax):
    cap, lens, logits, coin, u = _case()
    T, N = cap.shape
    uu = None if argmax else u
    out0, _ = R.mix(logits, cap, lens, coin, uu, 1.0, 0.0)
    np.testing.assert_array_equal(out0, cap)                       # rate 0: the input
    out1, cdfs = R.mix(logits, cap, lens, coin, uu, 1.0, 1.0)
    el = R.eligible(T, N, lens)
    assert el.sum() == sum(max(int(l) - 1, 0) for l in lens) and not el[0].any() and not el[:, lens == 0].any() and not el[:, lens == 1].any()
    np.testing.assert_array_equal(out1[~el], cap[~el])             # <BOS>, PAD positions, rows of length 0: never touched
    for t, n in zip(*np.nonzero(el)):                              # rate 1: every eligible position takes the model's word
        row = logits[(t - 1) * N + n].astype(np.float64)
        if argmax:
            assert out1[t, n] == np.argmax(row)
        else:
            c = cdfs[(t, n)]
            assert R.accepts(c, int(out1[t, n]), u[t, n]) and c[-1] == 1.0
            lo = c[out1[t, n] - 1] if out1[t, n] else 0.0
            assert lo <= u[t, n] < c[out1[t, n]]
    half, _ = R.mix(logits, cap, lens, coin, uu, 1.0, 0.5)
    sel = el & (coin < np.float32(0.5))
    np.testing.assert_array_equal(half[~sel], cap[~sel])
    np.testing.assert_array_equal(half[sel], out1[sel])
    # a coin exactly at the rate is not selected (strict comparison), a coin of 0 is selected at any positive rate
    t, n = [int(x[0]) for x in np.nonzero(el)]
    c2 = coin.copy()
    c2[t, n] = np.float32(0.25)
    assert R.mix(logits, cap, lens, c2, uu, 1.0, 0.25)[0][t, n] == cap[t, n]
    c2[t, n] = 0.0
    assert R.mix(logits, cap, lens, c2, uu, 1.0, 1e-6)[0][t, n] == out1[t, n]


def test_reference_draw_follows_the_distribution():
    """u = 0 draws the first word with any mass, u just below 1 the last one; a dominant logit takes every u; the temperature sharpens"""
    x = np.array([[0.0, 1.0, -2.0, 0.5]], np.float32)
    cap, lens, coin = np.array([[1], [5]], np.int32), np.array([2], np.int32), np.zeros((2, 1), np.float32)
    draw = lambda uv, temp=1.0, lg=x: int(R.mix(np.vstack([lg, lg]), cap, lens, coin, np.array([[0.0], [uv]], np.float32), temp, 1.0)[0][1, 0])
    assert draw(0.0) == 0 and draw(np.nextafter(np.float32(1), np.float32(0))) == 3
    p = np.exp(x[0].astype(np.float64)) / np.exp(x[0].astype(np.float64)).sum()
    assert draw(p[0] * 0.999) == 0 and draw(p[0] * 1.001) == 1
    dom = np.array([[0.0, 0.0, 60.0, 0.0]], np.float32)
    assert all(draw(uv, lg=dom) == 2 for uv in (1e-20, 0.5, 0.999999))
    assert draw(0.8, temp=2.0) == 3 and draw(0.8, temp=0.05) == 1   # cold: the mode


# ------------------------------------------------------------------------------------------------ the C-ABI entry (no device work)
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return abi.load()


def test_entry_is_declared_and_exported(built):
    protos = abi.parse_header()
    assert "vc_sched_mix_f32" in protos and hasattr(ctypes.CDLL(abi.LIB_PATH), "vc_sched_mix_f32")
    names = [a for _, a in protos["vc_sched_mix_f32"][1]]
    assert names == ["stream", "logits", "ld", "V", "T", "N", "cap_dec_t", "lens", "coin", "u", "temperature", "step", "schedule", "rate_max",
                     "ramp_steps", "dec_mix_t", "stats", "rate_out"]
    assert "vc_sched_mix_f32" in open(abi.HEADER).read().split("#define VC_ABI_VERSION")[0]   # the ABI history names it


def test_entry_argument_errors_come_before_any_device_work(built):
    X = 0x1000   # a non-NULL address that is never dereferenced: every call below fails validation
    good = dict(stream=None, logits=X, ld=8, V=8, T=3, N=2, cap=X, lens=X, coin=X, u=X, temp=1.0, step=X, schedule=1, rate_max=0.5, ramp=10, out=X,
                stats=None, rate_out=None)
    bad = [dict(V=0), dict(ld=7), dict(T=0), dict(N=0), dict(temp=0.0), dict(temp=-1.0), dict(rate_max=-0.01), dict(rate_max=1.01),
           dict(rate_max=float("nan")), dict(schedule=3), dict(schedule=-1), dict(schedule=1, ramp=0), dict(schedule=2, ramp=-3),
           dict(logits=None), dict(cap=None), dict(lens=None), dict(coin=None), dict(step=None), dict(out=None)]
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(abi.VaecapError, match="code 10001"):
            built.vc_sched_mix_f32(*a.values())
