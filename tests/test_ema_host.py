"""CPU: weight averaging -- the float64 reference against a hand-worked example, the argument checks of the four new entries (they come
before any launch, so they need no GPU: the pointers below are never dereferenced) and the parse errors of --ema_decay / --use_ema."""
from fractions import Fraction

import numpy as np
import pytest

from vae_captioning_amd import abi
from vae_captioning_amd.engine import EMA_SUFFIX, ema_omd, split_averages
from vae_captioning_amd.utils.parameters import Parameters

from . import ema_ref as R

A, B, C, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # 16-byte aligned addresses, 64 KiB apart: never dereferenced
LR = 0x60000


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_on_a_hand_worked_example():
    # decay 0.5, p = 1 throughout, e0 = 0, warm-up: w = 9/11, 9/12, 9/13 (each above 0.5)
    e1 = Fraction(9, 11)
    e2 = e1 + Fraction(3, 4) * (1 - e1)
    e3 = e2 + Fraction(9, 13) * (1 - e2)
    assert (e2, e3) == (Fraction(21, 22), Fraction(141, 143))
    e, M = R.ema_steps(np.zeros(2), [np.ones(2, np.float32)] * 3, 0.5)
    assert np.abs(e - float(e3)).max() <= 3 * 2.0 ** -24       # (the weights are float32)
    assert (M == 1).all()
    # constant decay: exact in binary
    e, M = R.ema_steps(np.zeros(1), [np.float32([2]), np.float32([4]), np.float32([8])], 0.5, warmup=False)
    assert e[0] == 5.25 and M[0] == 8
    # a later first step: w = max(0.5, 9/18), max(0.5, 9/19) -- both sides of the max
    assert R.weight(0.5, 7) == np.float32(9) / np.float32(17) and R.weight(0.5, 8) == np.float32(0.5) and R.weight(0.5, 9) == np.float32(0.5)
    assert R.weight(0.001, 12) == np.float32(9) / np.float32(22) and R.weight(0.25) == np.float32(0.25)
    assert R.bound(np.float64(2), 12) == 3 * 12 * 2.0 ** -24 * 2


def test_one_minus_decay_is_taken_in_double():
    decay, omd = ema_omd(0.9999)
    assert decay == 0.9999 and omd == 1.0 - 0.9999
    good, bad = np.float32(omd), np.float32(1) - np.float32(0.9999)
    assert abs(float(good) - 1e-4) <= 2.0 ** -24 * 1e-4 and abs(float(bad) - 1e-4) > 1e-4 * 1e-4   # what the kernels would get otherwise
    assert ema_omd(0) == (0.0, 1.0)
    for v in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            ema_omd(v)
    d = {"a/b": 1, "a/b" + EMA_SUFFIX: 2, "cnn/fc1/weights" + EMA_SUFFIX: 3}
    assert split_averages(d) == {"a/b": 2, "cnn/fc1/weights": 3} and EMA_SUFFIX == "/ExponentialMovingAverage"


# ------------------------------------------------------------------------------------------------ argument checks (no launch)
def _adam(lib, sumsq=False, **kw):
    a = dict(p=A, g=B, m=C, v=D, ema=E, n=1024, lr=LR, omd=0.5, step=None, part=LR + 64)
    a.update(kw)
    args = (None, a["p"], a["g"], a["m"], a["v"], a["ema"], a["n"], a["lr"], None, 0.8, 0.999, 1e-8, 0.0, a["omd"], a["step"])
    if sumsq:
        return lib.vc_adam_sumsq_ema_f32(*args, a["part"])
    return lib.vc_adam_ema_f32(*args)


@pytest.mark.parametrize("sumsq", [False, True], ids=["adam_ema", "adam_sumsq_ema"])
def test_fused_entries_check_their_arguments(lib, sumsq):
    name = "vc_adam_sumsq_ema_f32" if sumsq else "vc_adam_ema_f32"
    for ptr in ("p", "g", "m", "v", "ema", "lr"):
        with pytest.raises(abi.VaecapError, match=name + ".*null pointer"):
            _adam(lib, sumsq, **{ptr: None})
    for ptr in ("p", "g", "m", "v", "ema"):
        with pytest.raises(abi.VaecapError, match=name + ".*16-byte aligned"):
            _adam(lib, sumsq, **{ptr: A + 4 + 0x100000})
    with pytest.raises(abi.VaecapError, match=name + ".*null pointer or n"):
        _adam(lib, sumsq, n=-1)
    for omd in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(abi.VaecapError, match=name + ".*omd = 1 - decay must be in \\(0, 1\\]"):
            _adam(lib, sumsq, omd=omd)
    for other in (A, C, D):   # ema on p, m, v: the same base, and a range that overlaps by one float4
        with pytest.raises(abi.VaecapError, match=name + ".*ema must not alias p, m or v"):
            _adam(lib, sumsq, ema=other)
        with pytest.raises(abi.VaecapError, match=name + ".*ema must not alias p, m or v"):
            _adam(lib, sumsq, ema=other + 4 * 1020)
        with pytest.raises(abi.VaecapError, match=name + ".*ema must not alias p, m or v"):
            _adam(lib, sumsq, ema=other - 4 * 1020)
    if sumsq:
        with pytest.raises(abi.VaecapError, match=name + ".*null pointer or n <= 0"):
            _adam(lib, sumsq, part=None)
        with pytest.raises(abi.VaecapError, match=name + ".*null pointer or n <= 0"):   # like vc_adam_sumsq_f32: someone must write the sums
            _adam(lib, sumsq, n=0)
    else:
        assert _adam(lib, n=0) == 0 and _adam(lib, n=0, omd=1.0) == 0   # a successful no-op; omd = 1 (decay 0) is legal


def test_ema_update_checks_its_arguments(lib):
    call = lambda ema=E, p=A, n=1024, omd=0.5, step=None: lib.vc_ema_update_f32(None, ema, p, n, omd, step)
    for kw in (dict(ema=None), dict(p=None), dict(n=-1)):
        with pytest.raises(abi.VaecapError, match="vc_ema_update_f32.*null pointer or n < 0"):
            call(**kw)
    for kw in (dict(ema=E + 8), dict(p=A + 4)):
        with pytest.raises(abi.VaecapError, match="vc_ema_update_f32.*16-byte aligned"):
            call(**kw)
    for omd in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(abi.VaecapError, match="vc_ema_update_f32.*omd = 1 - decay"):
            call(omd=omd)
    for ema in (A, A + 4 * 1020, A - 4 * 1020):
        with pytest.raises(abi.VaecapError, match="vc_ema_update_f32.*ema must not alias p"):
            call(ema=ema)
    assert call(n=0) == 0 and call(ema=A + 4 * 1024, n=0) == 0


def test_swap_checks_its_arguments(lib):
    call = lambda a=A, b=B, n=1024: lib.vc_swap_f32(None, a, b, n)
    for kw in (dict(a=None), dict(b=None), dict(n=-1)):
        with pytest.raises(abi.VaecapError, match="vc_swap_f32.*null pointer or n < 0"):
            call(**kw)
    for kw in (dict(a=A + 4), dict(b=B + 8)):
        with pytest.raises(abi.VaecapError, match="vc_swap_f32.*16-byte aligned"):
            call(**kw)
    for b in (A, A + 4 * 1020, A - 4 * 1020):
        with pytest.raises(abi.VaecapError, match="vc_swap_f32.*a must not alias b"):
            call(b=b)
    assert call(n=0) == 0


def test_header_binds_the_new_prototypes(lib):
    protos = abi.parse_header()
    assert [t for t, _ in protos["vc_adam_ema_f32"][1]][-2:] == ["float", "const int32_t*"]
    assert [a for _, a in protos["vc_adam_sumsq_ema_f32"][1]][-3:] == ["omd", "step", "sumsq_partial"]
    assert [a for _, a in protos["vc_ema_update_f32"][1]] == ["stream", "ema", "p", "n", "omd", "step"]
    assert [a for _, a in protos["vc_swap_f32"][1]] == ["stream", "a", "b", "n"]
    assert lib.vc_abi_version() == 4   # additive: no bump


# ------------------------------------------------------------------------------------------------ command line
def _parse(argv):
    return Parameters().parse_args(["--synthetic"] + argv)


def test_flags_parse():
    p = _parse([])
    assert p.ema_decay == 0.0 and p.use_ema is False and Parameters.ema_decay == 0.0
    p = _parse(["--ema_decay", "0.999"])
    assert p.ema_decay == 0.999 and p.use_ema is False
    assert _parse(["--ema_decay", "0.99", "--fine_tune", "--restore"]).ema_decay == 0.99
    p = _parse(["--mode", "inference", "--use_ema"])
    assert p.use_ema is True and p.ema_decay == 0.0
    assert _parse(["--ema_decay", "0"]).ema_decay == 0.0


@pytest.mark.parametrize("argv, message", [
    (["--ema_decay", "1"], "--ema_decay must be in \\[0, 1\\)"),
    (["--ema_decay", "1.5"], "--ema_decay must be in \\[0, 1\\)"),
    (["--ema_decay", "-0.1"], "--ema_decay must be in \\[0, 1\\)"),
    (["--ema_decay", "nan"], "--ema_decay must be in \\[0, 1\\)"),
    (["--ema_decay", "0.9", "--mode", "inference"], "--ema_decay averages the weights of a training run: not with --mode inference"),
    (["--ema_decay", "0.9", "--scst"], "--ema_decay does not go with --scst"),
    (["--use_ema"], "--use_ema needs --mode inference"),
    (["--use_ema", "--ema_decay", "0.9"], "--use_ema needs --mode inference"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_parse_errors(capsys, argv, message):
    import re
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2
    assert re.search(message, capsys.readouterr().err)
