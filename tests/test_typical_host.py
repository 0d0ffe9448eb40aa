"""CPU: the host end of typical / min-p / eta sampling (DESIGN.md "Typical / min-p / eta sampling"): the flags, the new C-ABI entry's
prototype and its argument checks (which run before any device work), the validator and the generator's argument errors, the numpy
reference of tests/typical_ref.py against hand-computed rows, and the safe-row cap of every input the GPU test
(tests/test_gpu_typical.py) decodes."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from vae_captioning_amd import abi
from vae_captioning_amd.decode_host import check_typical
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.ops.inference import EVAL_FLAGS
from vae_captioning_amd.utils.parameters import Parameters

from . import typical_ref as ty

SAMPLE = ["--sample_gen", "diverse", "--diverse_method", "sample"]


# ------------------------------------------------------------------ flags
def test_flags_default_to_off_and_parse():
    q = Parameters().parse_args([])
    assert (q.typical_p, q.min_p, q.eta) == (1.0, 0.0, 0.0) and all(isinstance(v, float) for v in (q.typical_p, q.min_p, q.eta))
    p = Parameters().parse_args(SAMPLE + ["--typical_p", "0.9", "--min_p", "0.02", "--eta_cutoff", "1e-3"])
    assert (p.typical_p, p.min_p, p.eta) == (0.9, 0.02, 1e-3)
    assert Parameters().parse_args(["--sample_gen", "sample", "--min_p", "1"]).min_p == 1.0
    assert (Parameters.typical_p, Parameters.min_p, Parameters.eta) == (1.0, 0.0, 0.0)   # (class-level: a pickled older instance has them)
    assert {"typical_p", "min_p", "eta"} <= set(EVAL_FLAGS)


@pytest.mark.parametrize("argv,text", [
    (["--typical_p", "0"], "--typical_p must be"), (["--typical_p", "1.2"], "--typical_p must be"), (["--typical_p", "nan"], "--typical_p must be"),
    (["--min_p", "-0.1"], "--min_p must be"), (["--min_p", "1.5"], "--min_p must be"), (["--min_p", "nan"], "--min_p must be"),
    (["--eta_cutoff", "1"], "--eta_cutoff must be"), (["--eta_cutoff=-1e-3"], "--eta_cutoff must be"),
    (["--sample_gen", "diverse", "--diverse_method", "greedy", "--typical_p", "0.9"], "--diverse_method greedy"),
    (["--sample_gen", "diverse", "--min_p", "0.1"], "--diverse_method greedy"),
    (SAMPLE + ["--typical_p", "0.9", "--top_k", "40"], "--top_k / --top_p"), (SAMPLE + ["--eta_cutoff", "1e-3", "--top_p", "0.9"], "--top_k / --top_p"),
    (["--scst", "--min_p", "0.1"], "--scst"), (["--scst", "--typical_p", "0.5"], "--scst"),
], ids=["tau-zero", "tau-over-1", "tau-nan", "m-negative", "m-over-1", "m-nan", "eta-one", "eta-negative", "greedy", "greedy-by-default", "with-top-k",
        "with-top-p", "scst-min-p", "scst-typical"])
def test_bad_flag_combinations_error(argv, text, capsys):
    with pytest.raises(SystemExit):
        Parameters().parse_args(argv)
    assert text in capsys.readouterr().err


# ------------------------------------------------------------------ the validator and the generator's argument errors
def test_validator_returns_floats_and_accepts_the_edges():
    assert check_typical(1, 0, 0) == (1.0, 0.0, 0.0) and all(isinstance(v, float) for v in check_typical(1, 0, 0))
    assert check_typical(0.9, 1, 0.5) == (0.9, 1.0, 0.5)
    assert check_typical(1.0, 0.0, 0.0, "greedy", 5, 0.9) == (1.0, 0.0, 0.0)     # nothing asked: nothing to refuse


@pytest.mark.parametrize("args,text", [
    ((0.0, 0, 0), "typical_p"), ((1.5, 0, 0), "typical_p"), ((float("nan"), 0, 0), "typical_p"), ((1.0 - 1e-12, 0, 0), "float32"),
    ((1, -0.1, 0), "min_p"), ((1, 1.1, 0), "min_p"), ((1, float("nan"), 0), "min_p"), ((1, 0, 1.0), "eta"), ((1, 0, -1e-3), "eta"),
    ((1, 0, float("nan")), "eta"), ((0.9, 0, 0, "greedy"), "greedy"), ((1, 0.1, 0, "greedy"), "greedy"), ((1, 0, 1e-3, "greedy"), "greedy"),
    ((0.9, 0, 0, "sample", 5, 1.0), "top_k / top_p"), ((1, 0.1, 0, "sample", 0, 0.9), "top_k / top_p"),
], ids=["tau-zero", "tau-over-1", "tau-nan", "tau-is-1-in-f32", "m-negative", "m-over-1", "m-nan", "eta-one", "eta-negative", "eta-nan",
        "greedy-tau", "greedy-m", "greedy-eta", "with-top-k", "with-top-p"])
def test_validator_errors(args, text):
    with pytest.raises(ValueError, match=text):
        check_typical(*args)


def _gen():
    p = Parameters()
    p.gen_z_samples, p.latent_size = 4, 10
    return CaptionGenerator(types.SimpleNamespace(p=p, lib=None))


@pytest.mark.parametrize("kw", [dict(typical_p=0.0), dict(min_p=2.0), dict(eta=1.0), dict(typical_p=0.9, top_k=5), dict(min_p=0.1, top_p=0.9)],
                         ids=["tau-zero", "m-over-1", "eta-one", "with-top-k", "with-top-p"])
def test_generator_rejects_bad_cuts_before_any_device_work(kw):
    f = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="typical_p|min_p|eta"):
        _gen().diverse(f, draws=3, method="sample", **kw)
    with pytest.raises(ValueError, match="typical_p|min_p|eta"):
        _gen().sample(f, **kw)


def test_diverse_rejects_cuts_of_a_greedy_decode():
    f = np.zeros((2, 8), np.float32)
    for kw in (dict(typical_p=0.9), dict(min_p=0.1), dict(eta=1e-3)):
        with pytest.raises(ValueError, match="greedy"):
            _gen().diverse(f, draws=3, **kw)


# ------------------------------------------------------------------ the C ABI: declared, exported, and bad arguments refused before device work
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return abi.load()


def test_new_entry_is_declared_and_exported(built):
    protos = abi.parse_header()
    assert "vc_decode_pick_typical_f32" in protos and hasattr(ctypes.CDLL(abi.LIB_PATH), "vc_decode_pick_typical_f32")
    args = protos["vc_decode_pick_typical_f32"][1]
    trunc = protos["vc_decode_pick_trunc_f32"][1]
    assert [t for t, _ in args][5:9] == ["float", "float", "float", "float"]   # temperature, typical_p, min_p, eta
    assert [n for _, n in args][6:9] == ["typical_p", "min_p", "eta"]
    assert args[:6] == trunc[:6] and args[9:-1] == trunc[8:]                    # the truncated pick's arguments around them ...
    assert args[-2][1] == "kept" and args[-1][1] == "entropy" and "float" in args[-1][0] and "*" in args[-1][0]   # ... and entropy behind kept
    assert built.vc_abi_version() == 4


X = 4096   # a non-null pointer value: the checks must refuse the call before anything dereferences it
NAMES = ["stream", "logits", "rows", "V", "ld", "temperature", "typical_p", "min_p", "eta", "u", "u_rounds", "round", "eos", "tok", "done", "seq",
         "Lmax", "len", "logprob", "kept", "entropy"]
GOOD = (None, X, 4, 40, 40, 1.0, 0.9, 0.05, 1e-3, X, 1, None, 2, X, X, X, 8, X, X, None, None)


def _with(**kw):
    a = list(GOOD)
    for k, v in kw.items():
        a[NAMES.index(k)] = v
    return tuple(a)


@pytest.mark.parametrize("args", [
    _with(logits=None), _with(tok=None), _with(done=None), _with(seq=None), _with(len=None), _with(logprob=None), _with(ld=39), _with(rows=0),
    _with(Lmax=0), _with(u=None), _with(u_rounds=0), _with(temperature=0.0), _with(temperature=-1.0), _with(temperature=float("nan")),
    _with(temperature=float("inf")), _with(typical_p=0.0), _with(typical_p=-0.5), _with(typical_p=1.0001), _with(typical_p=float("nan")),
    _with(min_p=-0.01), _with(min_p=1.0001), _with(min_p=float("nan")), _with(eta=-1e-3), _with(eta=1.0), _with(eta=float("nan")),
    _with(typical_p=1.0, min_p=0.0, eta=0.0, u=None),
], ids=["null-logits", "null-tok", "null-done", "null-seq", "null-len", "null-logprob", "ld", "no-rows", "lmax", "no-uniforms", "u-rounds",
        "temperature-0", "temperature-negative", "temperature-nan", "temperature-inf", "tau-zero", "tau-negative", "tau-over-1", "tau-nan",
        "m-negative", "m-over-1", "m-nan", "eta-negative", "eta-one", "eta-nan", "all-off-no-uniforms"])
def test_entry_rejects_bad_arguments(built, args):
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_decode_pick_typical_f32(*args)


# ------------------------------------------------------------------ the reference on hand-computed rows
def test_reference_entropy_and_typical_order_by_hand():
    # p = (1/2, 1/4, 1/8, 1/8): H = 1.75 ln 2; surprisals (1, 2, 3, 3) ln 2: d = (0.75, 0.25, 1.25, 1.25) ln 2 -> order 1, 0, 2, 3
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    r = ty.typical_row(x, 1.0, 0.2, 0, 0, 0.5)
    assert abs(r["H"] - 1.75 * math.log(2)) < 1e-7
    assert r["kept_set"].tolist() == [1] and r["token"] == 1 and r["safe"]
    assert ty.typical_row(x, 1.0, 0.5, 0, 0, 0.1)["kept_set"].tolist() == [0, 1]        # 1/4 < 0.5 <= 3/4
    r = ty.typical_row(x, 1.0, 0.8, 0, 0, 0.99)                                         # 3/4 < 0.8 <= 7/8: the tie at d = 1.25 ln 2 by lower index
    assert r["kept_set"].tolist() == [0, 1, 2] and r["token"] == 2 and r["kept"] == 3
    assert ty.typical_row(x, 1.0, 1.0, 0, 0, 0.5)["kept"] == 4
    # the draw walks the kept words in index order: kept masses (1/2, 1/4) -> u < 2/3: word 0
    assert [ty.typical_row(x, 1.0, 0.5, 0, 0, u)["token"] for u in (0.0, 0.6, 0.7, 0.999)] == [0, 0, 1, 1]


def test_reference_floors_by_hand():
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    assert ty.typical_row(x, 1.0, 1.0, 0.3, 0, 0.5)["kept_set"].tolist() == [0, 1]      # floor 0.15
    assert ty.typical_row(x, 1.0, 1.0, 0.2, 0, 0.5)["kept_set"].tolist() == [0, 1, 2, 3]   # floor 0.1
    assert ty.typical_row(x, 1.0, 1.0, 1.0, 0, 0.99)["kept_set"].tolist() == [0]        # min_p = 1: the maximum
    t3 = np.array([2.0, 5.0, 5.0, 1.0, 5.0], np.float32)
    assert ty.typical_row(t3, 1.0, 1.0, 1.0, 0, 0.5)["kept_set"].tolist() == [1, 2, 4]  # ... every maximum of y
    # eta: H = 1.75 ln 2, exp(-H) = 2^-1.75 = 0.2973; eta = 0.25: min(0.25, 0.5 * 0.2973 = 0.1487) -> the 1/8 words go
    assert ty.typical_row(x, 1.0, 1.0, 0, 0.25, 0.5)["kept_set"].tolist() == [0, 1]
    assert ty.typical_row(x, 1.0, 1.0, 0, 0.01, 0.5)["kept"] == 4                       # min(0.01, 0.1 * 0.2973): all stay
    # the larger floor rules: min_p 0.6 (floor 0.3) over eta 0.25 (floor 0.1487)
    assert ty.typical_row(x, 1.0, 1.0, 0.6, 0.25, 0.5)["kept_set"].tolist() == [0]


def test_reference_intersection_on_the_full_distribution_and_the_empty_case():
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    # typical 0.2 keeps {1}; min_p 0.6 keeps {0}: empty -> the first maximum of y, one word, whatever u
    for u in (0.0, 0.5, 0.999999):
        r = ty.typical_row(x, 1.0, 0.2, 0.6, 0, u)
        assert r["kept_set"].tolist() == [0] and r["token"] == 0 and r["kept"] == 1 and r["safe"]
    # typical 0.8 keeps {0, 1, 2} of the FULL distribution, the floor 0.15 {0, 1}: no cut renormalises for the next
    assert ty.typical_row(x, 1.0, 0.8, 0.3, 0, 0.5)["kept_set"].tolist() == [0, 1]
    t3 = np.array([2.0, 5.0, 5.0, 1.0, 5.0], np.float32)
    assert ty.typical_row(t3, 1.0, 1e-6, 1.0, 0, 0.99)["kept_set"].tolist() == [1]      # a tie at the top: the first maximum


def test_reference_zero_mass_words_add_nothing_and_are_never_kept():
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    xb = np.concatenate([x, np.full(3, -ty.FLT_MAX, np.float32)])
    for t in (1.0, 0.7):   # 0.7 scales -FLT_MAX to -inf
        a, b = ty.typical_row(x, t, 0.8, 0, 0, 0.99), ty.typical_row(xb, t, 0.8, 0, 0, 0.99)
        assert math.isfinite(b["H"]) and abs(a["H"] - b["H"]) < 1e-12
        assert a["kept_set"].tolist() == b["kept_set"].tolist() and a["token"] == b["token"]
        assert ty.typical_row(xb, t, 1.0, 0, 1e-3, 0.99)["kept"] == 4 and ty.typical_row(xb, t, 1.0, 0, 1e-3, 0.999999)["token"] == 3


def test_reference_all_cuts_off_is_the_plain_inverse_cdf():
    rng = np.random.default_rng(3)
    R, V, temp = 32, 1003, 0.7
    logits = (rng.standard_normal((R, V)) * 2).astype(np.float32)
    u = rng.random(R).astype(np.float32)
    u[:3] = [0.0, 0.999999, 0.5]
    y = ty.scaled(logits, temp).astype(np.float64)
    cdf = np.cumsum(np.exp(y - y.max(1, keepdims=True)), axis=1)
    ref = [min(V - 1, int(np.searchsorted(cdf[r], float(u[r]) * cdf[r, -1], side="right"))) for r in range(R)]
    got = ty.typical_rows(logits, temp, 1.0, 0.0, 0.0, u)
    assert [g["token"] for g in got] == ref and all(g["kept"] == V for g in got)


def test_reference_marks_edge_and_margin_rows_unsafe():
    x = np.log(np.array([0.5, 0.25, 0.125, 0.125])).astype(np.float32)
    assert not ty.typical_row(x, 1.0, 1.0, 0, 0, 0.0)["safe"] and not ty.typical_row(x, 1.0, 1.0, 0, 0, 0.999999)["safe"]
    assert ty.typical_row(x, 1.0, 0.2, 0, 0, 0.0)["safe"]                               # one word kept
    r = ty.typical_row(x, 1.0, 0.75, 0, 0, 0.3)                                         # the cut sits on tau
    assert not r["safe"] and r["kept"] in (2, 3) and set(r["wide_set"].tolist()) >= {0, 1, 2}
    r = ty.typical_row(x, 1.0, 1.0, 0.25, 0, 0.3)                                       # p = 1/8 sits on the floor 0.25 * 1/2
    assert not r["safe"] and r["kept"] in (2, 3, 4) and r["wide_set"].tolist() == [0, 1, 2, 3]
    e = np.full(40, 1.25, np.float32)   # all d equal: the cut is by index, and 36 of 40 words hold exactly 0.9
    r = ty.typical_row(e, 1.0, 0.9, 0, 0, 0.5)
    assert not r["safe"] and r["kept"] in (36, 37) and r["kept_set"].tolist() == list(range(r["kept"]))


# ------------------------------------------------------------------ the GPU test's inputs
@pytest.mark.parametrize("shape_i", range(len(ty.SHAPES)), ids=["v%d" % v for v, _ in ty.SHAPES])
@pytest.mark.parametrize("setting_i", range(len(ty.SETTINGS)), ids=ty.SETTING_IDS)
def test_gpu_inputs_stay_within_the_unsafe_row_cap(shape_i, setting_i):
    x, V, ld, tau, min_p, eta, t, u = ty.make_case(shape_i, setting_i)
    assert x.shape == (ty.ROWS, ld) and (x[:, V:] == ty.PAD).all() and u[9] == 0.0 and u[11] == np.float32(0.999999)
    assert (x[ty.BANNED_ROW, :V] == -ty.FLT_MAX).sum() == min(ty.BANNED, V // 2)
    ref = ty.typical_rows(x[:, :V], t, tau, min_p, eta, u)
    unsafe = [r for r in range(ty.ROWS) if not ref[r]["safe"]]
    print("V %d tau %g min_p %g eta %g t %g: unsafe rows %s" % (V, tau, min_p, eta, t, unsafe))
    assert len(unsafe) <= ty.MAX_UNSAFE * ty.ROWS
    assert all(math.isfinite(q["H"]) and q["H"] >= 0 for q in ref)
    assert ref[5]["kept"] == 1 and ref[5]["H"] < 1e-6      # the raised logit holds all the mass
    assert len(np.unique(x[3, :V])) < V or V == 7          # the rounded row has exact ties
    assert abs(ref[7]["H"] - math.log(V)) < 1e-9           # all-equal logits
    assert not set(np.nonzero(x[ty.BANNED_ROW, :V] == -ty.FLT_MAX)[0].tolist()) & set(ref[ty.BANNED_ROW]["wide_set"].tolist())
