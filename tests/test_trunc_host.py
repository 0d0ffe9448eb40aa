"""CPU: the host end of truncated sampling (top-k / nucleus; DESIGN.md "Truncated sampling"): the flags, the new C-ABI entry's argument
checks (which run before any device work), the generator's own argument errors, the numpy reference of tests/trunc_ref.py against
hand-made rows, and the safe-row cap of every input the GPU test (tests/test_gpu_trunc.py) decodes."""
import ctypes
import os
import types

import numpy as np
import pytest

from vae_captioning_amd import abi
from vae_captioning_amd.generate import CaptionGenerator
from vae_captioning_amd.utils.parameters import Parameters

from . import trunc_ref as tr


# ------------------------------------------------------------------ flags
def test_flags_default_to_off_and_parse():
    q = Parameters().parse_args([])
    assert q.top_k == 0 and isinstance(q.top_k, int) and q.top_p == 1.0 and isinstance(q.top_p, float)
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_method", "sample", "--top_k", "50", "--top_p", "0.9"])
    assert p.top_k == 50 and isinstance(p.top_k, int) and p.top_p == 0.9 and p.diverse_method == "sample"
    assert Parameters().parse_args(["--top_p", "1"]).top_p == 1.0 and Parameters().parse_args(["--top_k", "0"]).top_k == 0
    assert Parameters.top_k == 0 and Parameters.top_p == 1.0   # (class-level defaults: a pickled instance of an older run has them too)


@pytest.mark.parametrize("argv,flag", [(["--top_k", "-1"], "--top_k"), (["--top_p", "0"], "--top_p"), (["--top_p", "1.5"], "--top_p"),
                                       (["--top_p", "nan"], "--top_p"), (["--top_p", "-0.2"], "--top_p")],
                         ids=["k-negative", "p-zero", "p-over-1", "p-nan", "p-negative"])
def test_bad_flag_values_error_naming_the_flag(argv, flag, capsys):
    with pytest.raises(SystemExit):
        Parameters().parse_args(argv)
    assert flag + " must be" in capsys.readouterr().err


# ------------------------------------------------------------------ the C ABI: exported, and bad arguments refused before device work
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return abi.load()


def test_new_entry_is_declared_and_exported(built):
    protos = abi.parse_header()
    assert "vc_decode_pick_trunc_f32" in protos and hasattr(ctypes.CDLL(abi.LIB_PATH), "vc_decode_pick_trunc_f32")
    assert [t for t, _ in protos["vc_decode_pick_trunc_f32"][1]][5:8] == ["float", "int", "float"]   # temperature, top_k, top_p
    assert built.vc_abi_version() == 4


X = 4096   # a non-null pointer value: the checks must refuse the call before anything dereferences it
#        stream logits rows V  ld  temp top_k top_p u  u_rounds round eos tok done seq Lmax len logprob kept
GOOD = (None, X, 4, 40, 40, 1.0, 5, 0.9, X, 1, None, 2, X, X, X, 8, X, X, None)


def _with(**kw):
    names = ["stream", "logits", "rows", "V", "ld", "temperature", "top_k", "top_p", "u", "u_rounds", "round", "eos", "tok", "done", "seq",
             "Lmax", "len", "logprob", "kept"]
    a = list(GOOD)
    for k, v in kw.items():
        a[names.index(k)] = v
    return tuple(a)


@pytest.mark.parametrize("args", [
    _with(logits=None), _with(done=None), _with(logprob=None), _with(ld=39), _with(rows=0), _with(Lmax=0), _with(u=None), _with(u_rounds=0),
    _with(temperature=0.0), _with(temperature=-1.0), _with(temperature=float("nan")), _with(top_k=-1), _with(top_p=0.0), _with(top_p=-0.5),
    _with(top_p=1.0001), _with(top_p=float("nan")),
], ids=["null-logits", "null-done", "null-logprob", "ld", "no-rows", "lmax", "no-uniforms", "u-rounds", "temperature-0", "temperature-negative",
        "temperature-nan", "k-negative", "p-zero", "p-negative", "p-over-1", "p-nan"])
def test_entry_rejects_bad_arguments(built, args):
    with pytest.raises(abi.VaecapError, match="invalid argument"):
        built.vc_decode_pick_trunc_f32(*args)


# ------------------------------------------------------------------ the generator's argument errors, before any device work
def _gen():
    p = Parameters()
    p.gen_z_samples, p.latent_size = 4, 10
    return CaptionGenerator(types.SimpleNamespace(p=p, lib=None))


@pytest.mark.parametrize("kw", [dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                                dict(top_p=1.0 - 1e-12)],
                         ids=["k-negative", "k-fraction", "p-zero", "p-over-1", "p-nan", "p-is-1-in-f32"])
def test_generator_rejects_out_of_range_truncation(kw):
    f = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="top_k|top_p"):
        _gen().diverse(f, draws=3, method="sample", **kw)
    with pytest.raises(ValueError, match="top_k|top_p"):
        _gen().sample(f, **kw)


def test_diverse_rejects_truncation_of_a_greedy_decode():
    f = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="greedy"):
        _gen().diverse(f, draws=3, method="greedy", top_k=5)
    with pytest.raises(ValueError, match="greedy"):
        _gen().diverse(f, draws=3, top_p=0.9)


# ------------------------------------------------------------------ the reference
def test_reference_without_truncation_is_the_plain_inverse_cdf():
    rng = np.random.default_rng(3)
    R, V, temp = 64, 1003, 0.7
    logits = (rng.standard_normal((R, V)) * 2).astype(np.float32)
    u = rng.random(R).astype(np.float32)
    u[:3] = [0.0, 0.999999, 0.5]
    y = tr.scaled(logits, temp).astype(np.float64)
    pr = np.exp(y - y.max(1, keepdims=True))
    cdf = np.cumsum(pr, axis=1)
    ref = [min(V - 1, int(np.searchsorted(cdf[r], float(u[r]) * cdf[r, -1], side="right"))) for r in range(R)]
    for top_k in (0, V, V + 5):
        got = tr.trunc_rows(logits, temp, top_k, 1.0, u)
        assert [g["token"] for g in got] == ref and all(g["kept"] == V for g in got)


def test_reference_kept_set_is_monotone_in_k_and_p():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(300) * 4.0).astype(np.float32)
    x[:40] = np.round(x[:40])
    prev = set()
    for k in (1, 2, 5, 40, 299, 300):
        cur = set(tr.trunc_row(x, 0.8, k, 1.0, 0.5)["kept_set"].tolist())
        assert len(cur) == k and prev <= cur
        prev = cur
    prev = set()
    for p in (1e-6, 0.1, 0.5, 0.9, 0.99, 1.0):
        r = tr.trunc_row(x, 0.8, 0, p, 0.5)
        cur = set(r["kept_set"].tolist())
        assert prev <= cur and r["kept"] == len(cur) >= 1
        prev = cur
    assert len(prev) == 300
    for p in (0.3, 0.9):   # the nucleus lives inside the top-k set
        assert set(tr.trunc_row(x, 0.8, 7, p, 0.5)["kept_set"].tolist()) <= set(tr.trunc_row(x, 0.8, 7, 1.0, 0.5)["kept_set"].tolist())


def test_reference_ties_go_to_the_lower_index():
    x = np.array([1.0, 3.0, 3.0, 0.0, 3.0, 3.0, -0.0, 2.0], np.float32)
    assert tr.trunc_row(x, 1.0, 1, 1.0, 0.99)["kept_set"].tolist() == [1]
    assert tr.trunc_row(x, 1.0, 3, 1.0, 0.5)["kept_set"].tolist() == [1, 2, 4]
    assert tr.trunc_row(x, 1.0, 0, 1e-6, 0.99)["token"] == 1                        # one word kept: the first maximum, whatever u
    # four equal words hold 4 e^3 / (4 e^3 + e^2 + e + 2) = 0.86 of the mass: a share of 0.5 needs three of them, the first three
    r = tr.trunc_row(x, 1.0, 0, 0.5, 0.9)
    assert r["kept_set"].tolist() == [1, 2, 4] and r["token"] == 4 and r["safe"]
    # +0.0 and -0.0 are equal: the lower index first
    z = np.array([-5.0, -0.0, 0.0, -5.0], np.float32)
    assert tr.trunc_row(z, 1.0, 1, 1.0, 0.5)["kept_set"].tolist() == [1]
    # the draw walks the kept words in index order
    assert [tr.trunc_row(x, 1.0, 3, 1.0, u)["token"] for u in (0.0, 0.3, 0.4, 0.7, 0.999)] == [1, 1, 2, 4, 4]


def test_reference_marks_edge_rows_unsafe_and_single_words_safe():
    x = np.array([0.0, 1.0, 2.0, 3.0], np.float32)
    assert not tr.trunc_row(x, 1.0, 0, 1.0, 0.0)["safe"] and not tr.trunc_row(x, 1.0, 0, 1.0, 0.999999)["safe"]
    assert tr.trunc_row(x, 1.0, 1, 1.0, 0.0)["safe"] and tr.trunc_row(x, 1.0, 0, 1.0, 0.5)["safe"]
    e = np.full(40, 1.25, np.float32)   # 36 of 40 equal words hold exactly 0.9: the cut sits on top_p
    r = tr.trunc_row(e, 1.0, 0, 0.9, 0.5)
    assert not r["safe"] and r["kept"] in (36, 37) and len(r["wide_set"]) == r["kept"] + 1


# ------------------------------------------------------------------ the GPU test's inputs
@pytest.mark.parametrize("shape_i", range(len(tr.SHAPES)), ids=["v%d" % v for v, _ in tr.SHAPES])
@pytest.mark.parametrize("setting_i", range(len(tr.SETTINGS)), ids=["k%d-p%g-t%g" % s for s in tr.SETTINGS])
def test_gpu_inputs_stay_within_the_unsafe_row_cap(shape_i, setting_i):
    x, V, ld, top_k, top_p, t, u = tr.make_case(shape_i, setting_i)
    assert x.shape == (tr.ROWS, ld) and (x[:, V:] == tr.PAD).all() and u[9] == 0.0 and u[11] == np.float32(0.999999)
    ref = tr.trunc_rows(x[:, :V], t, top_k, top_p, u)
    unsafe = [r for r in range(tr.ROWS) if not ref[r]["safe"]]
    print("V %d top_k %d top_p %g t %g: unsafe rows %s" % (V, top_k, top_p, t, unsafe))
    assert len(unsafe) <= tr.MAX_UNSAFE * tr.ROWS
    assert ref[5]["kept"] == 1 or top_p == 1.0           # the raised logit takes the nucleus alone
    assert len(np.unique(x[3, :V])) < V or V == 7        # the rounded row has exact ties
