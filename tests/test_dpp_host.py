"""CPU: the DPP selection's reference (tests/dpp_ref.py) against an independent brute force over determinants, its structural
properties, mbr.dpp_quality's normalisation and the parse rules of --diverse_select / --select_n / --dpp_quality.  (The kernel against
the reference: tests/test_gpu_dpp.py.)"""
import itertools

import numpy as np
import pytest

from vae_captioning_amd import mbr
from vae_captioning_amd.utils.parameters import Parameters

from . import dpp_ref as ref


def _psd_gram(rng, m, dim):
    """G with (G + G^T) / 20 = X X^T for unit rows X with non-negative entries: S is positive semidefinite with entries in [0, 1]"""
    X = np.abs(rng.standard_normal((m, dim)))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return 10.0 * (X @ X.T)


def _logdet(L, Y):
    sign, val = np.linalg.slogdet(L[np.ix_(Y, Y)])
    return val if sign > 0 else -np.inf


@pytest.mark.parametrize("m,seed", list(itertools.product((1, 2, 3, 5, 8), (0, 1, 2))))
def test_every_greedy_step_maximises_the_determinant(m, seed):
    """brute force, independent of the incremental update: at every step the pick maximises slogdet(L[Y + {i}]) over the untaken i, and
    gain = det(L[Y + {j}]) / det(L[Y]) to 1e-10 (relative)"""
    rng = np.random.default_rng(100 * m + seed)
    G = _psd_gram(rng, m, m + 3)
    q = np.exp(rng.random(m) * 2.0)
    L = ref.kernel_matrix(G, q)
    sel, gain, n_dpp = ref.select(G, q, m)
    assert n_dpp == m and sorted(sel.tolist()) == list(range(m))          # full rank: every caption is chosen by gain
    Y = []
    for k in range(m):
        rest = [i for i in range(m) if i not in Y]
        vals = {i: _logdet(L, Y + [i]) for i in rest}
        best = max(vals.values())
        j = int(sel[k])
        assert vals[j] >= best - 1e-10, (k, j, vals)
        base = _logdet(L, Y) if Y else 0.0
        assert abs(gain[k] - np.exp(vals[j] - base)) <= 1e-10 * gain[k], (k, gain[k], np.exp(vals[j] - base))
        Y.append(j)
    assert (np.diff(gain[:n_dpp]) <= 1e-12 * gain[0]).all()               # a PSD kernel: the gains do not rise
    # a shorter selection is a prefix; slots past min(n, m) hold -1 / 0
    s2, g2, n2 = ref.select(G, q, min(2, m))
    assert np.array_equal(s2, sel[:len(s2)]) and np.array_equal(g2, gain[:len(g2)]) and n2 == len(s2)
    s3, g3, n3 = ref.select(G, q, m + 3)
    assert np.array_equal(s3[:m], sel) and (s3[m:] == -1).all() and (g3[m:] == 0).all() and n3 == m


def test_the_identity_picks_by_descending_quality():
    q = np.array([1.5, 3.0, 0.5, 3.0, 2.0])
    G = 10.0 * np.eye(5)
    sel, gain, n_dpp = ref.select(G, q, 5)
    assert sel.tolist() == [1, 3, 4, 0, 2] and n_dpp == 5                  # equal qualities: the lower index first
    assert np.array_equal(gain, (q * q)[sel])
    # the diagonal is set, not read: a zero self-score (an empty caption) changes nothing
    sel0, gain0, _ = ref.select(np.zeros((5, 5)), q, 5)
    assert np.array_equal(sel0, sel) and np.array_equal(gain0, gain)


def test_duplicates_are_never_chosen_by_gain_and_fill_in_index_order():
    rng = np.random.default_rng(5)
    G = _psd_gram(rng, 4, 6)
    idx = [0, 1, 1, 2, 0, 3, 1]                                           # captions 2 and 6 repeat 1, caption 4 repeats 0
    Gd = G[np.ix_(idx, idx)]
    q = np.ones(len(idx))
    sel, gain, n_dpp = ref.select(Gd, q, 7)
    assert n_dpp == 4 and sorted(idx[j] for j in sel[:4]) == [0, 1, 2, 3]  # one of each, chosen by gain ...
    assert set(sel[:4].tolist()) == {0, 1, 3, 5}                          # ... the first copy of each (ties go to the lower index)
    assert sel[4:].tolist() == [2, 4, 6] and (gain[4:] == 0).all() and (gain[:4] > 0).all()
    sel5, gain5, n5 = ref.select(Gd, q, 5)
    assert n5 == 4 and sel5.tolist() == sel[:4].tolist() + [2] and gain5[4] == 0
    # replay of the same picks agrees, reports nothing live at the end, and every leftover ratio is a rounding of zero
    steps, tail = ref.replay(Gd, q, 7, sel[:4])
    assert not tail["more"] and np.array_equal(tail["sel"], sel) and np.array_equal(tail["gain"], gain) and tail["n_dpp"] == 4
    assert (np.abs(tail["ratios"]) < 1e-12).all()
    assert all(st["live"][j] and st["d"][j] == st["d"][st["live"]].max() for st, j in zip(steps, sel[:4]))


@pytest.mark.parametrize("seed", range(4))
def test_the_first_pick_is_the_best_quality(seed):
    rng = np.random.default_rng(seed)
    m = 12
    G = rng.random((m, m)) * 10.0                                         # not symmetric, not PSD: the procedure is defined anyway
    q = np.exp(rng.random(m) * 3.0)
    sel, gain, n_dpp = ref.select(G, q, 6)
    assert sel[0] == int(np.argmax(q)) and gain[0] == q.max() ** 2
    assert len(set(sel.tolist())) == 6 and (sel >= 0).all() and 1 <= n_dpp <= 6
    assert (gain[:n_dpp] > 0).all() and (gain[n_dpp:] == 0).all()


def test_an_empty_image_and_a_single_caption():
    sel, gain, n_dpp = ref.select(np.zeros((0, 0)), np.zeros(0), 3)
    assert sel.tolist() == [-1, -1, -1] and gain.tolist() == [0, 0, 0] and n_dpp == 0
    sel, gain, n_dpp = ref.select(np.zeros((1, 1)), np.array([2.0]), 3)
    assert sel.tolist() == [0, -1, -1] and gain.tolist() == [4.0, 0, 0] and n_dpp == 1


# ------------------------------------------------------------------ the qualities
def test_quality_normalisation():
    q = mbr.dpp_quality([-3.0, -1.0, -2.0], 2.0)
    assert q.dtype == np.float64 and np.array_equal(q, np.exp(2.0 * np.array([0.0, 1.0, 0.5])))
    assert np.array_equal(mbr.dpp_quality([0.7, 0.7, 0.7], 5.0), np.ones(3))                   # all keys equal: r = 0
    q = mbr.dpp_quality([1.0, -np.inf, 3.0, np.nan], 1.0)                                      # a non-finite key: r = 0, and it does not
    assert np.array_equal(q, np.exp(np.array([0.0, 0.0, 1.0, 0.0])))                           # enter the minimum
    assert np.array_equal(mbr.dpp_quality([-np.inf, -np.inf], 4.0), np.ones(2))
    assert np.array_equal(mbr.dpp_quality([5.0, 1.0, 2.0], 0.0), np.ones(3))                   # W = 0: diversity alone
    assert mbr.dpp_quality([], 1.0).shape == (0,)
    assert mbr.dpp_quality([1.0, 2.0], 8.0).max() == np.exp(8.0)                               # the best weighs e^W times the worst
    rng = np.random.default_rng(0)
    k = rng.standard_normal(9)
    assert np.array_equal(mbr.dpp_quality(k, 1.3), ref.quality(k, 1.3))


def test_select_of_table_checks_its_arguments_before_any_device_work():
    with pytest.raises(ValueError, match=r"1\.\.32"):
        mbr.select_of_table(None, None, None, None, [2], [1.0, 1.0], 33)
    with pytest.raises(ValueError, match="qualities for"):
        mbr.select_of_table(None, None, None, None, [2], [1.0], 2)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="finite and > 0"):
            mbr.select_of_table(None, None, None, None, [2], [1.0, bad], 2)
    sel, gain, n_dpp = mbr.select_of_table(None, None, None, None, [0, 0], [], 3)             # no caption at all: no launch
    assert sel.tolist() == [[-1] * 3] * 2 and gain.tolist() == [[0.0] * 3] * 2 and n_dpp.tolist() == [0, 0]


def test_the_entry_checks_its_arguments_before_any_device_work(lib):
    """vc_dpp_select_f64's VC_EINVAL cases and the B == 0 no-op return before anything touches a device, so they run without one: the
    pointers are host blocks that are never dereferenced"""
    import ctypes
    from vae_captioning_amd.abi import VaecapError
    buf = [ctypes.create_string_buffer(64) for _ in range(6)]
    head, gram, q, sel, gain, nd = (ctypes.addressof(b) for b in buf)

    def call(B=2, head=head, max_cands=8, gram=gram, ld=8, q=q, n=4, sel=sel, gain=gain, nd=nd):
        return lib.vc_dpp_select_f64(None, B, head, max_cands, gram, ld, q, n, sel, gain, nd)
    for bad in (dict(B=-1), dict(max_cands=0), dict(max_cands=-3), dict(max_cands=257), dict(n=0), dict(n=-1), dict(n=33), dict(ld=7), dict(ld=-1),
                dict(head=None), dict(gram=None), dict(q=None), dict(sel=None), dict(gain=None), dict(nd=None)):
        with pytest.raises(VaecapError, match="vc_dpp_select_f64: invalid argument"):
            call(**bad)
    assert call(B=0) == 0
    assert call(B=0, head=None, gram=None, q=None, sel=None, gain=None, nd=None) == 0      # B == 0: no pointer is looked at
    with pytest.raises(VaecapError, match="invalid argument"):
        call(B=0, n=0)                                                                      # ... but the scalars still are
    assert all(b.raw == bytes(64) for b in buf)


# ------------------------------------------------------------------ the flags
def test_flag_defaults_and_values():
    p = Parameters().parse_args([])
    assert (p.diverse_select, p.select_n, p.dpp_quality) == ("none", 5, 1.0)
    for mode in ("diverse", "diverse_beam", "stochastic_beam"):
        p = Parameters().parse_args(["--sample_gen", mode, "--diverse_select", "dpp"])
        assert (p.diverse_select, p.select_n, p.dpp_quality) == ("dpp", 5, 1.0)
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_select", "dpp", "--select_n", "32", "--dpp_quality", "0"])
    assert (p.select_n, p.dpp_quality) == (32, 0.0)
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_select", "dpp", "--select_n", "1", "--dpp_quality", "8",
                                 "--diverse_rerank", "mbr"])
    assert (p.select_n, p.dpp_quality, p.diverse_rerank) == (1, 8.0, "mbr")
    assert Parameters().parse_args(["--sample_gen", "diverse", "--diverse_select", "none"]).diverse_select == "none"


@pytest.mark.parametrize("argv,text", [
    (["--diverse_select", "dpp"], "diverse, diverse_beam or"),                                                  # beam_search is the default
    (["--sample_gen", "greedy", "--diverse_select", "dpp"], "got --sample_gen greedy"),
    (["--sample_gen", "marginal_beam", "--diverse_select", "dpp"], "got --sample_gen marginal_beam"),
    (["--sample_gen", "diverse", "--select_n", "3"], "belong to --diverse_select dpp"),
    (["--sample_gen", "diverse", "--dpp_quality", "1.0"], "belong to --diverse_select dpp"),
    (["--sample_gen", "diverse", "--diverse_select", "none", "--select_n", "3"], "belong to --diverse_select dpp"),
    (["--sample_gen", "diverse", "--diverse_select", "dpp", "--select_n", "0"], "--select_n must be 1..32"),
    (["--sample_gen", "diverse", "--diverse_select", "dpp", "--select_n", "33"], "--select_n must be 1..32"),
    (["--sample_gen", "diverse", "--diverse_select", "dpp", "--dpp_quality", "-0.1"], "--dpp_quality must be in [0, 8]"),
    (["--sample_gen", "diverse", "--diverse_select", "dpp", "--dpp_quality", "8.5"], "--dpp_quality must be in [0, 8]"),
    (["--sample_gen", "diverse", "--diverse_select", "dpp", "--dpp_quality", "nan"], "--dpp_quality must be in [0, 8]"),
    (["--sample_gen", "diverse", "--diverse_select", "greedy"], "invalid choice"),
])
def test_flag_errors(argv, text, capsys):
    with pytest.raises(SystemExit) as e:
        Parameters().parse_args(argv)
    assert e.value.code == 2
    assert text in " ".join(capsys.readouterr().err.split())


@pytest.mark.parametrize("argv,text", [
    (["--diverse_select", "dpp"], "--diverse_select dpp belongs to --gen_method diverse / stochastic_beam (got --gen_method greedy)"),
    (["--gen_method", "diverse", "--select_n", "3"], "--select_n / --dpp_quality belong to --diverse_select dpp"),
    (["--gen_method", "diverse", "--diverse_select", "dpp", "--select_n", "33"], "--select_n must be 1..32"),
    (["--gen_method", "stochastic_beam", "--diverse_select", "dpp", "--dpp_quality", "9"], "--dpp_quality must be in [0, 8]"),
])
def test_gen_caption_argument_errors(argv, text):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "gen_caption.py")] + argv, capture_output=True, text=True)
    assert r.returncode == 2 and text in " ".join(r.stderr.split()), r.stderr


def test_metrics_file_names_the_flags_only_when_a_selection_ran(tmp_path, monkeypatch):
    import json
    from vae_captioning_amd.evaluate import METRICS
    from vae_captioning_amd.ops.inference import store_metrics
    monkeypatch.chdir(tmp_path)
    metrics = {k: 0.5 for k in METRICS}
    p = Parameters().parse_args(["--sample_gen", "diverse"])
    plain = store_metrics(p, metrics, 2, 4)
    assert not {"diverse_select", "select_n", "dpp_quality"} & set(plain)
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_select", "dpp", "--select_n", "3"])
    with_sel = store_metrics(p, metrics, 2, 4)
    assert set(with_sel) == set(plain) | {"diverse_select", "select_n", "dpp_quality"}
    assert json.load(open(tmp_path / "val_00_metrics.json")) == with_sel
    assert (with_sel["diverse_select"], with_sel["select_n"], with_sel["dpp_quality"]) == ("dpp", 3, 1.0)
