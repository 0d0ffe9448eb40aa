"""CPU: decoding controls -- DecodeControls and parse_banned (controls.py), the command-line flags, and the float64 reference
(tests/controls_ref.py) that the GPU tests compare the decoders with: what its outputs satisfy, that it is oracle.decode's search when
the controls are off, and that every end-to-end case of tests/test_gpu_controls.py is SAFE (its smallest decision margin exceeds ten
times the score tolerance rtol 1e-4, atol 1e-5 of the beam tests -- no case may be unsafe)."""
import inspect
import json
import types

import numpy as np
import pytest

from oracle import decode as od
from vae_captioning_amd.controls import DecodeControls, active, from_params, load_banned, parse_banned
from vae_captioning_amd.utils.parameters import Parameters

from . import controls_ref as ref

BOS, EOS = ref.BOS, ref.EOS
CASE_GRID = [(k, mode, name) for k in range(len(ref.CASES)) for mode in ref.MODES for name in ref.SETTINGS]
GRID_IDS = ["%s-%s-%s" % (ref.CASE_IDS[k], mode, name) for k, mode, name in CASE_GRID]


# ------------------------------------------------------------------ DecodeControls
def test_defaults_are_a_noop():
    c = DecodeControls()
    assert c.is_noop() and active(c) is None and active(None) is None
    assert (c.no_repeat_ngram, c.min_len, c.repetition_penalty, c.banned.tolist()) == (0, 0, 1.0, [])
    assert c.banned.dtype == np.int32
    for kw in (dict(no_repeat_ngram=1), dict(min_len=1), dict(repetition_penalty=1.5), dict(banned=[4])):
        c = DecodeControls(**kw)
        assert not c.is_noop() and active(c) is c


def test_banned_is_sorted_unique_int32():
    c = DecodeControls(banned=[9, 3, 9, np.int64(5), 3])
    assert c.banned.dtype == np.int32 and c.banned.tolist() == [3, 5, 9]
    assert DecodeControls(banned=range(256)).banned.size == 256
    assert DecodeControls(banned={7, 4}).banned.tolist() == [4, 7]


@pytest.mark.parametrize("kw", [dict(no_repeat_ngram=-1), dict(no_repeat_ngram=9), dict(no_repeat_ngram=2.0), dict(no_repeat_ngram=True),
                                dict(min_len=-1), dict(min_len=1.5), dict(repetition_penalty=0.99), dict(repetition_penalty=10.5),
                                dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")), dict(repetition_penalty="2"),
                                dict(banned=[-1]), dict(banned=[1.5]), dict(banned=["dog"]), dict(banned=[True]), dict(banned=range(257))])
def test_invalid_values_raise(kw):
    with pytest.raises(ValueError):
        DecodeControls(**kw)


def test_key_is_hashable_and_names_what_a_graph_bakes():
    a, b = DecodeControls(2, 5, 1.3, [4, 9]), DecodeControls(2, 5, 1.3, [7, 11])
    assert hash(a.key()) == hash(b.key()) and a.key() == b.key()          # another list of the same length: the same graph
    assert len({a.key(), DecodeControls(3, 5, 1.3, [4, 9]).key(), DecodeControls(2, 4, 1.3, [4, 9]).key(),
                DecodeControls(2, 5, 1.2, [4, 9]).key(), DecodeControls(2, 5, 1.3, [4]).key()}) == 5
    with pytest.raises(ValueError):
        active("ngram=2")


def test_call_checks():
    DecodeControls(2, 5, 1.3, [4, 9]).check(40, EOS, 10, [[[5, 6]], []])
    for c, args in ((DecodeControls(banned=[EOS]), (40, EOS, 10)),            # <EOS> banned
                    (DecodeControls(banned=[40]), (40, EOS, 10)),             # outside the vocabulary
                    (DecodeControls(banned=range(3, 32)), (40, EOS, 10)),     # 29 + 10 + 1 >= 40: a row could lose every word
                    (DecodeControls(min_len=10), (40, EOS, 10)),              # min_len >= max_len
                    (DecodeControls(banned=[6]), (40, EOS, 10, [[[5, 6]], []]))):   # banned and required
        with pytest.raises(ValueError):
            c.check(*args)
    DecodeControls(banned=range(3, 31)).check(40, EOS, 10)                  # 28 + 10 + 1 < 40


def _vocab(V=12):
    words = ["<PAD>", "<BOS>", "<EOS>"] + ["w%d" % i for i in range(3, V)]
    return types.SimpleNamespace(word2idx={w: i for i, w in enumerate(words)}, vocab_size=V)


def test_parse_banned_words_ids_and_unknowns(capsys, tmp_path):
    v = _vocab()
    assert parse_banned(["w5", 7, "w5", "zebra", 99, -3, "w3"], v) == [3, 5, 7]
    assert "3 token ids; dropped 3 unknown words" in capsys.readouterr().out
    assert parse_banned("w4, w9,nothing", v) == [4, 9]
    with pytest.raises(ValueError):
        parse_banned([1.5], v)
    with pytest.raises(ValueError):
        parse_banned({"w5": 1}, v)
    f = tmp_path / "ban.json"
    f.write_text(json.dumps(["w6", 4]))
    assert load_banned(str(f), v) == [4, 6]
    f.write_text(json.dumps({"w6": 1}))
    with pytest.raises(ValueError):
        load_banned(str(f), v)
    p = Parameters()
    assert from_params(p, v) is None
    p.no_repeat_ngram, p.banned_words = 2, None
    assert from_params(p, v).key() == DecodeControls(2).key()


# ------------------------------------------------------------------ the flags
def test_flags_default_off_and_parse():
    p = Parameters().parse_args(["--synthetic"])
    assert (p.no_repeat_ngram, p.min_len, p.repetition_penalty, p.banned_words) == (0, 0, 1.0, None)
    p = Parameters().parse_args(["--synthetic", "--no_repeat_ngram", "2", "--min_len", "5", "--repetition_penalty", "1.3", "--banned_words", "f.json"])
    assert (p.no_repeat_ngram, p.min_len, p.repetition_penalty, p.banned_words) == (2, 5, 1.3, "f.json")


@pytest.mark.parametrize("argv", [["--no_repeat_ngram", "9"], ["--no_repeat_ngram", "-1"], ["--min_len", "-1"], ["--min_len", "30"],
                                  ["--repetition_penalty", "0.5"], ["--repetition_penalty", "11"], ["--repetition_penalty", "nan"],
                                  ["--sample_gen", "marginal_greedy", "--no_repeat_ngram", "2"], ["--sample_gen", "marginal_beam", "--min_len", "3"],
                                  ["--sample_gen", "marginal_greedy", "--repetition_penalty", "1.2"],
                                  ["--sample_gen", "marginal_beam", "--banned_words", "f.json"]])
def test_flag_errors(argv, capsys):
    with pytest.raises(SystemExit):
        Parameters().parse_args(["--synthetic"] + argv)
    capsys.readouterr()


def test_the_keyword_is_on_the_six_decoders_only():
    from vae_captioning_amd.generate import CaptionGenerator
    for name in ("greedy", "sample", "diverse", "beam_search", "diverse_beam_search", "constrained_beam_search"):
        assert inspect.signature(getattr(CaptionGenerator, name)).parameters["controls"].default is None
    for name in ("marginal_greedy", "marginal_beam_search", "score", "bound"):
        assert "controls" not in inspect.signature(getattr(CaptionGenerator, name)).parameters


# ------------------------------------------------------------------ the definition (process_row)
def test_overlapping_occurrences_count():
    a = 3
    x = np.zeros(6)
    out = ref.process_row(x, [a, a, a], DecodeControls(no_repeat_ngram=2), EOS)
    assert out[a] == ref.BANNED_LOGIT and np.count_nonzero(out) == 1
    assert np.array_equal(ref.process_row(x, [a], DecodeControls(no_repeat_ngram=2), EOS), x)          # W < n: nothing
    out = ref.process_row(x, [3, 4, 5, 3], DecodeControls(no_repeat_ngram=2), EOS)                      # ... 3 -> 4 is banned
    assert np.flatnonzero(out).tolist() == [4]
    out = ref.process_row(x, [3, 4, 5], DecodeControls(no_repeat_ngram=1), EOS)                         # n = 1: every emitted word
    assert np.flatnonzero(out).tolist() == [3, 4, 5]


def test_penalty_once_per_distinct_word_and_a_ban_wins():
    x = np.array([2.0, -2.0, 0.0, 4.0, -4.0, 1.0], np.float32)
    c = DecodeControls(repetition_penalty=2.0)
    out = ref.process_row(x, [0, 0, 0, 1, 1, 2, -7, 6], c, 5)
    assert out.dtype == np.float32 and out.tolist() == [1.0, -4.0, 0.0, 4.0, -4.0, 1.0]
    out = ref.process_row(x, [3, 3], DecodeControls(repetition_penalty=2.0, banned=[3], min_len=3), 5)
    assert out.tolist() == [2.0, -2.0, 0.0, ref.BANNED_LOGIT, -4.0, ref.BANNED_LOGIT]
    out = ref.process_row(x, [3, 3, 1], DecodeControls(min_len=3), 5)                                  # W = m: <EOS> free again
    assert np.array_equal(out, x)
    assert np.isfinite(ref.BANNED_LOGIT) and np.float32(ref.BANNED_LOGIT) == -np.finfo(np.float32).max


def test_process_row_follows_the_dtype():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(40)
    c = DecodeControls(2, 4, 1.3, [5, 9])
    a, b = ref.process_row(x, [3, 4, 3], c, EOS), ref.process_row(x.astype(np.float32), [3, 4, 3], c, EOS)
    assert a.dtype == np.float64 and b.dtype == np.float32
    np.testing.assert_allclose(b, a, rtol=1e-6)


# ------------------------------------------------------------------ the searches
@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=ref.CASE_IDS)
def test_controls_off_is_the_oracle(k):
    p, P0, feats, cv, eps, cm = ref.model_inputs(5, **ref.CASES[k])
    P64 = {kk: v.astype(np.float64) for kk, v in P0.items()}
    off = DecodeControls()
    for b in range(feats.shape[0]):
        a = (P64, p, feats[b].astype(np.float64), cv[b].astype(np.float64), eps[:, b:b + 1].astype(np.float64), BOS, EOS)
        assert ref.greedy(*a, off, c_means=cm, max_len=10)[0] == od.greedy(*a, c_means=cm, max_len=10)
        s, sc, _ = ref.beam_search(*a, off, c_means=cm, beam_size=3, max_len=10)
        s0, sc0 = od.beam_search(*a, c_means=cm, beam_size=3, max_len=10)
        assert s == s0 and sc == sc0


def _captions(mode, res):
    """every caption (without <BOS>) of one image's reference result"""
    if mode == "greedy":
        return [res[0]]
    if mode == "beam_search":
        return [s[1:] for s in res[0]]
    return [s[1:] for bank in res for s in bank[0]]


@pytest.mark.parametrize("k,mode,name", CASE_GRID, ids=GRID_IDS)
def test_every_gpu_case_is_safe_and_keeps_its_promises(k, mode, name):
    out, margin = ref.run_case(k, mode, name)
    print("margin %.3g" % margin)
    assert margin > ref.SAFE_MARGIN
    ctl = ref.settings()[name]
    n = 0
    for res in out:
        for cap in _captions(mode, res):
            assert ref.properties(cap, ctl, EOS) == (True, True, True), cap
            n += 1
    assert n >= len(out)


@pytest.mark.parametrize("name", ref.SETTINGS)
def test_the_controls_change_what_is_decoded(name):
    """(a case whose captions the controls leave alone would test nothing)"""
    changed = 0
    for k in range(len(ref.CASES)):
        on = ref.run_case(k, "greedy", name)[0]
        off = [ref.run_image(k, "greedy", None, i)[0] for i in ref.IMAGES[(k, "greedy", name)]]
        changed += sum(a[0] != b[0] for a, b in zip(on, off))
    assert changed > 0
