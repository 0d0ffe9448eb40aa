"""CPU: constrained beam search -- the reference of tests/cbs_ref.py pinned before it judges the kernel (its identities with plain
beam search, the candidate-list rule, the bank invariant, the result selection), the condition under which the GPU tests may compare
token ids exactly, and the host end (the constraints file, the flags, the argument checks)."""
import functools
import json

import numpy as np
import pytest

from oracle import decode as od
from vae_captioning_amd.constraints import Constraints, load_constraints, parse_must_include
from vae_captioning_amd.generate import check_constraints, select_bank
from vae_captioning_amd.utils.parameters import Parameters

from . import cbs_ref

BOS, EOS, V, B = 1, 2, 40, 6
SHAPES = [(0, 0, 5), (1, 1, 8), (1, 4, 2), (2, 2, 4), (3, 1, 2), (3, 4, 2), (2, 3, 3)]   # (C, Wc, w): the GPU test's end-to-end shapes


@functools.lru_cache(maxsize=None)
def inputs(case):
    return cbs_ref.model_inputs(7, V=V, B=B, **cbs_ref.CASES[case])


def cons_of(C, Wc):
    return cbs_ref.constraints(100 + 10 * C + Wc, B, V, C, Wc)


@functools.lru_cache(maxsize=None)
def ref(case, C, Wc, w, dtype=np.float64, kc=None):
    return cbs_ref.reference(*inputs(case), BOS, EOS, cons_of(C, Wc), dtype=dtype, kc=kc, beam_size=w, max_len=10)


@functools.lru_cache(maxsize=None)
def plain(case, beam, barred=None):
    p, P0, feats, cv, eps, cm = inputs(case)
    P64 = {k: v.astype(np.float64) for k, v in P0.items()}
    args = lambda b: (P64, p, feats[b].astype(np.float64), cv[b].astype(np.float64), eps[:, b:b + 1].astype(np.float64), BOS, EOS)
    if barred is None:
        return [od.beam_search(*args(b), c_means=cm, beam_size=beam, max_len=10) for b in range(B)]
    return [cbs_ref.barred_beam_search(*args(b), barred[b], c_means=cm, beam_size=beam, max_len=10) for b in range(B)]


@pytest.mark.parametrize("case", range(4), ids=cbs_ref.CASE_IDS)
def test_no_constraints_is_the_plain_beam_search(case):
    for w in (2, 5):
        got = ref(case, 0, 0, w)
        assert all(len(im) == 1 for im in got)
        assert [im[0] for im in got] == plain(case, w)   # (sentences, scores) exactly: the same float64 operations in the same order


def test_barred_search_without_barred_words_is_the_oracles():
    assert plain(1, 3, tuple(() for _ in range(B))) == plain(1, 3)


@pytest.mark.parametrize("case", range(4), ids=cbs_ref.CASE_IDS)
@pytest.mark.parametrize("C,Wc,w", SHAPES[1:])
def test_the_first_w_plus_NW_words_of_a_row_are_enough(case, C, Wc, w):
    """At most NW listed words are barred, so the first w admissible words of the whole vocabulary are among the w + NW most probable:
    the product's list length returns the banks of the full sort, scores included."""
    assert cbs_ref.n_words(cons_of(C, Wc), V) == C * Wc
    assert ref(case, C, Wc, w, kc="call") == ref(case, C, Wc, w)


@pytest.mark.parametrize("case", range(4), ids=cbs_ref.CASE_IDS)
@pytest.mark.parametrize("C,Wc,w", SHAPES[1:])
def test_bank_invariant_and_bank_zero(case, C, Wc, w):
    """Every caption of bank t contains a word of each set in t and no word of any set outside t; bank 0 is a beam search over the
    vocabulary without the constraint words; the banks of an absent set stay empty; every image's accepting bank holds a caption."""
    cons, got = cons_of(C, Wc), ref(case, C, Wc, w)
    barred = tuple(tuple(int(v) for v in cons[b].ravel() if v >= 0) for b in range(B))
    zero = plain(case, w, barred)
    for b in range(B):
        sets, full = cbs_ref.sets_of(cons[b], V), cbs_ref.full_mask(cons[b], V)
        assert len(got[b]) == 1 << C
        for t, (sentences, _) in enumerate(got[b]):
            if t & ~full:
                assert sentences == [], (b, t)
            for s in sentences:
                met = sum(1 << j for j, st in enumerate(sets) if set(st) & set(s))
                assert met == t, (b, t, s, sets)
        assert got[b][0] == zero[b], b
        assert len(got[b][full][0]) > 0, b
    if C >= 2:
        assert cbs_ref.full_mask(cons[B - 1], V) == (1 << (C - 1)) - 1   # the image with fewer sets than the call


@pytest.mark.parametrize("case", range(4), ids=cbs_ref.CASE_IDS)
@pytest.mark.parametrize("C,Wc,w", SHAPES)
def test_float32_and_float64_references_return_the_same_captions(case, C, Wc, w):
    """The condition under which the GPU parity test (float32 kernels against the float64 reference) may ask for identical token ids:
    on its inputs (seed 7, max_len 10) no selection is closer than float32's error -- every image, every bank, no exceptions."""
    r32, r64 = ref(case, C, Wc, w, dtype=np.float32), ref(case, C, Wc, w)
    for b in range(B):
        assert [g[0] for g in r32[b]] == [g[0] for g in r64[b]], b
        for g32, g64 in zip(r32[b], r64[b]):
            np.testing.assert_allclose(g32[1], g64[1], rtol=1e-4, atol=1e-5)


def test_a_round_by_hand():
    """one image, one constraint {7}, w = 1: round 1 leaves bank 0 its best free word and forces 7 into bank 1; round 2 moves bank 0's
    beam into bank 1 only if it beats what bank 1 made of its own beam"""
    probs = np.full((2, 10), 1e-13, np.float32)
    probs[0, [7, 5, 6]] = [0.5, 0.25, 0.125]
    cons = np.array([[[7]]], np.int32)
    rounds = cbs_ref.table_rounds([probs, probs], cons, 1, 1, 1, 2, BOS, EOS, 0.7)
    partial, complete = next(rounds)
    b0, = partial[0][0]._data
    b1, = partial[0][1]._data
    assert b0.sentence == [BOS, 5] and b0.logprob == float(np.log(np.float32(0.25))) and b0.state == 0
    assert b1.sentence == [BOS, 7] and b1.logprob == float(np.log(np.float32(0.5))) and b1.state == 0   # forced from bank 0's row
    probs[1, [7, 5]] = [0.25, 0.5]
    partial, complete = next(rounds)
    b0, = partial[0][0]._data
    b1, = partial[0][1]._data
    assert b0.sentence == [BOS, 5, 5] and b0.state == 0
    # bank 1: its own beam's best word (0.5 * 0.5) beats bank 0's beam forced through 7 (0.25 * 0.5); its parent is row 1, bank 1's
    assert b1.sentence == [BOS, 7, 5] and b1.state == 1 and b1.logprob == float(np.log(np.float32(0.5))) * 2
    assert all(c.size() == 0 for c in complete[0])


def test_result_selection_order():
    cap = lambda *w: ([BOS] + list(w) + [EOS], -1.0)
    live = lambda *w: ([BOS] + list(w), -2.0)
    # full = 0b11: the accepting bank first
    banks = [[cap(5)], [cap(7)], [cap(8)], [cap(7, 8)]]
    assert select_bank(banks, 3, EOS) == ([cap(7, 8)], 3)
    # the accepting bank stays empty: one constraint met, the smaller mask first
    assert select_bank([[cap(5)], [cap(7)], [cap(8)], []], 3, EOS) == ([cap(7)], 1)
    assert select_bank([[cap(5)], [], [cap(8)], []], 3, EOS) == ([cap(8)], 2)
    # a complete caption of a lesser bank beats live beams of a better one; live beams only when nothing is complete
    assert select_bank([[cap(5)], [live(7)], [], [live(7, 8)]], 3, EOS) == ([cap(5)], 0)
    assert select_bank([[live(5)], [live(7)], [], []], 3, EOS) == ([live(7)], 1)
    # banks outside the image's accepting state are never looked at (full = 0b01: the image has one set of the call's two)
    assert select_bank([[cap(5)], [], [cap(9)], [cap(9)]], 1, EOS) == ([cap(5)], 0)
    assert select_bank([[], [], [], []], 3, EOS) == ([], 0)
    # the reference's own selection agrees
    as_ref = lambda banks: [([s for s, _ in bk], [sc for _, sc in bk]) for bk in banks]
    for banks, full in ((banks, 3), ([[cap(5)], [], [cap(8)], []], 3), ([[live(5)], [live(7)], [], []], 3)):
        (sents, scores), state = cbs_ref.select(as_ref(banks), full, EOS)
        assert (list(zip(sents, scores)), state) == select_bank(banks, full, EOS)


# ---------------------------------------------------------------- host end
W2I = {"<PAD>": 0, "<BOS>": 1, "<EOS>": 2, "dog": 3, "puppy": 4, "frisbee": 5, "grass": 6, "park": 7, "a": 8}


def test_constraints_file_parsing(tmp_path):
    path = tmp_path / "c.json"
    path.write_text(json.dumps({"*": [["dog", "puppy", "wolf"], [5]], "img1": [["grass"], ["unicorn"], ["park", 7, 99, 2]], "42": []}))
    c = load_constraints(str(path), W2I, 9, 1, 2)
    assert c.default == [[3, 4], [5]] and c.by_id == {"img1": [[6], [7]], "42": []}
    assert (c.dropped_words, c.dropped_sets) == (4, 1)   # wolf, unicorn, 99 (outside the vocabulary), 2 (<EOS>); the unicorn set
    assert c.C == 2 and c.width == 4                     # the largest that fits: 16 >> 2
    assert c.for_images(["img1", 42, "other"]) == [[[6], [7]], [], [[3, 4], [5]]]
    assert "4 unknown words" in c.summary() and "1 emptied sets" in c.summary()
    assert load_constraints(str(path), W2I, 9, 1, 2, width=3).width == 3
    with pytest.raises(ValueError, match="beams per state"):
        load_constraints(str(path), W2I, 9, 1, 2, width=5)   # 5 << 2 > 16
    m = parse_must_include("dog,puppy;frisbee", W2I, 9, 1, 2)
    assert m.default == [[3, 4], [5]] and m.width == 4 and m.for_images(["x.jpg"]) == [[[3, 4], [5]]]
    assert parse_must_include("", W2I, 9, 1, 2).width == 16


@pytest.mark.parametrize("entries,word", [({"*": [["dog"], ["puppy"], ["grass"], ["park"]]}, "4 sets"),
                                          ({"*": [["dog", "puppy", "grass", "park", "a"]]}, "5 words"),
                                          ({"*": [["dog", "puppy"], ["frisbee", "dog"]]}, "two sets"),
                                          ({"*": [["dog", 1.5]]}, "string or an integer"), ({"*": ["dog"]}, "list of word lists"), (["dog"], "JSON object")])
def test_constraints_file_errors(entries, word):
    with pytest.raises(ValueError, match=word):
        Constraints(entries, W2I, 9, 1, 2)


def test_flags_defaults_and_values():
    p = Parameters().parse_args(["--sample_gen", "constrained_beam", "--constraints", "c.json"])
    assert (p.sample_gen, p.constraints, p.cbs_width) == ("constrained_beam", "c.json", 0)
    p = Parameters().parse_args(["--sample_gen", "constrained_beam", "--constraints", "c.json", "--cbs_width", "4"])
    assert p.cbs_width == 4
    p = Parameters().parse_args([])
    assert p.constraints is None and p.cbs_width == 0 and p.sample_gen == "beam_search"


@pytest.mark.parametrize("argv,flag", [(["--sample_gen", "constrained_beam"], "--constraints"),
                                       (["--sample_gen", "constrained_beam", "--constraints", "c.json", "--cbs_width", "17"], "--cbs_width"),
                                       (["--sample_gen", "constrained_beam", "--constraints", "c.json", "--cbs_width", "-1"], "--cbs_width"),
                                       (["--constraints", "c.json"], "--constraints"), (["--sample_gen", "greedy", "--cbs_width", "2"], "--cbs_width"),
                                       (["--sample_gen", "diverse_beam", "--constraints", "c.json"], "--constraints")])
def test_flag_errors_name_the_flag(argv, flag, capsys):
    with pytest.raises(SystemExit):
        Parameters().parse_args(argv)
    assert flag in capsys.readouterr().err


def test_check_constraints_builds_the_table_and_rejects_bad_arguments():
    C, Wc, cons, NW = check_constraints([[[3, 4], [5]], [], [[6]]], 3, 9, 1, 2, 4)
    assert (C, Wc, NW) == (2, 2, 3) and cons.dtype == np.int32
    assert cons.tolist() == [[[3, 4], [5, -1]], [[-1, -1], [-1, -1]], [[6, -1], [-1, -1]]]
    C, Wc, cons, NW = check_constraints([[], []], 2, 9, 1, 2, 16)
    assert (C, Wc, NW) == (0, 1, 0) and cons.shape == (2, 0, 1)
    for bad, w in (([[[3], [4], [5], [6]]], 2), ([[[3, 4, 5, 6, 7]]], 2), ([[[]]], 2), ([[[3, 4], [4]]], 2), ([[[3, 3]]], 2), ([[[9]]], 2),
                   ([[[-1]]], 2), ([[[1]]], 2), ([[[2]]], 2), ([[[3], [4]]], 5), ([[[3]]], 9), ([[]], 17), ([[]], 0), ([[], []], 2), ([[[3.5]]], 2)):
        with pytest.raises(ValueError):
            check_constraints(bad, 1, 9, 1, 2, w)
