"""CPU: the host end of ROUGE-L (vae_captioning_amd/evaluate.py: rouge_l, METRICS; scst.py: SumReward; --scst_rouge) and the
plain-Python reference tests/rouge_ref.py -- the bit-parallel LCS recurrence the kernel runs against the quadratic dynamic programme,
values worked by hand, the tie rule, the float64 formula, the flag and its parse errors, and the weighted sum of rewards."""
import itertools
import pickle

import numpy as np
import pytest

from vae_captioning_amd.utils.parameters import Parameters

from . import rouge_ref as ref

BOS, EOS = 1, 2
THE, CAT, SAT, ON, MAT, IS = 3, 4, 5, 6, 7, 8
EDGES = (0, 1, 31, 32, 33, 63, 64)
TODAY = ("bleu_1", "bleu_2", "bleu_3", "bleu_4", "cider_d", "oracle_cider_d", "mean_cider_d", "distinct", "div_1", "div_2", "mbleu_4",
         "novel")


# ------------------------------------------------------------------ the recurrence
def test_the_bitparallel_recurrence_equals_the_dp_exhaustively_on_two_letters():
    seqs = [list(s) for n in range(7) for s in itertools.product((3, 4), repeat=n)]
    assert len(seqs) == 127
    for a in seqs:
        for b in seqs:
            assert ref.lcs_bitparallel(a, b) == ref.lcs(a, b), (a, b)


@pytest.mark.parametrize("vocab", [2, 50])
def test_the_bitparallel_recurrence_equals_the_dp_at_the_word_size_edges(vocab):
    """lengths around 32 and at 64 (the low mask of 64 positions, the carry out of bit 63), both sides"""
    rng = np.random.default_rng(100 + vocab)
    for la in EDGES:
        for lb in EDGES:
            for _ in range(4):
                a, b = rng.integers(3, 3 + vocab, size=la).tolist(), rng.integers(3, 3 + vocab, size=lb).tolist()
                assert ref.lcs_bitparallel(a, b) == ref.lcs(a, b), (la, lb, a, b)
    assert ref.lcs_bitparallel([5] * 64, [5] * 64) == 64 and ref.lcs_bitparallel([5] * 64, [5] * 3) == 3
    assert ref.lcs_bitparallel([5] * 64, [6] * 64) == 0 and ref.lcs([], [5]) == 0 and ref.lcs_bitparallel([], [5]) == 0


# ------------------------------------------------------------------ by hand
def test_the_hand_worked_value():
    hyp = [THE, CAT, SAT, ON, MAT]               # "the cat sat on mat"
    r = [THE, CAT, IS, ON, THE, MAT]             # "the cat is on the mat": the cat .. on .. mat
    assert ref.lcs(hyp, r) == 4
    (m, l, n), = ref.overlap([hyp], [r], [0], [1], [-1])
    assert (m, l, n) == (4, 4, 6)
    assert m / len(hyp) == 0.8 and l / n == 2 / 3
    assert ref.rouge_l(m, l, n, len(hyp)) == pytest.approx(0.7155425219941348, rel=1e-15)
    sc = ref.evaluate_rouge([[[BOS] + hyp + [EOS]]], [[[BOS] + r + [EOS, 0, 0]]], BOS, EOS)
    assert sc[0] == sc[1] == sc[2] == sc[3][0][0] == ref.rouge_l(4, 4, 6, 5)


def test_precision_and_recall_take_their_maxima_from_different_references():
    hyp = [THE, CAT, SAT, ON, MAT]
    short = [CAT, ON]                             # contained in the hypothesis: recall 2 / 2
    long_ = [THE, CAT, IS, ON, THE, MAT]          # the larger LCS: 4, recall 4 / 6
    for rows in ([short, long_], [long_, short]):
        (m, l, n), = ref.overlap([hyp], rows, [0], [2], [-1])
        assert (m, l, n) == (4, 2, 2)
    want = (1 + 1.2 ** 2) * 0.8 * 1.0 / (1.0 + 1.2 ** 2 * 0.8)
    assert ref.rouge_l(4, 2, 2, 5) == want and want > ref.rouge_l(4, 4, 6, 5)


def test_a_tie_in_the_ratio_goes_to_the_shorter_reference():
    hyp = [THE, CAT]
    four, two = [THE, IS, CAT, IS], [IS, CAT]     # 2 / 4 and 1 / 2
    for rows in ([four, two], [two, four]):
        (m, l, n), = ref.overlap([hyp], rows, [0], [2], [-1])
        assert (m, l, n) == (2, 1, 2)
    # rows without a word take no part; no row at all: zeros; the skip
    assert ref.overlap([hyp], [[], four, []], [0], [3], [-1]) == [(2, 2, 4)]
    assert ref.overlap([hyp], [[], []], [0], [2], [-1]) == [(0, 0, 0)] and ref.overlap([hyp], [four], [0], [0], [-1]) == [(0, 0, 0)]
    assert ref.overlap([hyp], [four, two], [0], [2], [0]) == [(1, 1, 2)] and ref.overlap([hyp], [four], [0], [1], [0]) == [(0, 0, 0)]
    assert ref.overlap([[MAT]], [four, two], [0], [2], [-1]) == [(0, 0, 2)]     # ratio 0 on both: the shorter


def test_the_product_formula_equals_the_reference_formula():
    from vae_captioning_amd.evaluate import rouge_l
    rng = np.random.default_rng(9)
    h = rng.integers(1, 65, size=400)
    n = rng.integers(1, 65, size=400)
    m = np.array([rng.integers(1, min(a, b) + 1) for a, b in zip(h, n)])
    l = np.array([rng.integers(1, x + 1) for x in m])
    cols = [m, l, n, h]
    for z in range(4):                            # zeros in each of the four inputs
        cols[z][z::7] = 0
    got = rouge_l(*cols)
    want = np.array([ref.rouge_l(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*cols)], np.float64)
    assert got.dtype == np.float64 and got.shape == (400,)
    assert np.array_equal(got, want) and (want == 0).sum() >= 4 * 50 and (want > 0).sum() > 100 and want.max() <= 1.0
    assert rouge_l([4], [4], [6], [5])[0] == pytest.approx(0.7155425219941348, rel=1e-15)
    assert rouge_l([4], [4], [6], [5], beta=1.0)[0] == 2 * 0.8 * (4 / 6) / (4 / 6 + 0.8)
    assert rouge_l([], [], [], []).shape == (0,)


# ------------------------------------------------------------------ flags
def test_scst_rouge_flag():
    p = Parameters().parse_args([])
    assert p.scst_rouge == 0.0 and "scst_rouge" in vars(p)          # materialised on the instance (--save_params pickles vars(p))
    p = Parameters().parse_args("--scst --restore --scst_rouge 0.5".split())
    assert p.scst is True and p.scst_rouge == 0.5
    assert Parameters().parse_args("--scst --scst_rouge 0".split()).scst_rouge == 0.0


@pytest.mark.parametrize("argv", ["--scst_rouge 0.5", "--scst --scst_rouge -1", "--scst --scst_rouge inf", "--scst --scst_rouge nan"],
                         ids=lambda a: a.replace(" ", "_"))
def test_scst_rouge_parse_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        Parameters().parse_args(argv.split())
    assert e.value.code == 2 and "--scst_rouge" in capsys.readouterr().err


def test_an_old_parameters_pickle_reads_back_with_the_default():
    """a Parameters pickled before the flag existed has no such attribute in its instance dict"""
    p = Parameters()
    p.prior, p.scst = "AG", True
    assert "scst_rouge" not in vars(p)
    q = pickle.loads(pickle.dumps(p))
    assert q.prior == "AG" and q.scst is True and q.scst_rouge == 0.0


# ------------------------------------------------------------------ the weighted sum
class _Part(object):
    def __init__(self, values, seconds):
        self.values, self.seconds, self.host_seconds, self.calls = np.asarray(values, np.float64), seconds, 0.0, []

    def rewards(self, cands, refs):
        self.calls.append((cands, refs))
        self.host_seconds += self.seconds
        return self.values


def test_sum_reward_is_the_weighted_sum_of_its_parts():
    from vae_captioning_amd.scst import SumReward
    a, b = _Part([1.0, 2.0, 0.0], 0.25), _Part([0.5, 0.0, 1.0], 0.5)
    s = SumReward([(a, 1), (b, 0.5)])
    cands, refs = [[[3, EOS]], [[4, EOS], [EOS]]], [[[3, EOS]], [[5, EOS]]]
    got = s.rewards(cands, refs)
    assert got.dtype == np.float64 and got.tolist() == [1.25, 2.0, 0.5]
    assert a.calls == b.calls == [(cands, refs)]                    # fake parts hold no word-row entry: each converts for itself
    assert s.host_seconds == 0.75
    s.rewards(cands, refs)
    assert s.host_seconds == 1.5
    s.host_seconds = 0.0                                            # what the timing tool does between steps
    assert s.host_seconds == 0.0 and a.host_seconds == 0.0 and b.host_seconds == 0.0
    with pytest.raises(ValueError):
        SumReward([])


def test_metrics_keep_their_places_and_gain_three():
    from vae_captioning_amd.evaluate import METRICS
    assert METRICS[:12] == TODAY
    assert METRICS[12:] == ("rouge_l", "oracle_rouge_l", "mean_rouge_l")
