"""Host side of consensus re-ranking (vae_captioning_amd/consensus.py): CIDEr-D values worked by hand on the float64 reference
(tests/consensus_ref.py), the df / idf table, n-gram keys, the limits, the training-image gatherer, the flags and the tie rule of
the re-ordering.  No GPU."""
import math

import numpy as np
import pytest

from vae_captioning_amd import consensus as cs
from vae_captioning_amd.utils.parameters import Parameters

from . import consensus_ref as ref

BOS, EOS = 1, 2


def _vec(tokens, index):
    idf, unseen = ref.df_idf(index, BOS, EOS)
    return ref.vector(tokens, BOS, EOS, idf, unseen)


# an index in which every n-gram of [5 6 7 8 9] is missing from at least one image (the second image shares nothing with it)
INDEX = [[[BOS, 5, 6, 7, 8, 9, EOS]], [[BOS, 20, 21, EOS]], [[BOS, 5, 30, EOS]]]


def test_a_caption_against_itself_scores_ten():
    v = _vec([5, 6, 7, 8, 9, EOS], INDEX)
    assert abs(ref.cider_d(v, v) - 10.0) < 1e-12


def test_a_two_word_caption_has_no_3_or_4_grams_and_scores_five():
    v = _vec([5, 6], INDEX)
    assert abs(ref.cider_d(v, v) - 5.0) < 1e-12


def test_disjoint_captions_score_zero():
    assert ref.cider_d(_vec([5, 6, 7], INDEX), _vec([20, 21, 30], INDEX)) == 0.0


def test_a_pure_length_difference_scales_by_the_gaussian_penalty():
    # c and r have the same n-gram vectors but r has three more tokens that are PAD / BOS / EOS: not words, so no penalty...
    c = _vec([5, 6, 7, 8, 9], INDEX)
    assert abs(ref.cider_d(c, _vec([BOS, 5, 6, 0, 7, 8, 9, EOS, 0], INDEX)) - 10.0) < 1e-12
    # ...while a pure 3-word length difference (same vectors, different L) scales the score by exp(-9/72)
    L, vec, norms = c
    assert abs(ref.cider_d((L + 3, vec, norms), c) - 10.0 * math.exp(-9.0 / 72.0)) < 1e-12


def test_a_repeated_word_is_clipped_by_the_min():
    idx = [[[5, 6]], [[7]]]
    idf, unseen = ref.df_idf(idx, BOS, EOS)
    c = ref.vector([5, 5, 5], BOS, EOS, idf, unseen)
    r = ref.vector([5], BOS, EOS, idf, unseen)
    w = float(idf[5])
    # sim_1 = min(3w, w) * w / (3w * w) = 1/3; no 2-, 3- or 4-grams in r
    assert abs(ref.cider_d(c, r) - 10.0 * math.exp(-4.0 / 72.0) * (1.0 / 3.0) / 4.0) < 1e-12
    assert c[1][1][cs.ngram_key([5])] == np.float32(3) * idf[5]


def test_df_counts_images_not_captions_and_unseen_ngrams_get_log_d():
    caps = [[[BOS, 5, 6, EOS], [BOS, 5, 6, EOS], [5, 7]], [[8, 9]], [[5, 9, EOS]], [[10]]]
    h = cs.host_index(caps, BOS, EOS)
    table = dict(zip(h.df_keys.tolist(), h.idf.tolist()))
    D = 4
    assert h.D == D
    assert table[cs.ngram_key([5])] == np.float32(math.log(D) - math.log(2))        # images 0 and 2 (three captions of image 0: once)
    assert table[cs.ngram_key([5, 6])] == np.float32(math.log(D) - math.log(1))
    assert table[cs.ngram_key([9])] == np.float32(math.log(D) - math.log(2))
    assert cs.ngram_key([6, 5]) not in table and cs.ngram_key([BOS, 5]) not in table
    assert h.idf_unseen == np.float32(math.log(D))
    ridf, runseen = ref.df_idf(caps, BOS, EOS)
    assert table == {g: float(v) for g, v in ridf.items()} and runseen == h.idf_unseen
    assert h.img_cap.tolist() == [0, 3, 4, 5, 6] and h.L.tolist() == [2, 2, 2, 2, 2, 1]
    assert list(h.df_keys) == sorted(h.df_keys)


def test_df_table_matches_the_reference_on_random_captions():
    rng = np.random.default_rng(3)
    caps = [[[BOS] + rng.integers(3, 12, size=rng.integers(0, 9)).tolist() + [EOS] for _ in range(rng.integers(1, 4))] for _ in range(40)]
    h = cs.host_index(caps, BOS, EOS)
    ridf, _ = ref.df_idf(caps, BOS, EOS)
    assert dict(zip(h.df_keys.tolist(), h.idf.tolist())) == {g: float(v) for g, v in ridf.items()}


def test_keys_round_trip_through_packing():
    for g in ([1], [65535], [3, 4], [7, 1, 65535], [65535, 65535, 65535, 65535], [9, 8, 7, 6]):
        k = cs.ngram_key(g)
        assert cs.unpack_key(k) == g and k == ref.key(g)
        assert k < 2 ** 64
    assert cs.ngram_key([1, 2]) == (1 << 16) | 2           # last word in the low bits
    W, L = cs.word_rows([[BOS, 7, 1, 65535, 4, EOS, 0]], BOS, EOS)
    keys, rows = cs.ngram_keys(W, L)
    assert sorted(keys.tolist()) == sorted(ref.key(g) for n in range(1, 5) for g in [[7, 65535, 4][i:i + n] for i in range(4 - n)])


def test_ids_above_65535_and_captions_over_64_words_raise():
    with pytest.raises(ValueError, match="65535"):
        cs.host_index([[[BOS, 5, 65536, EOS]]], BOS, EOS)
    with pytest.raises(ValueError, match="65536"):
        cs.host_index([[[5]]], BOS, EOS, vocab_size=65537)
    cs.host_index([[[5]]], BOS, EOS, vocab_size=65536)
    cs.host_index([[[BOS] + [5] * 64 + [EOS]]], BOS, EOS)
    with pytest.raises(ValueError, match="index image 2 has 65 words"):
        cs.host_index([[[5]], [[6]], [[7], [BOS] + [5] * 65 + [EOS]]], BOS, EOS)
    with pytest.raises(ValueError, match="no caption"):
        cs.host_index([[[5]], []], BOS, EOS)


def test_limits_name_the_limit():
    with pytest.raises(ValueError, match="1..256"):
        cs.check_limits(0, 125)
    with pytest.raises(ValueError, match="1..256"):
        cs.check_limits(257, 125)
    with pytest.raises(ValueError, match=">= 1"):
        cs.check_limits(90, 0)
    cs.check_limits(256, 1)


def test_capacity_counts_every_ngram_slot():
    assert cs.capacity([0, 1, 2, 3, 4, 64]).tolist() == [0, 1, 3, 6, 10, 64 + 63 + 62 + 61]


# ------------------------------------------------------------------ training images of a Batch_Generator
class _FakeGen(object):
    """The attributes index_data_from_generator reads: a repartitioned generator (train + part of val, the rest held out)."""

    def __init__(self):
        self._iterable = ["/d/train2014/t0.jpg", "/d/train2014/t1.jpg", "/d/val2014/v0.jpg", "/d/val2014/v1.jpg"]
        self.unused_cap_in = ["/d/val2014/v2.jpg", "/d/val2014/v3.jpg"]
        self.feature_dict = {"t0.jpg": np.full((1, 4), 1.0), "t1.jpg": np.full((1, 4), 2.0)}
        self.val_feature_dict = {"v0.jpg": np.full((1, 4), 3.0), "v1.jpg": np.full((1, 4), 4.0), "v2.jpg": np.full((1, 4), 5.0),
                                 "v3.jpg": np.full((1, 4), 6.0)}
        self.captions = {"t0.jpg": [[BOS, 5, EOS]], "t1.jpg": [[BOS, 6, EOS], [BOS, 7, EOS]]}
        self.val_captions = {"v0.jpg": [[BOS, 8, EOS]], "v1.jpg": [[BOS, 9, EOS]], "v2.jpg": [[BOS, 10, EOS]], "v3.jpg": [[BOS, 11, EOS]]}

    def _lookup(self, d, alt, key):
        if key in d:
            return d[key]
        if alt is not None and key in alt:
            return alt[key]
        raise KeyError(key)


def test_index_data_from_generator_takes_training_images_only():
    g = _FakeGen()
    feats, caps = cs.index_data_from_generator(g)
    assert feats.dtype == np.float32 and feats.shape == (4, 4)
    assert feats[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0]
    assert caps == [[[BOS, 5, EOS]], [[BOS, 6, EOS], [BOS, 7, EOS]], [[BOS, 8, EOS]], [[BOS, 9, EOS]]]
    g._iterable.append("/d/val2014/v2.jpg")    # even if a held-out image reached the list, it stays out of the index
    feats, caps = cs.index_data_from_generator(g)
    assert feats.shape[0] == 4 and [[BOS, 10, EOS]] not in caps
    g.feature_dict = None
    with pytest.raises(ValueError, match="fc2"):
        cs.index_data_from_generator(g)


# ------------------------------------------------------------------ flags
def test_consensus_flag_defaults_and_validation():
    q = Parameters().parse_args([])
    assert q.diverse_rerank == "likelihood" and q.consensus_k == 90 and q.consensus_m == 125
    assert Parameters().diverse_rerank == "likelihood"
    p = Parameters().parse_args(["--sample_gen", "diverse", "--diverse_rerank", "consensus", "--consensus_k", "12", "--consensus_m", "7"])
    assert p.diverse_rerank == "consensus" and p.consensus_k == 12 and p.consensus_m == 7 and isinstance(p.consensus_k, int)
    for bad in (["--diverse_rerank", "cider"], ["--consensus_k", "0"], ["--consensus_k", "257"], ["--consensus_m", "0"]):
        with pytest.raises(SystemExit):
            Parameters().parse_args(bad)
    Parameters().parse_args(["--consensus_k", "256", "--consensus_m", "1"])


# ------------------------------------------------------------------ re-ordering
def test_reordering_is_by_consensus_and_exact_ties_keep_the_likelihood_order():
    entries = [([5, EOS], -0.1, 3), ([6, EOS], -0.2, 1), ([7, EOS], -0.3, 1), ([8, EOS], -0.4, 2)]
    got = cs.rerank_entries(entries, [1.0, 2.5, 1.0, 2.5])
    assert [e[0][0] for e in got] == [6, 8, 5, 7]
    assert got[0] == ([6, EOS], -0.2, 1, 2.5)
    assert [e[0][0] for e in cs.rerank_entries(entries, [0.0] * 4)] == [5, 6, 7, 8]
    assert [e[0][0] for e in cs.rerank_entries(entries, [0.0, 3.0, 1.0, 3.0], n_best=2)] == [6, 8]
