"""CPU: the host side of self-critical training -- the float64 reference of the policy loss against finite differences of its own
scalar, the advantages, the policy batch, the flags and their parse errors, an old Parameters pickle, and the document-frequency
table of CiderReward against the float64 CIDEr-D of tests/eval_ref.py / tests/consensus_ref.py."""
import pickle

import numpy as np
import pytest

from vae_captioning_amd import scst
from vae_captioning_amd.utils.parameters import Parameters

from . import consensus_ref as cref
from . import eval_ref
from . import scst_ref as R

BOS, EOS = 1, 2
NEW_DEFAULTS = dict(scst=False, scst_baseline="average", scst_entropy=0.0)


# ------------------------------------------------------------------------------------------------ the loss reference
@pytest.mark.parametrize("beta", [0.0, 0.25])
def test_reference_gradient_matches_finite_differences(beta):
    """central differences of J in float64; the advantages are negative, zero and positive; a PAD row and an out-of-range label are dead"""
    rng = np.random.default_rng(3)
    T, N, V = 3, 3, 7
    x = rng.standard_normal((T * N, V)) * 2.0
    labels = rng.integers(1, V, size=T * N)
    labels[0], labels[4] = 0, V          # PAD; a label outside the vocabulary
    adv = np.array([-0.8, 0.0, 1.3])
    scale = 1.0 / N
    lp, ent, g = R.policy_xent(x, labels, adv, N, scale, beta)
    assert lp[0] == 0 and ent[0] == 0 and (g[0] == 0).all() and (g[4] == 0).all()
    assert (lp[labels > 0][:3] < 0).all()
    h = 1e-6
    fd = np.zeros_like(x)
    for r in range(T * N):
        for v in range(V):
            xp, xm = x.copy(), x.copy()
            xp[r, v] += h
            xm[r, v] -= h
            fd[r, v] = (R.policy_J(xp, labels, adv, N, scale, beta) - R.policy_J(xm, labels, adv, N, scale, beta)) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-9)
    if beta == 0:   # the rows of the zero-advantage caption (n = 1) carry no gradient without the entropy term
        assert (g[1::N] == 0).all()
    else:
        assert np.abs(g[1::N][labels[1::N] != V]).max() > 0


def test_reference_entropy_and_underflow():
    x = np.zeros((2, 11))
    x[1, 4] = 800.0                      # every other probability underflows to 0 in float64
    lp, ent, g = R.policy_xent(x, np.array([3, 4]), np.array([1.0]), 1, 1.0, 0.5)
    assert ent[0] == pytest.approx(np.log(11)) and lp[0] == pytest.approx(-np.log(11))
    assert ent[1] == 0.0 and lp[1] == 0.0 and np.isfinite(g).all() and (g[1] == 0).all()


def test_policy_cases_hold_their_plants():
    for V, ld, off, T, N in R.POLICY_SHAPES:
        buf, labels, adv, plants = R.policy_case(V, ld, off, T, N)
        assert buf.shape == (T * N, ld) and (buf[:, V:] == 777.0).all() and adv.shape == (N,)
        if plants:
            assert labels[plants["pad"]] == 0 and labels[plants["last"]] == V - 1 and labels[plants["first"]] == 1
            lp, ent, g = R.policy_xent(buf[:, :V], labels, adv, N, 1.0 / N, 0.25)
            assert ent[plants["equal"]] == pytest.approx(np.log(V)) and 0 <= ent[plants["spike"]] < 1e-6
        else:
            assert labels.tolist() == [1023, 1024]
    assert any(a < 0 for a in R.policy_case(203, 204, 0, 3, 3)[2]) and 0.0 in R.policy_case(203, 204, 0, 3, 3)[2]


# ------------------------------------------------------------------------------------------------ advantages, policy batch
def test_average_advantages():
    rng = np.random.default_rng(5)
    r = rng.random((6, 5))
    a = scst.advantages(r, "average")
    assert a.dtype == np.float64 and a.shape == r.shape
    np.testing.assert_allclose(a.sum(1), 0.0, atol=1e-14)
    for b in range(6):
        for k in range(5):
            assert a[b, k] == pytest.approx(r[b, k] - np.delete(r[b], k).mean(), abs=1e-14)
    assert (scst.advantages(np.full((3, 4), 0.37), "average") == 0).all()
    with pytest.raises(ValueError, match="num_captions >= 2"):
        scst.advantages(r[:, :1], "average")
    with pytest.raises(ValueError):
        scst.advantages(r, "median")


def test_greedy_advantages():
    r = np.random.default_rng(6).random((4, 3))
    assert (scst.advantages(r, "greedy", r) == 0).all()
    g = r[:, ::-1]
    np.testing.assert_array_equal(scst.advantages(r, "greedy", g), r - g)
    assert scst.advantages(r[:, :1], "greedy", g[:, :1]).shape == (4, 1)    # one sample per image is fine here
    with pytest.raises(ValueError):
        scst.advantages(r, "greedy")
    with pytest.raises(ValueError):
        scst.advantages(r, "greedy", g[:, :2])


def test_policy_batch_layout():
    samples = [[5, 6, 7, EOS], [EOS], [8, 9, 10, 11, 12]]          # ended, empty, cut without <EOS>
    b = scst.policy_batch(samples, BOS, EOS)
    np.testing.assert_array_equal(b["lengths"], [4, 1, 5])
    np.testing.assert_array_equal(b["cap_enc"], [[5, 6, 7, EOS, 0], [EOS, 0, 0, 0, 0], [8, 9, 10, 11, 12]])
    np.testing.assert_array_equal(b["cap_dec"], [[BOS, 5, 6, 7, 0], [BOS, 0, 0, 0, 0], [BOS, 8, 9, 10, 11]])
    _, dec, enc, lens = R.sample_case(np.random.default_rng(2), 12, 6, 50)
    s, _, _, _ = R.sample_case(np.random.default_rng(2), 12, 6, 50)
    b = scst.policy_batch(s, BOS, EOS)
    np.testing.assert_array_equal(b["cap_dec"], dec)
    np.testing.assert_array_equal(b["cap_enc"], enc)
    np.testing.assert_array_equal(b["lengths"], lens)
    with pytest.raises(ValueError):
        scst.policy_batch([[5], []], BOS, EOS)
    b = scst.policy_batch([[5, 0, 6]], BOS, EOS)      # a sampled id 0 stays where it is: fed to the decoder, masked as a label
    np.testing.assert_array_equal(b["cap_enc"], [[5, 0, 6]])
    np.testing.assert_array_equal(b["cap_dec"], [[BOS, 5, 0]])


def test_batch_references_are_the_images_own_rows():
    enc = np.array([[5, 6, EOS, 0], [7, EOS, 0, 0], [0, 0, 0, 0], [8, 9, 10, EOS], [0, 0, 0, 0], [0, 0, 0, 0]], np.int32)
    lens = np.array([3, 2, 0, 4, 0, 0])
    assert scst.batch_references(enc, lens, 2) == [[[5, 6, EOS], [7, EOS]], [[8, 9, 10, EOS]], [[]]]


# ------------------------------------------------------------------------------------------------ flags
def test_defaults_and_flags():
    p = Parameters().parse_args([])
    for k, v in NEW_DEFAULTS.items():
        assert getattr(p, k) == v
    p = Parameters().parse_args("--scst --restore --scst_baseline greedy --scst_entropy 0.01".split())
    assert p.scst is True and p.scst_baseline == "greedy" and p.scst_entropy == 0.01
    p = Parameters()
    p.num_captions = 1
    assert p.parse_args("--scst --scst_baseline greedy".split()).scst_baseline == "greedy"


@pytest.mark.parametrize("argv", [
    "--scst --fine_tune", "--scst --mode inference", "--scst --temperature 0.7", "--scst --top_k 5", "--scst --top_p 0.9",
    "--scst --kl_free_bits 0.05", "--scst --kl_weight 0.5", "--scst --kl_cycle_steps 10", "--scst --kl_cycle_ramp 0.3", "--scst --kl_cycles 2",
    "--scst --label_smoothing 0.1", "--scst --word_drop 0.2",
    "--scst --scst_entropy -0.1", "--scst --scst_entropy inf", "--scst --scst_entropy nan", "--scst --scst_baseline median",
    "--scst_baseline greedy", "--scst_entropy 0.1",
], ids=lambda a: a.replace(" ", "_"))
def test_parse_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        Parameters().parse_args(argv.split())
    assert e.value.code == 2
    assert "--" in capsys.readouterr().err


def test_average_baseline_needs_two_captions(capsys):
    p = Parameters()
    p.num_captions = 1
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--scst"])
    assert e.value.code == 2 and "num_captions" in capsys.readouterr().err


def test_old_parameters_pickle_loads_with_the_defaults():
    """a Parameters pickled before the flags existed has none of the attributes in its instance dict"""
    p = Parameters()
    p.prior, p.latent_size = "AG", 99
    assert not any(k in vars(p) for k in NEW_DEFAULTS)
    q = pickle.loads(pickle.dumps(p))
    assert q.prior == "AG" and q.latent_size == 99
    for k, v in NEW_DEFAULTS.items():
        assert getattr(q, k) == v, k


# ------------------------------------------------------------------------------------------------ document frequencies
def _caps(rng, n, vocab, lo=1, hi=9):
    return [[BOS] + rng.integers(3, vocab, size=rng.integers(lo, hi + 1)).tolist() + [EOS] for _ in range(n)]


def test_corpus_document_frequencies_give_the_reference_cider_d():
    """scst.corpus_df (what CiderReward uploads) against consensus_ref.df_idf on the same corpus, and the float64 CIDEr-D computed with
    either table: equal scores, and equal to eval_ref.cider_scores when the corpus IS the reference set"""
    rng = np.random.default_rng(17)
    vocab = 25
    corpus = [_caps(rng, 3, vocab) for _ in range(40)]
    keys, idf, unseen = scst.corpus_df(corpus, BOS, EOS, vocab)
    want, want_unseen = cref.df_idf(corpus, BOS, EOS)
    assert unseen == pytest.approx(float(want_unseen), rel=1e-7) and keys.size == len(want)
    assert (np.diff(keys.astype(np.uint64)) > 0).all()
    table = {int(k): np.float32(v) for k, v in zip(keys, idf)}
    for k, v in want.items():
        assert table[k] == pytest.approx(float(v), rel=1e-6, abs=1e-7), k
    refs = corpus[:6]
    cands = [_caps(rng, 4, vocab) for _ in range(6)]
    cands[0][0] = [BOS, EOS]                       # an empty candidate: reward 0
    same = [BOS, 3, 4, 5, 6, 7, 8, EOS]            # (four words or more: every n-gram order is present, a self-match scores 10)
    cands[1] = [list(same)] * 4
    refs = [list(r) for r in refs]
    refs[1] = [list(same)] * 3                     # an image whose references all equal the candidate
    a = R.cider_rewards(cands, refs, corpus, BOS, EOS, idf=table, unseen=np.float32(unseen))
    b = R.cider_rewards(cands, refs, corpus, BOS, EOS)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-12)
    assert a[0][0] == 0.0 and a[1][0] == pytest.approx(10.0, rel=1e-6) and a[1][0] >= max(map(np.max, a))
    own = R.cider_rewards(cands, refs, refs, BOS, EOS)
    for x, y in zip(own, eval_ref.cider_scores(cands, refs, BOS, EOS)):
        np.testing.assert_array_equal(x, y)
