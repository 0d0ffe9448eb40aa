"""-m gpu: ROUGE-L (csrc/lcs.hip, vae_captioning_amd/evaluate.py, scst.py).  vc_lcs_overlap against the plain-Python reference of
tests/rouge_ref.py with exact equality of its three integer outputs -- at every length around the word size of its bit-parallel
recurrence, in every range form, at the launch edges, independent of the launch, inside its output arrays; CaptionEvaluator.evaluate
end to end; RougeReward and SumReward; one self-critical step on the summed reward; and the command line."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from vae_captioning_amd import scst, spec, synth
from vae_captioning_amd import evaluate as ev
from vae_captioning_amd.abi import VaecapError
from vae_captioning_amd.consensus import word_rows
from vae_captioning_amd.evaluate import METRICS, CaptionEvaluator
from vae_captioning_amd.trainer import Trainer

from . import rouge_ref as ref
from . import scst_ref
from .gpu_util import P, dev, host, stream
from .test_gpu_engine import small_params
from .test_gpu_eval import _caps, _related

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -559038737   # what an output array holds before a launch, and a guard word always
NEW_KEYS = ("rouge_l", "oracle_rouge_l", "mean_rouge_l")


def _launch(lib, c_tok, c_len, r_tok, r_len, lo, hi, skip, C=None):
    """vc_lcs_overlap through the C ABI on host arrays -> int32 [C, 3] (lcs_max, rec_lcs, rec_len); every output starts as GUARD"""
    c_tok, r_tok = np.asarray(c_tok, np.int32), np.asarray(r_tok, np.int32)
    C = c_tok.shape[0] if C is None else C
    out = torch.full((3, max(C, 1)), GUARD, dtype=torch.int32, device="cuda")
    lib.vc_lcs_overlap(stream(), C, P(dev(c_tok)), c_tok.shape[1], P(dev(c_len, np.int32)), r_tok.shape[0], P(dev(r_tok)), r_tok.shape[1],
                       P(dev(r_len, np.int32)), P(dev(lo, np.int32)), P(dev(hi, np.int32)), P(dev(skip, np.int32)), P(out[0]), P(out[1]),
                       P(out[2]))
    return host(out)[:, :C].T


def _rows(seqs, ld, poison):
    """word lists -> (tok [n, ld], len [n]); the entries at and past len hold poison[i] ids, cycled (never 0: PAD would not match)"""
    tok, lens = np.zeros((len(seqs), ld), np.int32), np.array([len(s) for s in seqs], np.int32)
    for i, s in enumerate(seqs):
        tok[i, :len(s)] = s
        fill = list(poison[i]) or list(s) or [7]
        tok[i, len(s):] = [fill[j % len(fill)] for j in range(ld - len(s))]
    return tok, lens


def _want(cw, rw, lo, hi, skip):
    return np.array(ref.overlap(cw, rw, list(lo), list(hi), list(skip)), np.int32).reshape(len(cw), 3)


def _assert_rows(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.shape == want.shape and bad.size == 0, (what, "row %d: got %s want %s" % (bad[0], got[bad[0]], want[bad[0]]))


# ------------------------------------------------------------------ lengths
HYP_LENS, REF_LENS = (0, 1, 2, 31, 32, 33, 63, 64), (0, 1, 5, 63, 64)


def _length_pairs():
    rng = np.random.default_rng(64)
    cw, rw = [], []
    for vocab in (2, 50):
        for a in HYP_LENS:
            for b in REF_LENS:
                cw.append(rng.integers(3, 3 + vocab, size=a).tolist())
                rw.append(rng.integers(3, 3 + vocab, size=b).tolist())
    cw += [[9] * 64, [9] * 64]          # an all-equal 64-word row against itself and against three of the same word
    rw += [[9] * 64, [9] * 3]
    return cw, rw


@pytest.mark.parametrize("ld", [64, 67])
def test_every_length_pair_through_width_one_ranges(lib, ld):
    """80 + 2 (hypothesis, reference) pairs, pair i = hypothesis row i against the range [i, i + 1): lcs_max = rec_lcs = the LCS of the
    pair and rec_len = the reference's words (0, 0, 0 against a reference without words), bit for bit against the DP.  The entries at and
    past len hold words of the OTHER row of the pair: a kernel that read them, or let a padding lane into a match mask, would find a
    longer subsequence.  A small vocabulary gives long LCS (repeated words), 64 words on both sides exercise the dropped carry."""
    cw, rw = _length_pairs()
    n = len(cw)
    c_tok, c_len = _rows(cw, ld, rw)
    r_tok, r_len = _rows(rw, ld, cw)
    lo = np.arange(n)
    got = _launch(lib, c_tok, c_len, r_tok, r_len, lo, lo + 1, np.full(n, -1))
    want = _want(cw, rw, lo, lo + 1, np.full(n, -1))
    pair = np.array([[ref.lcs(a, b)] * 2 + [len(b)] if b else [0, 0, 0] for a, b in zip(cw, rw)], np.int32)
    assert np.array_equal(want, pair)
    _assert_rows(got, want, "ld %d" % ld)
    assert got[-2].tolist() == [64, 64, 64] and got[-1].tolist() == [3, 3, 3]
    assert (want[:, 0] >= 30).sum() >= 8 and (want[:, 0] == 0).sum() >= 16


# ------------------------------------------------------------------ ranges
def _range_case():
    rng = np.random.default_rng(77)
    rw = [rng.integers(3, 12, size=rng.integers(1, 17)).tolist() for _ in range(320)]
    for r in (40, 41, 42, 43):
        rw[r] = []                                   # a stretch of rows without words
    rw[50] = [1, 65535, 1, 1, 65535]                 # the smallest and the largest id
    rw[319] = [65535] * 64
    cw = [rng.integers(3, 12, size=rng.integers(1, 17)).tolist() for _ in range(14)]
    cw[5], cw[6] = [65535, 1, 1, 4], []
    lo = [0, 320, 7, 7, 7, 50, 50, 40, 10, 319, 12, 30, 44, 0]
    hi = [0, 320, 12, 12, 8, 51, 51, 44, 310, 320, 13, 60, 45, 320]
    skip = [-1, -1, 9, 100, 7, -1, -1, -1, 200, -1, -1, 41, 44, 319]
    return cw, rw, np.array(lo), np.array(hi), np.array(skip)


def test_ranges_skips_and_rows_without_words(lib):
    """through evaluate.lcs_overlap on word tables: lo == hi at both ends of the table; a skip inside the range, outside it and equal to
    the only row; a range of rows without words (and a larger one that holds them); 300 rows (no limit per range); ids 1 and 65535"""
    cw, rw, lo, hi, skip = _range_case()
    d = torch.device("cuda", torch.cuda.current_device())
    (Wc, Lc), (Wr, Lr) = _rows(cw, 16, [[5]] * len(cw)), _rows(rw, 64, [[5]] * len(rw))
    hyp, table = ev.word_table(d, Wc, Lc), ev.word_table(d, Wr, Lr)
    o = ev.lcs_overlap(lib, hyp, table, lo, hi, skip)
    assert set(o) == {"lcs_max", "rec_lcs", "rec_len"} and all(o[k].dtype == np.int32 and o[k].shape == (14,) for k in o)
    got = np.stack([o["lcs_max"], o["rec_lcs"], o["rec_len"]], axis=1)
    want = _want(cw, rw, lo, hi, skip)
    _assert_rows(got, want, "ranges")
    for c in (0, 1, 4, 7, 12):                       # empty, empty, emptied by the skip, rows without words, emptied by the skip
        assert got[c].tolist() == [0, 0, 0], c
    assert got[5].tolist() == [3, 3, 5] and got[6].tolist() == [0, 0, 5] and got[9].tolist()[2] == 64
    assert got[8][0] >= 8 and got[13][1] == got[13][2] > 0     # 300 rows: some row holds most of the hypothesis
    none = ev.lcs_overlap(lib, hyp, table, lo, hi)            # skip=None: nothing skipped
    assert none["rec_len"][4] == len(rw[7]) and none["lcs_max"][12] == ref.lcs(cw[12], rw[44])
    # past the host check, what the library documents for a bad range: clamped into the table, lo > hi empty
    blo = np.array([-5, 7, 3, 320, 400, 0, 2, 2, 2, 0, 0, 0, 0, 0], np.int32)
    bhi = np.array([500, 3, 3, 999, 500, -3, 11, 2, 1, 1, 1, 1, 1, 1], np.int32)
    got = _launch(lib, Wc, Lc, Wr, Lr, blo, bhi, np.full(14, -1))
    clo = np.clip(blo, 0, 320)
    _assert_rows(got, _want(cw, rw, clo, np.clip(np.maximum(bhi, clo), 0, 320), np.full(14, -1)), "clamp")


# ------------------------------------------------------------------ launch edges, independence, guards
def _mixed(rng, n_hyp, n_ref, vocab=6):
    cw = [rng.integers(3, 3 + vocab, size=rng.integers(0, 21)).tolist() for _ in range(n_hyp)]
    rw = [rng.integers(3, 3 + vocab, size=rng.integers(0, 21)).tolist() for _ in range(n_ref)]
    lo = rng.integers(0, n_ref - 6, size=n_hyp)
    hi = lo + rng.integers(0, 7, size=n_hyp)
    skip = np.where(rng.random(n_hyp) < 0.3, lo + 1, -1)
    return cw, rw, lo, hi, skip


@pytest.mark.parametrize("C", [0, 1, 3, 4, 5, 9])
def test_launch_edges_with_four_hypotheses_per_workgroup(lib, C):
    """part of a workgroup, exactly one, one more, two and a quarter; the rows past C stay as they were; C = 0 is a no-op"""
    cw, rw, lo, hi, skip = _mixed(np.random.default_rng(5), 12, 30)
    (Wc, Lc), (Wr, Lr) = _rows(cw, 24, [[4]] * 12), _rows(rw, 21, [[4]] * 30)
    full = torch.full((3, 12), GUARD, dtype=torch.int32, device="cuda")
    lib.vc_lcs_overlap(stream(), C, P(dev(Wc)), 24, P(dev(Lc)), 30, P(dev(Wr)), 21, P(dev(Lr)), P(dev(lo, np.int32)), P(dev(hi, np.int32)),
                       P(dev(skip, np.int32)), P(full[0]), P(full[1]), P(full[2]))
    got = host(full).T
    _assert_rows(got[:C], _want(cw[:C], rw, lo[:C], hi[:C], skip[:C]), "C %d" % C)
    assert (got[C:] == GUARD).all()
    if C == 0:
        lib.vc_lcs_overlap(stream(), 0, None, 24, None, 30, None, 21, None, None, None, None, None, None, None)
        d = torch.device("cuda", torch.cuda.current_device())
        empty = ev.lcs_overlap(lib, ev.word_table(d, Wc[:0], Lc[:0]), ev.word_table(d, Wr, Lr), [], [])
        assert all(empty[k].shape == (0,) for k in ("lcs_max", "rec_lcs", "rec_len"))


def test_rows_do_not_depend_on_the_launch(lib):
    """the same 40 rows launched alone, in reversed order, and as rows 480..519 of a launch of C = 1000: bit-identical outputs"""
    rng = np.random.default_rng(31)
    cw, rw, lo, hi, skip = _mixed(rng, 1000, 200)
    (Wc, Lc), (Wr, Lr) = _rows(cw, 20, [[5]] * 1000), _rows(rw, 20, [[5]] * 200)
    big = _launch(lib, Wc, Lc, Wr, Lr, lo, hi, skip)
    s = slice(480, 520)
    alone = _launch(lib, Wc[s], Lc[s], Wr, Lr, lo[s], hi[s], skip[s])
    back = _launch(lib, Wc[s][::-1], Lc[s][::-1], Wr, Lr, lo[s][::-1], hi[s][::-1], skip[s][::-1])
    assert np.array_equal(alone, big[s]) and np.array_equal(back[::-1], alone)
    assert np.array_equal(_launch(lib, Wc, Lc, Wr, Lr, lo, hi, skip), big)
    _assert_rows(alone, _want(cw[s], rw, lo[s], hi[s], skip[s]), "alone")
    assert (alone[:, 0] > 0).sum() >= 20 and (big != GUARD).all()


def test_outputs_stay_inside_their_arrays(lib):
    """the three outputs in one allocation, guard words between and behind them: C = 9 values each, nothing else written"""
    cw, rw, lo, hi, skip = _mixed(np.random.default_rng(6), 9, 30)
    (Wc, Lc), (Wr, Lr) = _rows(cw, 20, [[4]] * 9), _rows(rw, 20, [[4]] * 30)
    G, C = 64, 9
    buf = torch.full((G + C + G + C + G + C + G,), GUARD, dtype=torch.int32, device="cuda")
    o = [G, G + C + G, G + 2 * (C + G)]
    lib.vc_lcs_overlap(stream(), C, P(dev(Wc)), 20, P(dev(Lc)), 30, P(dev(Wr)), 20, P(dev(Lr)), P(dev(lo, np.int32)), P(dev(hi, np.int32)),
                       P(dev(skip, np.int32)), P(buf) + 4 * o[0], P(buf) + 4 * o[1], P(buf) + 4 * o[2])
    b = host(buf)
    got = np.stack([b[x:x + C] for x in o], axis=1)
    _assert_rows(got, _want(cw, rw, lo, hi, skip), "guards")
    keep = np.ones(b.size, bool)
    for x in o:
        keep[x:x + C] = False
    assert (b[keep] == GUARD).all() and keep.sum() == 4 * G


def test_bad_arguments(lib):
    d = torch.device("cuda", torch.cuda.current_device())
    (Wc, Lc), (Wr, Lr) = _rows([[4, 5], [5]], 4, [[3]] * 2), _rows([[3], [4, 5], [5]], 4, [[3]] * 3)
    hyp, table = ev.word_table(d, Wc, Lc), ev.word_table(d, Wr, Lr)
    with pytest.raises(ValueError, match="row 1: range"):
        ev.lcs_overlap(lib, hyp, table, [0, 2], [3, 1])
    with pytest.raises(ValueError, match="row 0: range"):
        ev.lcs_overlap(lib, hyp, table, [0, 0], [4, 3])
    with pytest.raises(ValueError, match="one entry per hypothesis"):
        ev.lcs_overlap(lib, hyp, table, [0], [3])
    out = torch.zeros(6, dtype=torch.int32, device="cuda")
    rg = dev(np.array([0, 0, 3, 3, -1, -1], np.int32))
    call = lambda C=2, c_ld=4, n_ref=3, r_ld=4, tok=P(hyp.tok): lib.vc_lcs_overlap(
        stream(), C, tok, c_ld, P(hyp.len), n_ref, P(table.tok), r_ld, P(table.len), P(rg), P(rg) + 8, P(rg) + 16, P(out), P(out) + 8,
        P(out) + 16)
    for bad in (dict(c_ld=0), dict(r_ld=0), dict(C=-1), dict(n_ref=-1), dict(tok=None)):
        with pytest.raises(VaecapError, match="invalid argument"):
            call(**bad)
    call()
    # "4 5" against 3 | 4 5 | 5: the largest LCS is 2; 2 of 2 words and 1 of 1 tie, the shorter row wins.  "5": 1 of 2 loses to 1 of 1
    assert host(out).tolist() == [2, 1, 1, 1, 1, 1]


# ------------------------------------------------------------------ the evaluator
@pytest.fixture(scope="module")
def e2e():
    rng = np.random.default_rng(44)
    cands, refs = _related(rng, 12, 20, 5, 30)
    cands[4], cands[9] = [], cands[9][:1]
    return cands, refs, ref.evaluate_rouge(cands, refs, BOS, EOS)


def test_evaluate_end_to_end_against_the_reference(lib, e2e, monkeypatch):
    """12 images x 20 captions x 5 references, vocabulary 30; image 4 lists nothing and image 9 one caption.  The three integers per
    caption are exact and both sides apply one float64 formula to them: 1e-12 relative.  With the LCS launch patched out every other
    number is what it was, to the bit."""
    cands, refs, (want_top, want_best, want_mean, want_caps) = e2e
    assert 0 < want_top < want_best < 1 and 0 < want_mean < want_best            # (the data make the ordering strict)
    evaluator = CaptionEvaluator(lib, refs, BOS, EOS, vocab_size=30)
    res = evaluator.evaluate(cands)
    assert set(res) == set(METRICS) | {"per_image"}
    for k, w in zip(NEW_KEYS, (want_top, want_best, want_mean)):
        assert isinstance(res[k], float), k
        np.testing.assert_allclose(res[k], w, rtol=1e-12, atol=0, err_msg=k)
    per = res["per_image"]
    for b in range(12):
        np.testing.assert_allclose(per["caption_rouge_l"][b], want_caps[b], rtol=1e-12, atol=0, err_msg="image %d" % b)
    assert per["caption_rouge_l"][4].shape == (0,) and np.isnan(per["rouge_l"][4]) and np.isnan(per["oracle_rouge_l"][4])
    assert per["rouge_l"][9] == per["oracle_rouge_l"][9] == per["caption_rouge_l"][9][0]
    np.testing.assert_allclose(np.delete(per["oracle_rouge_l"], 4), [w.max() for w in want_caps if len(w)], rtol=1e-12, atol=0)
    assert 0 < res["rouge_l"] < res["oracle_rouge_l"] < 1
    # the old numbers did not move
    launched = []

    def no_launch(lib_, hyp, table, rng, out):
        launched.append(hyp.n)
        out.zero_()
    monkeypatch.setattr(ev, "_launch_lcs", no_launch)
    old = evaluator.evaluate(cands)
    assert launched == [201] and old["rouge_l"] == old["oracle_rouge_l"] == old["mean_rouge_l"] == 0.0
    for k in METRICS[:12]:
        assert old[k] == res[k], k
    for k in ("captions", "cider_d", "oracle_cider_d", "distinct", "div_1", "div_2"):
        np.testing.assert_array_equal(old["per_image"][k], per[k], err_msg=k)
    for a, b in zip(old["per_image"]["caption_cider_d"], per["caption_cider_d"]):
        assert np.array_equal(a, b)
    monkeypatch.undo()
    # lists of one: the three numbers are one number
    one = CaptionEvaluator(lib, refs, BOS, EOS).evaluate([cs[:1] for cs in cands])
    assert one["rouge_l"] == one["oracle_rouge_l"] == one["mean_rouge_l"] > 0
    np.testing.assert_allclose(one["rouge_l"], np.mean([w[0] for w in want_caps if len(w)]), rtol=1e-12, atol=0)
    nothing = CaptionEvaluator(lib, refs, BOS, EOS).evaluate([[] for _ in cands])
    assert nothing["rouge_l"] == nothing["oracle_rouge_l"] == nothing["mean_rouge_l"] == 0.0


# ------------------------------------------------------------------ the rewards
@pytest.fixture(scope="module")
def reward_case():
    rng = np.random.default_rng(52)
    V = 30
    corpus = [[[BOS] + rng.integers(3, V, size=rng.integers(4, 9)).tolist() + [EOS] for _ in range(3)] for _ in range(40)]
    refs = [[list(r) for r in c[:2]] for c in corpus[:6]]
    cands = [[[BOS] + rng.permutation(r[0][1:-1]).tolist()[:rng.integers(2, 9)] + [EOS] for _ in range(2)] + [list(r[1])] for r in refs]
    cands[0][0] = [EOS]                                  # a candidate without words
    refs[2][1] = [BOS, EOS]                              # an image with one empty reference
    cider = np.concatenate(scst_ref.cider_rewards(cands, refs, corpus, BOS, EOS))
    rouge = np.concatenate(ref.scores(cands, refs, BOS, EOS))
    return V, corpus, cands, refs, cider, rouge


def test_rouge_reward_matches_the_reference(lib, reward_case):
    V, corpus, cands, refs, _, rouge = reward_case
    rw = scst.RougeReward(lib, BOS, EOS)
    got = rw.rewards(cands, refs)
    assert got.dtype == np.float64 and got.shape == rouge.shape == (18,)
    np.testing.assert_allclose(got, rouge, rtol=1e-12, atol=0)
    assert got[0] == 0.0 and got[2] == 1.0 and 0 < got[1] < 1 and rw.host_seconds > 0
    # the empty reference takes no part: the image's other one decides
    assert (got[6:8] > 0).all() and np.array_equal(got[6:9], rw.rewards([cands[2]], [refs[2][:1]]))
    assert rw.rewards([[] for _ in refs], refs).shape == (0,)
    with pytest.raises(ValueError, match="images of candidates"):
        rw.rewards(cands, refs[:3])
    with pytest.raises(ValueError, match="image 1 has no reference caption"):
        rw.rewards(cands[:2], [refs[0], []])
    with pytest.raises(ValueError, match="candidate row 1 has 65 words"):
        rw.rewards([[[3], [4] * 65]], [refs[0]])


def test_sum_reward_is_cider_plus_half_rouge(lib, reward_case):
    """rtol 1e-5, atol 1e-6: what tests/test_gpu_scst.py holds CiderReward to -- the CIDEr-D half (f32 on the device) carries it"""
    V, corpus, cands, refs, cider, rouge = reward_case
    c, r = scst.CiderReward(lib, corpus, BOS, EOS, V), scst.RougeReward(lib, BOS, EOS)
    s = scst.SumReward([(c, 1), (r, 0.5)])
    assert s.shared                                      # one conversion of the token lists for both parts
    got = s.rewards(cands, refs)
    assert got.dtype == np.float64 and got.shape == (18,)
    np.testing.assert_allclose(got, cider + 0.5 * rouge, rtol=1e-5, atol=1e-6)
    assert np.array_equal(got, c.rewards(cands, refs) + 0.5 * r.rewards(cands, refs))     # shared rows or not: the same numbers
    assert got[0] == 0.0 and s.host_seconds > 0 and s.rewards([[] for _ in refs], refs).shape == (0,)


def test_one_self_critical_step_on_the_summed_reward(lib):
    """the step's reported reward is the mean summed reward of the captions it sampled (the sampler re-run on the same injected
    draws before the step), and the step moves the decoder"""
    p = small_params(prior="Normal")
    V, B, T, K, max_len = 203, 4, 6, p.num_captions, 8
    rng = np.random.default_rng(11)
    batch = synth.make_batch(rng, B, K, T, V, use_ci=False, variable_len=True, feature_size=p.cnn_feature_size)
    tr = Trainer(p, V, lib=lib, seed=3)
    P0 = spec.init_caption_params(p, V, seed=8)
    tr.load_state_dict(P0)
    corpus = [[[BOS] + rng.integers(3, V, size=rng.integers(4, 9)).tolist() + [EOS] for _ in range(3)] for _ in range(20)]
    reward = scst.SumReward([(scst.CiderReward(tr.cap, corpus, BOS, EOS, V), 1.0), (scst.RougeReward(tr.cap, BOS, EOS), 0.5)])
    tr.enable_scst(reward, BOS, EOS, baseline="average", beta=0.0, max_len=max_len)
    tr.cap.store.param("decoder/rnn_logits/bias")[EOS] += 3.0
    tr.cap.store.param("decoder/rnn_logits/bias")[0] -= 30.0
    before = tr.state_dict()
    eps = rng.standard_normal((K, p.gen_z_samples, B, p.latent_size)).astype(np.float32)
    uniforms = rng.random((K, max_len, B)).astype(np.float32)
    cands, _ = tr.scst_sample(batch, "sample", eps, uniforms)
    lists = [[list(c[0]) for c in cs] for cs in cands]
    refs = scst.batch_references(batch["cap_enc"], batch["lengths"], K)
    want = reward.rewards(lists, refs)
    rouge = np.concatenate(ref.scores(lists, refs, BOS, EOS))
    assert want.shape == (B * K,) and (rouge > 0).any()
    np.testing.assert_allclose(want - reward.parts[0][0].rewards(lists, refs), 0.5 * rouge, rtol=1e-9, atol=1e-12)
    st = tr.scst_step(batch, eps=eps, uniforms=uniforms)
    np.testing.assert_allclose(st["reward"], want.mean(), rtol=1e-12, atol=0)
    after = tr.state_dict()
    assert any(not np.array_equal(after[k], before[k]) for k in after if k.startswith("decoder/"))


# ------------------------------------------------------------------ the command line
SMALL = ["--synthetic", "--vocab", "200", "--embed_dim", "32", "--enc_hid", "64", "--dec_hid", "64", "--latent", "10", "--gen_z_samples", "4",
         "--bs", "4", "--ckpt_format", "npz"]


def _main(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=cwd, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_main_inference_with_eval_captions_reports_rouge_l(tmp_path):
    _main(SMALL + ["--epochs", "1", "--max_steps", "1"], tmp_path)
    out = _main(SMALL + ["--mode", "inference", "--sample_gen", "diverse", "--diverse_draws", "4", "--eval_captions"], tmp_path)
    m = json.load(open(tmp_path / "val_00_metrics.json"))
    assert set(METRICS) <= set(m)
    for k in NEW_KEYS:
        assert 0.0 <= m[k] <= 1.0, k
        assert len(re.findall(r"^%s: \d+\.\d{6}$" % k, out, flags=re.M)) == 1, k
    assert m["rouge_l"] <= m["oracle_rouge_l"] and m["mean_rouge_l"] <= m["oracle_rouge_l"]


def test_main_scst_with_and_without_the_rouge_weight(tmp_path):
    base = SMALL + ["--checkpoint", "rougetest", "--epochs", "1", "--max_steps", "1"]
    _main(base, tmp_path)
    start = r"^SCST: document frequencies from \d+ training images, baseline average, entropy weight 0%s$"
    out = _main(base + ["--scst", "--restore", "--scst_rouge", "0.5"], tmp_path)
    assert len(re.findall(start % ", ROUGE-L weight 0.5", out, flags=re.M)) == 1, out
    line = [l for l in out.splitlines() if "SCST: reward:" in l]
    assert line and all(k in line[-1] for k in ("baseline:", "sample_len:", "entropy:")) and "Model saved" in out
    out = _main(base + ["--scst", "--restore"], tmp_path)
    assert len(re.findall(start % "", out, flags=re.M)) == 1 and "ROUGE" not in out, out
