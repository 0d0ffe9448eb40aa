"""-m gpu: in-set CIDEr-D (csrc/cider_gram.hip, csrc/cider_pair.h, vae_captioning_amd/mbr.py).  vc_cider_gram bit for bit against
vc_consensus_score (the shared pair function) and within test_gpu_consensus.py's bound of the float64 reference of tests/gram_ref.py,
at the group-of-four and wave boundaries and at the 256-caption limit; its float64 weighted means; its independence of the launch, the
chunking and the row's place; its argument checks; CaptionEvaluator.evaluate(self_cider=True); the decoder's mbr mode; the command
line."""
import json
import math
import re

import numpy as np
import pytest
import torch

from vae_captioning_amd import mbr
from vae_captioning_amd.abi import VaecapError
from vae_captioning_amd.consensus import ngram_vectors, word_rows
from vae_captioning_amd.evaluate import METRICS, SET_METRICS, CaptionEvaluator

from . import consensus_ref as cref
from . import gram_ref as ref
from .gpu_util import P, dev, host, stream
from .test_gpu_consensus import _Dict, _facade_params
from .test_gpu_eval import _caps, _related
from .test_gpu_rouge import SMALL, _main

pytestmark = pytest.mark.gpu
BOS, EOS = 1, 2
PER = (0, 1, 2, 4, 5, 64, 65, 256)     # captions per image: the group-of-four and wave boundaries, and the limit
CANARY = -7777.0
LD = 264                               # > 256: every row has columns that must stay untouched
RTOL, ATOL = 1e-5, 1e-6                # tests/test_gpu_consensus.py's bound for the same f32 arithmetic
# CaptionEvaluator.evaluate(self_cider=True) against the float64 reference: 4 x the largest deviation measured over this file's
# evaluator case, capped at 1e-4 -- tests/test_gpu_bound.py's rule.  MEASURED: the deviations seen on the MI355X.
MEASURED = dict(self_cider=4.7e-10, mbr_cider_d=1.1e-7, image_self_cider=7.9e-9)
SET_BOUND = {k: min(4 * d, 1e-4) for k, d in MEASURED.items()}
E2E_SEED = 45


def _variants(rng, base, n, lo, hi, swap=0.25, vocab=30):
    out = []
    for _ in range(n):
        c = np.where(rng.random(base.size) < swap, rng.integers(3, vocab, size=base.size), base)[:rng.integers(lo, hi + 1)]
        out.append([BOS] + c.tolist() + [EOS])
    return out


@pytest.fixture(scope="module")
def case():
    """corpus (the idf), the eight images, the reference table (idf, unseen) and the float64 matrices of the images up to 65 captions"""
    rng = np.random.default_rng(7)
    corpus = [_caps(rng, 3, 30, 3, 10) for _ in range(40)]
    imgs = []
    for n in PER:
        if n == 256:
            imgs.append(_variants(rng, rng.integers(3, 30, size=6), n, 1, 6))          # at most 6 words per caption
        else:
            imgs.append(_variants(rng, rng.integers(3, 30, size=16), n, 6, 16))
    imgs[3][0], imgs[3][1] = [BOS, EOS], [BOS, 5, EOS]                                  # 0 words, 1 word
    imgs[4][0] = [BOS, 3, 4, 5, EOS]                                                   # 3 words
    imgs[5][0] = [BOS] + rng.integers(3, 30, size=64).tolist() + [EOS]                 # 64 words
    imgs[5][1] = [BOS, 65535, 4, 65535, 65535, 7, EOS]                                 # the largest id
    imgs[5][2] = list(imgs[5][0][:60]) + [EOS]                                         # shares long n-grams with the 64-word row
    imgs[4][3] = list(imgs[4][2])                                                      # duplicates in two images
    imgs[6][10] = list(imgs[6][20])
    idf, unseen = cref.df_idf(corpus, BOS, EOS)
    want = [ref.gram(cs, idf, unseen) for cs in imgs[:7]]
    return corpus, imgs, idf, unseen, want


@pytest.fixture(scope="module")
def cg(lib, case):
    return mbr.CiderGram(lib, case[0], BOS, EOS, vocab_size=65536)


def _table(cg, imgs):
    """the idf-weighted ngram_vectors table of the images' captions, head = cand_img [B + 1]"""
    per = np.array([len(c) for c in imgs], np.int64)
    cand_img = np.concatenate([[0], np.cumsum(per)])
    W, L = word_rows([c for cs in imgs for c in cs], BOS, EOS)
    return ngram_vectors(cg.lib, cg.dev, W, L, BOS, EOS, cg.df_keys, cg.idf, cg.n_df, cg.idf_unseen, head=cand_img), per, cand_img


def _raw(lib, v, per, weight=None, gram=True, want_mbr=True, ld=LD, max_cands=None, b0=0, B=None):
    """vc_cider_gram through the C ABI -> (gram [C + 3, ld] float32, mbr [C + 3] float64), both CANARY before the launch"""
    C = int(per.sum())
    g = torch.full((C + 3, ld), CANARY, dtype=torch.float32, device="cuda")
    m = torch.full((C + 3,), CANARY, dtype=torch.float64, device="cuda")
    w = None if weight is None else dev(np.asarray(weight, np.float64))
    lib.vc_cider_gram(stream(), len(per) - b0 if B is None else B, P(v.head) + 4 * b0, int(per.max()) if max_cands is None else max_cands,
                      P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm), P(v.words), P(w), P(g) if gram else None, ld,
                      P(m) if want_mbr else None)
    return host(g), host(m)


@pytest.fixture(scope="module")
def full(lib, cg, case):
    """the one call over the eight images: (table, per, cand_img, gram, mbr)"""
    v, per, cand_img = _table(cg, case[1])
    g, m = _raw(lib, v, per)
    return v, per, cand_img, g, m


def _image(g, cand_img, b):
    n = cand_img[b + 1] - cand_img[b]
    return g[cand_img[b]:cand_img[b + 1], :n]


# ------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("b", [4, 6])
def test_every_pair_has_the_bits_of_consensus_score(lib, cg, case, full, b):
    """the 5- and the 65-caption image: vc_consensus_score with one reference caption per "index image" (img_cap = arange), query q
    looking at index image q alone (k = 1, nbr[q] = q, m = 1) and listing all K captions as its candidates (K copies of the candidate
    table) returns score[q * K + i] = CIDEr-D(caption i, reference q) -- the same float32, exactly"""
    caps = case[1][b]
    K = len(caps)
    rv, _, _ = _table(cg, [caps])
    cv, _, cand = _table(cg, [caps] * K)
    score = torch.full((K * K,), CANARY, dtype=torch.float64, device="cuda")
    lib.vc_consensus_score(stream(), K, 1, P(dev(np.arange(K), np.int32)), P(dev(np.arange(K + 1), np.int32)), P(rv.off), P(rv.nnz),
                           P(rv.keys), P(rv.w), P(rv.norm), P(rv.words), P(cv.head), K, P(cv.off), P(cv.nnz), P(cv.keys), P(cv.w), P(cv.norm),
                           P(cv.words), 1, P(score))
    s = host(score).reshape(K, K).T                               # [i, q]
    G = _image(full[3], full[2], b)
    assert G.dtype == np.float32 and G.shape == (K, K)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)            # the scores ARE float32 values
    assert np.array_equal(G, s.astype(np.float32)), np.argwhere(G != s.astype(np.float32))[:5]
    assert (G > 0).sum() > K                                     # (not a comparison of zeros)


def test_the_matrix_against_the_float64_reference(case, full):
    corpus, imgs, idf, unseen, want = case
    v, per, cand_img, g, m = full
    for b in range(7):
        G = _image(g, cand_img, b)
        assert G.shape == want[b].shape == (PER[b], PER[b])
        np.testing.assert_allclose(G, want[b], rtol=RTOL, atol=ATOL, err_msg="image %d" % b)
        diag = np.array([2.5 * ref.orders(c, idf, unseen) for c in imgs[b]])
        np.testing.assert_allclose(np.diag(G), diag, rtol=RTOL, atol=ATOL, err_msg="diagonal of image %d" % b)
    rows = [0, 3, 124, 127, 252, 255]                            # the first and last row of the first, a middle and the last group ...
    rows += [1, 2, 125, 126, 253, 254]                           # ... and the rows between them: 12 rows
    G = _image(g, cand_img, 7)
    np.testing.assert_allclose(G[rows], ref.gram_rows(imgs[7], rows, idf, unseen), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(np.diag(G), [2.5 * ref.orders(c, idf, unseen) for c in imgs[7]], rtol=RTOL, atol=ATOL)
    # what the plants are there for
    G3, G4, G5 = (_image(g, cand_img, b) for b in (3, 4, 5))
    assert (G3[0] == 0).all() and (G3[:, 0] == 0).all() and abs(G3[1, 1] - 2.5) <= 1e-5       # no word: zeros; one word: one order
    assert np.array_equal(G4[3], G4[2]) and np.array_equal(G4[:, 3], G4[:, 2])              # duplicates: equal rows and columns
    np.testing.assert_allclose(G5[0, 0], 10.0, rtol=RTOL)                                    # 64 words: all four orders
    np.testing.assert_allclose(G5[1, 1], 10.0, rtol=RTOL)                                    # the largest id: keys with all 16 bits set
    assert G5[0, 2] > 0.5 and G5[2, 0] > 0.5 and G5[0, 2] != G5[2, 0]                        # CIDEr-D is not symmetric
    assert np.isfinite(g[g != CANARY]).all()


def test_nothing_is_written_outside_the_matrices(full):
    v, per, cand_img, g, m = full
    C = int(per.sum())
    for b, n in enumerate(PER):
        assert (g[cand_img[b]:cand_img[b + 1], n:] == CANARY).all(), b     # columns j >= n_b of a row
        assert (g[cand_img[b]:cand_img[b + 1], :n] != CANARY).all(), b
    assert (g[C:] == CANARY).all() and (m[C:] == CANARY).all() and (m[:C] != CANARY).all()


# ------------------------------------------------------------------ the weighted means
def _host_mbr(G, w=None):
    """float64 weighted mean of the returned float32 matrix, on the host"""
    G = G.astype(np.float64)
    w = np.ones(G.shape[0]) if w is None else np.asarray(w, np.float64)
    return (G * w[None, :]).sum(axis=1) / w.sum() if w.sum() != 0 else np.zeros(G.shape[0])


def test_uniform_means(lib, full):
    """against the host's float64 mean of the returned float32 matrix, and against vc_consensus_score taking the mean over the whole
    "pool" of the image's own captions (k = 1, nbr[b] = b, img_cap = cand_img, m = 2048): 1e-13 -- at most 256 positive float64 terms
    in two summation orders"""
    v, per, cand_img, g, m = full
    B = len(per)
    for b in range(B):
        np.testing.assert_allclose(m[cand_img[b]:cand_img[b + 1]], _host_mbr(_image(g, cand_img, b)), rtol=1e-13, atol=0, err_msg="image %d" % b)
    score = torch.full((int(per.sum()),), CANARY, dtype=torch.float64, device="cuda")
    lib.vc_consensus_score(stream(), B, 1, P(dev(np.arange(B), np.int32)), P(v.head), P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm),
                           P(v.words), P(v.head), 256, P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm), P(v.words), 2048, P(score))
    np.testing.assert_allclose(m[:int(per.sum())], host(score), rtol=1e-13, atol=0)
    assert (m[:int(per.sum())] >= 0).all() and m[cand_img[7]:cand_img[8]].min() > 0


def test_weighted_means_and_absent_outputs(lib, full):
    v, per, cand_img, g, m = full
    C, rng = int(per.sum()), np.random.default_rng(2)
    counts = rng.integers(1, 9, size=C).astype(np.float64)
    frac = rng.random(C)
    for b in range(len(per)):
        if per[b]:
            frac[cand_img[b]:cand_img[b + 1]] /= frac[cand_img[b]:cand_img[b + 1]].sum()      # fractional weights summing to 1
    zero = counts.copy()
    zero[cand_img[4]:cand_img[5]] = 0.0                                                       # a zero-weight image
    zero[cand_img[6]:cand_img[6] + 60] = 0.0                                                  # zero weights inside an image
    for name, w in (("counts", counts), ("fractions", frac), ("zeros", zero)):
        gw, mw = _raw(lib, v, per, weight=w)
        assert np.array_equal(gw, g), name                                                    # the weights do not touch the matrix
        for b in range(len(per)):
            s = slice(cand_img[b], cand_img[b + 1])
            np.testing.assert_allclose(mw[s], _host_mbr(_image(g, cand_img, b), w[s]), rtol=1e-13, atol=0, err_msg="%s, image %d" % (name, b))
        if name == "zeros":
            assert (mw[cand_img[4]:cand_img[5]] == 0.0).all() and (mw[cand_img[6]:cand_img[7]] > 0).any()
    only_g, m_none = _raw(lib, v, per, want_mbr=False)
    g_none, only_m = _raw(lib, v, per, gram=False)
    assert np.array_equal(only_g, g) and (m_none == CANARY).all()
    assert np.array_equal(only_m, m) and (g_none == CANARY).all()


# ------------------------------------------------------------------ independence
def test_rows_do_not_depend_on_the_launch_the_chunk_or_their_place(lib, cg, case, full, monkeypatch):
    corpus, imgs, idf, unseen, want = case
    v, per, cand_img, g, m = full
    Gs, ms = cg.gram(imgs)                                        # one chunk
    for b in range(len(PER)):
        assert Gs[b].dtype == np.float32 and ms[b].dtype == np.float64 and Gs[b].shape == (PER[b], PER[b]) and ms[b].shape == (PER[b],)
        assert np.array_equal(Gs[b], _image(g, cand_img, b)) and np.array_equal(ms[b], m[cand_img[b]:cand_img[b + 1]]), b
    for b in (2, 4, 6, 7):                                        # an image evaluated alone
        G1, m1 = cg.gram([imgs[b]])
        assert np.array_equal(G1[0], Gs[b]) and np.array_equal(m1[0], ms[b]), b
    # a launch that starts at image 5 of the same table (B = 2), into a narrower matrix
    g2, m2 = _raw(lib, v, per, b0=5, B=2, ld=68, max_cands=65)
    for b in (5, 6):
        assert np.array_equal(g2[cand_img[b]:cand_img[b + 1], :PER[b]], Gs[b]) and np.array_equal(m2[cand_img[b]:cand_img[b + 1]], ms[b])
    assert (g2[:cand_img[5]] == CANARY).all() and (g2[cand_img[7]:] == CANARY).all() and (m2[cand_img[7]:] == CANARY).all()
    # without its first caption every row of the 65-caption image moves to another place in its group of four
    G6, _ = cg.gram([imgs[6][1:]])
    assert np.array_equal(G6[0], Gs[6][1:, 1:])
    # one image per chunk
    monkeypatch.setattr(mbr, "GRAM_BLOCK_BYTES", 1)
    assert len(mbr.chunks(PER, mbr.GRAM_BLOCK_BYTES)) == len(PER)
    w = [np.arange(1, n + 1, dtype=np.float64).tolist() for n in PER]
    Gc, mc = cg.gram(imgs, w)
    monkeypatch.undo()
    Gw, mw = cg.gram(imgs, w)
    for b in range(len(PER)):
        assert np.array_equal(Gc[b], Gs[b]) and np.array_equal(Gw[b], Gs[b]) and np.array_equal(mc[b], mw[b]), b
    assert not np.array_equal(mw[6], ms[6])
    nothing = cg.gram([[], []])
    assert [x.shape for x in nothing[0]] == [(0, 0)] * 2 and [x.shape for x in nothing[1]] == [(0,)] * 2 and cg.gram([]) == ([], [])


def test_bad_arguments(lib, full):
    v, per, cand_img, g, m = full
    out = torch.full((int(per.sum()), LD), CANARY, dtype=torch.float32, device="cuda")
    mb = torch.full((int(per.sum()),), CANARY, dtype=torch.float64, device="cuda")

    def call(B=8, head=P(v.head), max_cands=256, keys=P(v.keys), gram=P(out), ld=LD, mbr_=P(mb)):
        lib.vc_cider_gram(stream(), B, head, max_cands, P(v.off), P(v.nnz), keys, P(v.w), P(v.norm), P(v.words), None, gram, ld, mbr_)
    for bad in (dict(keys=None), dict(head=None), dict(ld=255), dict(max_cands=257), dict(gram=None, mbr_=None), dict(B=-1), dict(max_cands=-1)):
        with pytest.raises(VaecapError, match="invalid argument"):
            call(**bad)
    call(B=0)
    call(max_cands=0)
    assert (host(out) == CANARY).all() and (host(mb) == CANARY).all()          # no launch so far
    call()
    assert np.array_equal(host(out), g[:int(per.sum())])


# ------------------------------------------------------------------ the evaluator
@pytest.fixture(scope="module")
def e2e():
    """12 images x up to 20 captions x 5 references, vocabulary 30 (a caption drawn twice for an image is listed once); image 4 lists
    nothing, image 9 one caption, image 7 six copies of one.  The seed keeps every reference eigenvalue that is not a structural zero at or above 1e-3 (small eigenvalues amplify float32
    differences under the square root) and the best two mbr values of every image more than 1e-4 apart."""
    rng = np.random.default_rng(E2E_SEED)
    cands, refs = _related(rng, 12, 20, 5, 30)
    cands = [[list(c) for c in dict.fromkeys(map(tuple, cs))] for cs in cands]
    cands[4], cands[9], cands[7] = [], cands[9][:1], [list(cands[7][0]) for _ in range(6)]
    want = ref.evaluate(cands, refs, BOS, EOS)
    for b, G in enumerate(want["per_image"]["gram"]):
        if b in (4, 7, 9):
            continue
        lam = ref.eigenvalues(G)
        assert lam.min() >= 1e-3, (b, lam[:3])
        top2 = np.sort(want["per_image"]["caption_mbr"][b])[-2:]
        assert top2[1] - top2[0] > 1e-4, (b, top2)
    return cands, refs, want



def test_evaluate_with_the_set_metrics(lib, e2e, monkeypatch):
    cands, refs, want = e2e
    evaluator = CaptionEvaluator(lib, refs, BOS, EOS, vocab_size=30)
    launches = []
    real = mbr._launch

    def counted(*a):
        launches.append(a[1])
        return real(*a)
    monkeypatch.setattr(mbr, "_launch", counted)
    res = evaluator.evaluate(cands, self_cider=True)
    assert launches == [12]                                       # one vc_cider_gram pass over the 12 images
    assert set(res) == set(METRICS) | set(SET_METRICS) | {"per_image"}
    per, wper = res["per_image"], want["per_image"]
    for k in SET_METRICS:
        print("%s: got %.17g want %.17g deviation %.3e (bound %.3e)" % (k, res[k], want[k], abs(res[k] - want[k]), SET_BOUND[k]))
    live = [b for b in range(12) if b != 4]
    worst = max(abs(per["self_cider"][b] - wper["self_cider"][b]) for b in live)
    print("self_cider of one image: largest deviation %.3e (bound %.3e)" % (worst, SET_BOUND["image_self_cider"]))
    for k in SET_METRICS:
        assert isinstance(res[k], float) and abs(res[k] - want[k]) <= SET_BOUND[k], k
    assert np.array_equal(per["mbr_choice"], wper["mbr_choice"]) and per["mbr_choice"][4] == -1 and per["mbr_choice"][7] == 0
    for b in range(12):
        np.testing.assert_allclose(per["caption_mbr"][b], wper["caption_mbr"][b], rtol=RTOL, atol=ATOL, err_msg="image %d" % b)
    assert worst <= SET_BOUND["image_self_cider"]
    assert per["self_cider"][7] == 0.0 and per["self_cider"][9] == 0.0 and math.isnan(per["self_cider"][4])
    assert 0 < res["self_cider"] < 1 and res["mbr_cider_d"] <= res["oracle_cider_d"]
    np.testing.assert_allclose(res["mbr_cider_d"], np.mean([per["caption_cider_d"][b][per["mbr_choice"][b]] for b in range(12) if b != 4]),
                               rtol=1e-15)
    # without the flag: the old key set, the old bits, no launch
    del launches[:]
    old = evaluator.evaluate(cands)
    assert launches == [] and set(old) == set(METRICS) | {"per_image"}
    assert not {"self_cider", "mbr_choice", "caption_mbr"} & set(old["per_image"])
    for k in METRICS:
        assert old[k] == res[k] or (old[k] is None and res[k] is None), k
    for a, c in zip(old["per_image"]["caption_cider_d"], per["caption_cider_d"]):
        assert np.array_equal(a, c)
    nothing = evaluator.evaluate([[] for _ in cands], self_cider=True)
    assert launches == [] and nothing["self_cider"] == 0.0 and nothing["mbr_cider_d"] == 0.0


# ------------------------------------------------------------------ the decoder
def _decoder(lib, rerank="mbr"):
    from vae_captioning_amd.vae_model.decoder import Decoder
    p = _facade_params()
    p.diverse_rerank = rerank
    dec = Decoder(None, None, None, p, _Dict)
    rng = np.random.default_rng(12)
    corpus = [_caps(rng, 3, 40, 2, 9) for _ in range(30)]
    dec.mbr = mbr.CiderGram(lib, corpus, BOS, EOS, vocab_size=40)
    return dec, p, cref.df_idf(corpus, BOS, EOS)


def test_decoder_diverse_inference_with_mbr(lib):
    dec, p, (idf, unseen) = _decoder(lib)
    feats = np.maximum(np.random.default_rng(0).standard_normal((3, 48)), 0).astype(np.float32)
    recs = dec.diverse_inference(None, ["a", "b", "c"], feats, None)
    ids = dec.last_token_ids
    for r, toks in zip(recs, ids):
        assert set(r) == {"image_id", "caption", "captions", "scores", "counts", "mbr"} and sum(r["counts"]) == 6
        assert r["mbr"] == sorted(r["mbr"], reverse=True) and len(r["mbr"]) == len(r["captions"]) == len(toks)
        assert r["caption"] == r["captions"][0] and r["captions"] == [dec._text(t, (BOS, EOS)) for t in toks]
        np.testing.assert_allclose(r["mbr"], ref.mbr(ref.gram(toks, idf, unseen), r["counts"]), rtol=RTOL, atol=ATOL)
    two = dec.diverse_inference(None, ["a", "b", "c"], feats, None, n_best=2)
    assert [r["captions"] for r in two] == [r["captions"][:2] for r in recs] and [r["mbr"] for r in two] == [r["mbr"][:2] for r in recs]
    p.diverse_rerank = "likelihood"
    plain = dec.diverse_inference(None, ["a", "b", "c"], feats, None)
    assert all("mbr" not in r for r in plain) and [sorted(r["captions"]) for r in plain] == [sorted(r["captions"]) for r in recs]
    dec.mbr, p.diverse_rerank = None, "mbr"
    with pytest.raises(RuntimeError, match=r"mbr\.CiderGram"):
        dec.diverse_inference(None, ["a", "b", "c"], feats, None)
    assert dec.last_token_ids is None


def test_decoder_stochastic_beam_search_with_mbr(lib):
    dec, p, (idf, unseen) = _decoder(lib)
    p.temperature = 1.0
    feats = np.maximum(np.random.default_rng(3).standard_normal((3, 48)), 0).astype(np.float32)
    recs = dec.stochastic_beam_search(None, ["a", "b", "c"], feats, None, beam_size=4)
    for r, toks in zip(recs, dec.last_token_ids):
        assert len(r["captions"]) == len(r["norm_weight"]) == len(r["mbr"]) == len(toks) == 4 and r["caption"] == r["captions"][0]
        assert r["mbr"] == sorted(r["mbr"], reverse=True) and r["captions"] == [dec._text(t, (BOS, EOS)) for t in toks]
        np.testing.assert_allclose(r["mbr"], ref.mbr(ref.gram(toks, idf, unseen), r["norm_weight"]), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ the command line
def test_main_inference_with_mbr_and_the_set_metrics(tmp_path):
    _main(SMALL + ["--epochs", "1", "--max_steps", "1"], tmp_path)
    out = _main(SMALL + ["--mode", "inference", "--sample_gen", "diverse", "--diverse_draws", "4", "--diverse_rerank", "mbr", "--eval_captions",
                         "--eval_self_cider"], tmp_path)
    assert len(re.findall(r"^mbr re-ranking: idf over the captions of 512 training images$", out, flags=re.M)) == 1, out
    m = json.load(open(tmp_path / "val_00_metrics.json"))
    recs = json.load(open(tmp_path / "val_00_diverse.json"))
    assert set(METRICS) | set(SET_METRICS) <= set(m) and m["eval_self_cider"] is True and m["diverse_rerank"] == "mbr"
    assert 0.0 <= m["self_cider"] <= 1.0 and m["mbr_cider_d"] <= m["oracle_cider_d"]
    for k in SET_METRICS:
        assert len(re.findall(r"^%s: \d+\.\d{6}$" % k, out, flags=re.M)) == 1, k
    assert len(recs) == 8 and all(r["mbr"] == sorted(r["mbr"], reverse=True) and len(r["mbr"]) == len(r["captions"]) for r in recs)
    assert all(sum(r["counts"]) == 4 for r in recs)
