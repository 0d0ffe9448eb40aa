"""Evaluation of caption sets on the GPU: the numbers the AG-CVAE paper reports for a set of captions per image -- accuracy of the top
caption (BLEU-1..4, CIDEr-D, ROUGE-L), "oracle" accuracy of the best caption of the set, and the diversity of the set (share of distinct
captions, share of novel sentences, Div-1, Div-2, mBLEU-4).

`CaptionEvaluator(lib_or_engine, references, bos, eos)` holds the n-gram vectors of every image's human captions on the device;
`evaluate(candidates)` takes per image a ranked list of token-id lists (best first, possibly empty) and returns a dict of float64
values (METRICS) plus per-image arrays under "per_image".

Words are token ids without <BOS>, <EOS> and PAD (0), as in consensus.py, whose limits hold here: at most 64 words per caption, ids
<= 65535, at most 256 captions and 2048 references per image.

Every integer comes from the device, every float from float64 arithmetic on those integers on the host:

* BLEU-style counts: csrc/evaluate.hip's vc_ngram_overlap on count vectors (vc_ngram_vectors with an empty df table), called three
  times on one hypothesis table -- against the image's references (BLEU), against the image's EARLIER captions (an n-gram unseen there
  is a new distinct n-gram of the image: Div-n), against the image's OTHER captions (mBLEU).  One copy-back of the integer arrays.
* CIDEr-D: vc_consensus_score on idf-weighted vectors with k = 1, nbr[b] = b, the references' offsets as img_cap and m = 2048, i.e.
  the mean over ALL references of the image of the one-reference CIDEr-D.  The idf is coco-caption's convention: document frequencies
  over the evaluated images' references (consensus.host_index), unseen n-grams log D.
* ROUGE-L: csrc/lcs.hip's vc_lcs_overlap on the word rows the hypothesis and reference count tables already hold on the device, against
  the image's references (the range array of the BLEU call): per caption the largest LCS and the (LCS, words) pair of the reference
  with the largest LCS / words, three integers that ride in the one copy-back.  `rouge_l` turns them into coco-caption's score
  (precision and recall take their maxima over the references separately, beta = 1.2).

BLEU here is the plain corpus-level definition (corpus_bleu): it does NOT imitate coco-caption's smoothing constants (its 1e-9 "tiny" /
1e-15 "small" terms), and the tokens are vocabulary ids after the vocabulary cut, not PTB tokens -- the numbers compare runs of this
project with each other, not with a leaderboard ("Evaluation").

`evaluate(candidates, self_cider=True)` adds SET_METRICS from one more pass over the CIDEr-D path's candidate table (mbr.py,
csrc/cider_gram.hip's vc_cider_gram: the CIDEr-D of every caption of an image against every caption of the same image): `self_cider`,
the Self-CIDEr diversity of the set (host float64 eigenvalues of that matrix), and `mbr_cider_d`, the CIDEr-D of the caption with the
highest mean in-set CIDEr-D -- what minimum-Bayes-risk selection would take.  Without it nothing changes and the kernel is not launched.

Single-caption modes (greedy, sample, beam_search) hand in lists of one: the set metrics are then those of lists of one -- `distinct`
1.0, `mbleu_4` 0.0 (no hypotheses), `oracle_cider_d` = `mean_cider_d` = `cider_d`, `oracle_rouge_l` = `mean_rouge_l` = `rouge_l`."""
import math
import types

import numpy as np
import torch

from .abi import ptr as P
from .consensus import MAX_POOL, host_index, library_and_device, ngram_vectors, upload, word_rows
from .engine import _stream
from .generate import DIVERSE_MAX_DRAWS

METRICS = ("bleu_1", "bleu_2", "bleu_3", "bleu_4", "cider_d", "oracle_cider_d", "mean_cider_d", "distinct", "div_1", "div_2", "mbleu_4",
           "novel", "rouge_l", "oracle_rouge_l", "mean_rouge_l")
SET_METRICS = ("self_cider", "mbr_cider_d")   # evaluate(self_cider=True) only: they need the in-set CIDEr-D matrix (mbr.py, vc_cider_gram)
MAX_REFS = MAX_POOL       # references per image (vc_consensus_score stages an image's pool in LDS)
OUT_COLS = 17             # total, match, distinct, unseen [., 4] + ref_len per hypothesis
LCS_COLS = 3              # lcs_max, rec_lcs, rec_len per hypothesis (vc_lcs_overlap)


def corpus_bleu(match, total, hyp_len, ref_len):
    """Corpus-level BLEU-1..4 from integer sums over the hypotheses: match[n-1] / total[n-1] the clipped and the total n-gram counts,
    hyp_len = C and ref_len = R the summed hypothesis and closest-reference lengths.  p_n = match_n / total_n, BLEU_n = BP * exp(mean
    over i <= n of log p_i), BP = 1 if C >= R else exp(1 - R / C); 0.0 when any p_i is 0 (or has no n-gram) or C is 0.  Plain float64,
    no smoothing constants.  -> [BLEU_1 .. BLEU_4]"""
    C, R = int(hyp_len), int(ref_len)
    out, logsum, dead = [], 0.0, C == 0
    bp = 1.0 if C >= R or C == 0 else math.exp(1.0 - R / C)
    for n in range(4):
        m, t = int(match[n]), int(total[n])
        dead = dead or m == 0 or t == 0
        if not dead:
            logsum += math.log(m / t)
        out.append(0.0 if dead else bp * math.exp(logsum / (n + 1)))
    return out


def count_vectors(lib, dev, W, L, bos, eos, head=None):
    """n-gram COUNT vectors of word rows: vc_ngram_vectors with an empty df table and idf_unseen = 1, so w is the exact count"""
    return ngram_vectors(lib, dev, W, L, bos, eos, None, None, 0, 1.0, head)


def check_ranges(lo, hi, skip, n_hyp, n_ref):
    """lo / hi / skip [n_hyp] of vc_ngram_overlap, checked on the host (the library itself clamps a bad range to an empty one)"""
    lo, hi, skip = (np.asarray(a, np.int64).reshape(-1) for a in (lo, hi, skip))
    if not (lo.size == hi.size == skip.size == n_hyp):
        raise ValueError("lo, hi and skip must hold one entry per hypothesis row (%d)" % n_hyp)
    if n_hyp and ((lo < 0) | (lo > hi) | (hi > n_ref)).any():
        r = int(np.flatnonzero((lo < 0) | (lo > hi) | (hi > n_ref))[0])
        raise ValueError("row %d: range [%d, %d) is not inside the %d reference rows" % (r, lo[r], hi[r], n_ref))
    if n_hyp and (skip < -1).any():
        raise ValueError("skip must be a reference row or -1")
    return lo.astype(np.int32), hi.astype(np.int32), skip.astype(np.int32)


def _launch(lib, hyp, ref, rng, out):
    """rng: int32 device [3, C] (lo, hi, skip); out: int32 device [OUT_COLS * C]"""
    C = hyp.n
    o = [P(out) + 4 * C * 4 * i for i in range(5)]
    lib.vc_ngram_overlap(_stream(), C, P(hyp.off), P(hyp.nnz), P(hyp.keys), P(hyp.w), P(hyp.words), ref.n, P(ref.off), P(ref.nnz),
                         P(ref.keys), P(ref.w), P(ref.words), P(rng), P(rng) + 4 * C, P(rng) + 8 * C, o[0], o[1], o[2], o[3], o[4])


def _split(a, C):
    """host int32 [OUT_COLS * C] -> dict of the five outputs"""
    q = a[:16 * C].reshape(4, C, 4)
    return dict(total=q[0], match=q[1], distinct=q[2], unseen=q[3], ref_len=a[16 * C:17 * C])


def ngram_overlap(lib_or_engine, hyp, ref, lo, hi, skip=None):
    """One vc_ngram_overlap call on two count_vectors tables (they may be the same one): hypothesis row c against reference rows
    [lo[c], hi[c]) without row skip[c] (-1 / None: none).  -> dict of int32 arrays total, match, distinct, unseen [C, 4], ref_len [C]."""
    lib, dev = library_and_device(lib_or_engine)
    C = hyp.n
    lo, hi, skip = check_ranges(lo, hi, np.full(C, -1) if skip is None else skip, C, ref.n)
    if C == 0:
        return _split(np.zeros(0, np.int32), 0)
    rng = upload(dev, np.stack([lo, hi, skip]))
    out = torch.empty(OUT_COLS * C, dtype=torch.int32, device=dev)
    _launch(lib, hyp, ref, rng, out)
    return _split(out.cpu().numpy(), C)


def _launch_lcs(lib, hyp, ref, rng, out):
    """hyp / ref: tables that hold their word rows on the device (tok [n, ld], len [n]: ngram_vectors outputs or word_table);
    rng: int32 device [3, C] (lo, hi, skip); out: int32 device [LCS_COLS * C]"""
    C = hyp.n
    lib.vc_lcs_overlap(_stream(), C, P(hyp.tok), hyp.ld, P(hyp.len), ref.n, P(ref.tok), ref.ld, P(ref.len), P(rng), P(rng) + 4 * C,
                       P(rng) + 8 * C, P(out), P(out) + 4 * C, P(out) + 8 * C)


def _split_lcs(a, C):
    """host int32 [LCS_COLS * C] -> dict of the three outputs"""
    return dict(lcs_max=a[:C], rec_lcs=a[C:2 * C], rec_len=a[2 * C:3 * C])


def word_table(dev, W, L, head=None):
    """Word rows (consensus.word_rows) on the device, in one copy: what vc_lcs_overlap needs of a table (n, tok [n, ld], len [n]) without
    the n-gram vectors.  head: an int32 array sent along (t.head is its device copy)."""
    n = int(W.shape[0])
    head = np.zeros(0, np.int32) if head is None else np.asarray(head, np.int32).reshape(-1)
    h = head.size
    up = upload(dev, np.concatenate([head, np.asarray(L, np.int32), np.asarray(W, np.int32).reshape(-1)]))
    return types.SimpleNamespace(n=n, head=up[:h], len=up[h:h + n], tok=up[h + n:], ld=int(W.shape[1]))


def lcs_overlap(lib_or_engine, hyp, ref, lo, hi, skip=None):
    """One vc_lcs_overlap call on two tables that hold their word rows on the device (count_vectors / ngram_vectors outputs or
    word_table; they may be the same one): hypothesis row c against reference rows [lo[c], hi[c]) without row skip[c] (-1 / None:
    none).  -> dict of int32 arrays [C]: lcs_max (the largest LCS over the range), rec_lcs and rec_len (LCS and words of the row with the
    largest LCS / words; a tie goes to the shorter row); all 0 when no row of the range has a word."""
    lib, dev = library_and_device(lib_or_engine)
    C = hyp.n
    lo, hi, skip = check_ranges(lo, hi, np.full(C, -1) if skip is None else skip, C, ref.n)
    if C == 0:
        return _split_lcs(np.zeros(0, np.int32), 0)
    rng = upload(dev, np.stack([lo, hi, skip]))
    out = torch.empty(LCS_COLS * C, dtype=torch.int32, device=dev)
    _launch_lcs(lib, hyp, ref, rng, out)
    return _split_lcs(out.cpu().numpy(), C)


def rouge_l(lcs_max, rec_lcs, rec_len, hyp_len, beta=1.2):
    """coco-caption's ROUGE-L per caption from vc_lcs_overlap's integers and the captions' word counts: P = lcs_max / hyp_len,
    R = rec_lcs / rec_len (each its maximum over the references), score = (1 + beta^2) P R / (R + beta^2 P) in float64, evaluated in
    this order; 0.0 where hyp_len, rec_len or either LCS is 0.  -> float64 array"""
    m, l, n, h = (np.asarray(a, np.float64).reshape(-1) for a in (lcs_max, rec_lcs, rec_len, hyp_len))
    live = (m > 0) & (l > 0) & (n > 0) & (h > 0)
    p = m / np.where(live, h, 1.0)
    r = l / np.where(live, n, 1.0)
    score = (1 + beta ** 2) * p * r / np.where(live, r + beta ** 2 * p, 1.0)
    return np.where(live, score, 0.0)


def _mean(x):
    x = np.asarray(x, np.float64)
    return float(x.mean()) if x.size else 0.0


class CaptionEvaluator(object):
    """references: per image a list of token-id lists (1..2048); train_captions: an optional flat list of token-id lists for `novel`.
    lib_or_engine: the C-ABI library (abi.load()) or a CaptionEngine (its library and device)."""

    def __init__(self, lib_or_engine, references, bos, eos, vocab_size=None, train_captions=None):
        self.lib, self.dev = library_and_device(lib_or_engine)
        self.bos, self.eos = int(bos), int(eos)
        self.B = len(references)
        if self.B == 0:
            raise ValueError("the evaluator needs the references of at least one image")
        per = np.fromiter((len(r) for r in references), np.int64, self.B)
        if per.min() < 1:
            raise ValueError("image %d has no reference caption" % int(np.argmin(per)))
        if per.max() > MAX_REFS:
            raise ValueError("at most %d references per image (image %d has %d)" % (MAX_REFS, int(np.argmax(per)), per.max()))
        h = host_index(references, bos, eos, vocab_size)
        self.ref_off = h.img_cap                                   # int64 [B + 1]
        self.n_refs = int(h.L.size)
        self.n_df = int(h.df_keys.size)
        self.df_keys = upload(self.dev, h.df_keys.view(np.int64) if self.n_df else np.zeros(1, np.int64))
        self.idf = upload(self.dev, h.idf if self.n_df else np.zeros(1, np.float32))
        self.idf_unseen = float(h.idf_unseen)
        self.ref_counts = count_vectors(self.lib, self.dev, h.W, h.L, bos, eos)
        self.ref_idf = self._idf_vectors(h.W, h.L, head=np.concatenate([h.img_cap, np.arange(self.B)]))   # head: img_cap, nbr [B, 1]
        self.train = None
        if train_captions is not None:
            Wt, Lt = word_rows(list(train_captions), bos, eos, owner=lambda i: "training caption %d" % i)
            Wt = Wt.astype(np.int32)
            self.train = {Wt[i, :Lt[i]].tobytes() for i in range(Wt.shape[0])}

    def _idf_vectors(self, W, L, head=None):
        return ngram_vectors(self.lib, self.dev, W, L, self.bos, self.eos, self.df_keys, self.idf, self.n_df, self.idf_unseen, head)

    def _cider(self, W, L, cand_img, max_cands, table=None):
        """CIDEr-D of every candidate: the mean over its image's references (vc_consensus_score, k = 1, m = 2048) -> device float64.
        table: the candidates' idf-weighted vectors (_idf_vectors(W, L, head=cand_img)) when the caller has built them already."""
        cv, rv, B = table if table is not None else self._idf_vectors(W, L, head=cand_img), self.ref_idf, self.B
        out = torch.empty(max(1, cv.n), dtype=torch.float64, device=self.dev)
        self.lib.vc_consensus_score(_stream(), B, 1, P(rv.head[B + 1:]), P(rv.head[:B + 1]), P(rv.off), P(rv.nnz), P(rv.keys), P(rv.w),
                                    P(rv.norm), P(rv.words), P(cv.head), int(max_cands), P(cv.off), P(cv.nnz), P(cv.keys), P(cv.w),
                                    P(cv.norm), P(cv.words), MAX_REFS, P(out))
        return out

    def _set_metrics(self, cv, per, cider, cand_img):
        """evaluate(self_cider=True): one vc_cider_gram pass over the candidates' idf-weighted table `cv` (uniform weights), then per
        image Self-CIDEr of its matrix (host float64 eigenvalues) and the caption MBR selection would take: the first maximum of mbr"""
        from . import mbr as M
        B = self.B
        if cv is None:
            G, mb = [np.zeros((0, 0), np.float32)] * B, [np.zeros(0, np.float64)] * B
        else:
            G, mb = M.gram_of_table(self.lib, self.dev, cv, cv.head, per)
        sc = np.array([M.self_cider(g) for g in G], np.float64)
        choice = np.array([int(np.argmax(m)) if m.size else -1 for m in mb], np.int64)
        chosen = np.array([cider[cand_img[b] + choice[b]] if choice[b] >= 0 else np.nan for b in range(B)], np.float64)
        return sc, choice, chosen, mb

    def evaluate(self, candidates, self_cider=False):
        """self_cider=True adds SET_METRICS: `self_cider`, the mean over the images that list a caption of mbr.self_cider of the
        image's in-set CIDEr-D matrix, and `mbr_cider_d`, the mean over those images of the CIDEr-D (against the human references) of
        the caption with the highest mean in-set CIDEr-D (uniform weights, first maximum); per_image gains self_cider, mbr_choice (-1:
        no caption) and caption_mbr.  Without it vc_cider_gram is never launched and nothing else changes."""
        B = self.B
        if len(candidates) != B:
            raise ValueError("%d images of candidates for %d images of references" % (len(candidates), B))
        per = np.fromiter((len(c) for c in candidates), np.int64, B)
        if per.max() > DIVERSE_MAX_DRAWS:
            raise ValueError("at most %d captions per image (image %d has %d)" % (DIVERSE_MAX_DRAWS, int(np.argmax(per)), per.max()))
        cand_img = np.zeros(B + 1, np.int64)
        cand_img[1:] = np.cumsum(per)
        C = int(cand_img[-1])
        image_of = np.repeat(np.arange(B), per)
        flat = [c for cs in candidates for c in cs]
        W, L = word_rows(flat, self.bos, self.eos, owner=lambda i: "caption %d of image %d" % (i - cand_img[image_of[i]], image_of[i]))
        W = W.astype(np.int32)
        rows = np.arange(C)
        start, end = cand_img[image_of], cand_img[image_of + 1]
        if C:
            # ---- device: one hypothesis table, three overlap calls, the LCS call, the CIDEr-D path; one copy-back of the integers
            hyp = count_vectors(self.lib, self.dev, W, L, self.bos, self.eos)
            none = np.full(C, -1)
            rng = upload(self.dev, np.stack([self.ref_off[image_of], self.ref_off[image_of + 1], none,      # the image's references
                                             start, rows, none,                                             # its earlier captions
                                             start, end, rows]).astype(np.int32).reshape(3, 3 * C))         # its other captions
            flat_out = torch.empty((3 * OUT_COLS + LCS_COLS) * C, dtype=torch.int32, device=self.dev)
            out = flat_out[:3 * OUT_COLS * C].view(3, OUT_COLS * C)
            for i, ref in enumerate((self.ref_counts, hyp, hyp)):
                _launch(self.lib, hyp, ref, rng[i], out[i])
            _launch_lcs(self.lib, hyp, self.ref_counts, rng[0], flat_out[3 * OUT_COLS * C:])   # the word rows of the two count tables
            cv = self._idf_vectors(W, L, head=cand_img)          # built once: the CIDEr-D call and the in-set matrices share it
            cider_dev = self._cider(W, L, cand_img, int(per.max()), table=cv)
            ints = flat_out.cpu().numpy()
            cider = cider_dev.cpu().numpy()[:C]
            to_ref, to_prev, to_rest = (_split(ints[OUT_COLS * C * i:OUT_COLS * C * (i + 1)], C) for i in range(3))
            lcs = _split_lcs(ints[3 * OUT_COLS * C:], C)
        else:
            cv, cider = None, np.zeros(0, np.float64)
            to_ref = to_prev = to_rest = _split(np.zeros(0, np.int32), 0)
            lcs = _split_lcs(np.zeros(0, np.int32), 0)
        # ---- host: float64 from exact integers
        have = per > 0
        top = cand_img[:-1][have]
        bleu = corpus_bleu(to_ref["match"][top].sum(axis=0, dtype=np.int64), to_ref["total"][top].sum(axis=0, dtype=np.int64),
                           L[top].sum(), to_ref["ref_len"][top].sum(dtype=np.int64))
        best = np.array([cider[cand_img[b]:cand_img[b + 1]].max() if per[b] else np.nan for b in range(B)], np.float64)
        top_cider = np.full(B, np.nan)
        top_cider[have] = cider[top]
        rouge = rouge_l(lcs["lcs_max"], lcs["rec_lcs"], lcs["rec_len"], L)
        top_rouge, best_rouge = np.full(B, np.nan), np.full(B, np.nan)
        top_rouge[have] = rouge[top]
        if C:
            best_rouge[have] = np.maximum.reduceat(rouge, top)   # (`top`: the first row of every image that lists a caption)
        # distinct word sequences per image: rows are 0-padded, so equal rows are equal captions
        uniq = np.unique(np.column_stack([image_of, W]), axis=0)[:, 0] if C else np.zeros(0, np.int64)
        n_distinct = np.bincount(uniq, minlength=B)
        share = np.full(B, np.nan)
        share[have] = n_distinct[have] / per[have]
        words = np.bincount(image_of, weights=L, minlength=B)
        div = np.full((2, B), np.nan)
        for n in range(2):
            new = np.bincount(image_of, weights=to_prev["unseen"][:, n], minlength=B) if C else np.zeros(B)
            div[n][words > 0] = new[words > 0] / words[words > 0]
        multi = per[image_of] >= 2
        mbleu = corpus_bleu(to_rest["match"][multi].sum(axis=0, dtype=np.int64), to_rest["total"][multi].sum(axis=0, dtype=np.int64),
                            L[multi].sum(), to_rest["ref_len"][multi].sum(dtype=np.int64))
        novel = None
        if self.train is not None:
            novel = (sum(W[i, :L[i]].tobytes() not in self.train for i in range(C)) / C) if C else 0.0
        res = dict(bleu_1=bleu[0], bleu_2=bleu[1], bleu_3=bleu[2], bleu_4=bleu[3], cider_d=_mean(top_cider[have]),
                   oracle_cider_d=_mean(best[have]), mean_cider_d=_mean(cider), distinct=_mean(share[have]), div_1=_mean(div[0][words > 0]),
                   div_2=_mean(div[1][words > 0]), mbleu_4=mbleu[3], novel=novel, rouge_l=_mean(top_rouge[have]),
                   oracle_rouge_l=_mean(best_rouge[have]), mean_rouge_l=_mean(rouge))
        res["per_image"] = dict(captions=per, cider_d=top_cider, oracle_cider_d=best, distinct=share, div_1=div[0], div_2=div[1],
                                caption_cider_d=[cider[cand_img[b]:cand_img[b + 1]].copy() for b in range(B)],
                                rouge_l=top_rouge, oracle_rouge_l=best_rouge,
                                caption_rouge_l=[rouge[cand_img[b]:cand_img[b + 1]].copy() for b in range(B)])
        if self_cider:
            sc, choice, chosen, mb = self._set_metrics(cv, per, cider, cand_img)
            res.update(self_cider=_mean(sc[have]), mbr_cider_d=_mean(chosen[have]))
            res["per_image"].update(self_cider=sc, mbr_choice=choice, caption_mbr=mb)
        return res
