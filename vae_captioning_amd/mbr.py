"""In-set CIDEr-D: minimum-Bayes-risk re-ranking of an image's captions and the Self-CIDEr diversity of the set.

Both need one matrix per image: G[i][j] = CIDEr-D(hypothesis = caption i, reference = caption j) over the image's OWN captions
(csrc/cider_gram.hip: vc_cider_gram, the pair function of vc_consensus_score).

* MBR selection (Kumar & Byrne 2004; sampling-based: Eikema & Aziz 2020): the caption with the highest expected CIDEr-D against the
  image's samples, mbr[i] = sum_j weight_j G[i][j] / sum_j weight_j.  It needs no index of training images, no features and no extra
  decoder pass; the weights are how often each distinct caption was drawn (`diverse`) or the captions' `norm_weight` (stochastic beam
  search).  The sum runs over all j, i itself included.
* Self-CIDEr (Wang & Chan, CVPR 2019): `self_cider(G)`, a function of the eigenvalues of the symmetrised matrix, on the host in float64.
* DPP selection (Chen, Zhang & Zhou, NeurIPS 2018): `CiderGram.select`, n captions chosen jointly for quality and for difference from
  each other -- greedy MAP of a determinantal point process whose kernel is the same symmetrised matrix scaled by the captions'
  qualities (csrc/dpp.hip: vc_dpp_select_f64, on the device block vc_cider_gram has just written; the matrix is not copied to the host).

`CiderGram` holds the df / idf table of a CORPUS (the training captions per image) on the device, as scst.CiderReward does; words, keys
and limits are consensus.py's: token ids without <BOS>, <EOS> and PAD (0), at most 64 words per caption, ids <= 65535, at most 256
captions per image.  DESIGN.md, "In-set CIDEr-D: MBR re-ranking and Self-CIDEr"."""
import math

import numpy as np
import torch

from .abi import ptr as P
from .consensus import library_and_device, ngram_vectors, rerank_entries, upload, word_rows
from .engine import _stream
from .generate import DIVERSE_MAX_DRAWS

ZERO_EIG = float(np.finfo(np.float64).eps)   # self_cider: eigenvalues up to ZERO_EIG * m * (the largest) are zeros (numpy.linalg.matrix_rank's rule)
GRAM_BLOCK_BYTES = 256 << 20   # the [captions, ld] f32 block of one vc_cider_gram call stays under this (one image always goes)
DPP_MAX_SELECT = 32            # vc_dpp_select_f64: captions selected per image (the c vectors of 32 steps x 256 captions fill 64 KiB of LDS)


def self_cider(G):
    """Self-CIDEr of one image's m x m matrix G (CIDEr-D of caption i against caption j, scaled by 10 as CIDEr-D is), host float64:
    S = (G + G^T) / 20 (CIDEr-D is not symmetric in hypothesis and reference), lam = eigvalsh(S) with negative values set to 0,
    r = sqrt(max lam) / sum sqrt(lam), result -log(r) / log(m).  0.0 for m == 1 and when sum sqrt(lam) == 0, NaN for m == 0; 0 for m
    identical captions, 1 for m captions that share no n-gram.
    An eigenvalue at or below ZERO_EIG * m * max lam is the solver's rounding of a zero (a rank-deficient S: duplicate captions)
    and is set to 0 with the negative ones: under the square root 1e-16 would come back as 1e-8, and m identical captions would not
    score exactly 0."""
    G = np.asarray(G, np.float64)
    m = int(G.shape[0])
    if m == 0:
        return float("nan")
    if m == 1:
        return 0.0
    lam = np.linalg.eigvalsh((G + G.T) / 20.0)
    top = float(lam.max())
    root = np.sqrt(np.where(lam > ZERO_EIG * m * top, lam, 0.0)) if top > 0.0 else np.zeros(m)
    total = float(root.sum())
    if total == 0.0 or float(root.max()) >= total:
        return 0.0
    return float(-math.log(float(root.max()) / total) / math.log(m))


def chunks(per, block_bytes):
    """Images 0 .. len(per) - 1 in consecutive chunks [b0, b1) whose [captions, ld] f32 block (ld: the chunk's longest list rounded
    up to 4) stays within block_bytes; a chunk holds at least one image.  -> [(b0, b1, ld), ...]"""
    out, b0, rows, longest = [], 0, 0, 0
    for b, n in enumerate(int(x) for x in per):
        big = max(longest, n)
        if b > b0 and (rows + n) * ((big + 3) // 4 * 4) * 4 > block_bytes:
            out.append((b0, b, (longest + 3) // 4 * 4))
            b0, rows, big = b, 0, n
        rows, longest = rows + n, big
    if len(per) > b0:
        out.append((b0, len(per), (longest + 3) // 4 * 4))
    return out


def _launch(lib, B, cand_img, max_cands, v, weight, gram, ld, mbr):
    """one vc_cider_gram call on an ngram_vectors table; cand_img / weight / gram / mbr: device pointers (ints) or None"""
    lib.vc_cider_gram(_stream(), int(B), cand_img, int(max_cands), P(v.off), P(v.nnz), P(v.keys), P(v.w), P(v.norm), P(v.words), weight,
                      gram, int(ld), mbr)


def _blocks(lib, dev, v, cand_img_dev, per, start, wdev, mbr_dev):
    """The chunk loop of gram_of_table and select_of_table: one vc_cider_gram call per chunk of `chunks(per, GRAM_BLOCK_BYTES)` into ONE
    device block that every chunk reuses.  Yields (b0, b1, ld, r0, n, block, base) after a chunk's launch: images b0 .. b1 - 1, table
    rows r0 .. r0 + n - 1, block[:n * ld] = their [n, ld] f32 rows, base = the `gram` pointer of the call (table row i lives at base +
    4 * i * ld with i the row's index in the WHOLE table: the chunk's block starts at row r0).  Chunks without captions are skipped."""
    parts = chunks(per, GRAM_BLOCK_BYTES)
    rows_max = max(int(start[b1] - start[b0]) * ld for b0, b1, ld in parts)
    block = torch.empty(max(1, rows_max), dtype=torch.float32, device=dev)
    for b0, b1, ld in parts:
        r0, n = int(start[b0]), int(start[b1] - start[b0])
        if n == 0:
            continue
        base = P(block) - 4 * r0 * ld
        _launch(lib, b1 - b0, P(cand_img_dev) + 4 * b0, int(per[b0:b1].max()), v, P(wdev), base, ld, P(mbr_dev))
        yield b0, b1, ld, r0, n, block, base


def _starts(per):
    per = np.asarray(per, np.int64)
    start = np.zeros(per.size + 1, np.int64)
    start[1:] = np.cumsum(per)
    return per, start


def gram_of_table(lib, dev, v, cand_img_dev, per, weights=None):
    """The matrices and means of every image of an idf-weighted ngram_vectors table `v`: image b owns rows sum(per[:b]) .. +per[b],
    cand_img_dev is the device int32 [B + 1] array of those offsets, weights a host float64 [C] array or None (uniform).
    -> (G: per image float32 [n_b, n_b], mbr: per image float64 [n_b]).  Images go in `chunks` of GRAM_BLOCK_BYTES; a row's bits do not
    depend on its chunk."""
    per, start = _starts(per)
    B, C = int(per.size), int(start[-1])
    if C == 0:
        return [np.zeros((0, 0), np.float32) for _ in range(B)], [np.zeros(0, np.float64) for _ in range(B)]
    wdev = None
    if weights is not None:
        wh = np.ascontiguousarray(weights, np.float64).reshape(-1)
        if wh.size != C:
            raise ValueError("%d weights for %d captions" % (wh.size, C))
        wdev = upload(dev, wh)
    mbr_dev = torch.empty(C, dtype=torch.float64, device=dev)
    G = [None] * B
    for b0, b1, ld, r0, n, block, _ in _blocks(lib, dev, v, cand_img_dev, per, start, wdev, mbr_dev):
        blk = block[:n * ld].cpu().numpy().reshape(n, ld)
        for b in range(b0, b1):
            G[b] = blk[start[b] - r0:start[b + 1] - r0, :per[b]].copy()
    for b in range(B):
        if G[b] is None:
            G[b] = np.zeros((0, 0), np.float32)
    m = mbr_dev.cpu().numpy()
    return G, [m[start[b]:start[b + 1]].copy() for b in range(B)]


def dpp_quality(keys, weight):
    """The qualities of one image's captions for the DPP selection from their ranking keys (higher = better): r_i = (key_i - min) /
    (max - min) over the image's finite keys -- 0 when they are all equal, 0 for a non-finite key -- and q_i = exp(weight * r_i), float64
    [m].  The best-ranked caption weighs e^weight times the worst; weight 0 gives all ones (selection on diversity alone)."""
    k = np.asarray(keys, np.float64).reshape(-1)
    r = np.zeros(k.size, np.float64)
    fin = np.isfinite(k)
    if fin.any():
        lo, hi = float(k[fin].min()), float(k[fin].max())
        if hi > lo:
            r[fin] = (k[fin] - lo) / (hi - lo)
    return np.exp(float(weight) * r)


def list_keys(entries):
    """The default keys of one image's ranked entries: the value the list is ordered by -- entry[1], or the fourth field of an entry
    that a `rerank` extended -- as a running minimum down the list.  For a list ordered by that value alone this IS the value; the
    ranked lists put <EOS>-ended captions before captions cut at max_len whatever their scores, and there a caption gets no better
    key than the captions ranked above it, so the list's first caption always has the largest quality.  (A NaN key is passed over.)"""
    k = np.array([e[3] if len(e) > 3 else e[1] for e in entries], np.float64)
    return np.fmin.accumulate(k) if k.size else k


def select_of_table(lib, dev, v, cand_img_dev, per, q, n):
    """vc_dpp_select_f64 over every image of an ngram_vectors table (arguments as gram_of_table's; q: host float64 [C], one finite
    positive quality per table row; n: 1..DPP_MAX_SELECT), on each chunk's device block right behind the vc_cider_gram call that wrote
    it: the matrices never reach the host.  -> (sel int32 [B, n]: indices within the image, -1 past min(n, n_b); gain float64 [B, n];
    n_dpp int32 [B]).  An image's results do not depend on its chunk."""
    per, start = _starts(per)
    B, C, n = int(per.size), int(start[-1]), int(n)
    if not 1 <= n <= DPP_MAX_SELECT:
        raise ValueError("n must be 1..%d (got %d)" % (DPP_MAX_SELECT, n))
    qh = np.ascontiguousarray(q, np.float64).reshape(-1)
    if qh.size != C:
        raise ValueError("%d qualities for %d captions" % (qh.size, C))
    if not (np.isfinite(qh) & (qh > 0)).all():
        raise ValueError("the qualities must be finite and > 0")
    sel, gain, n_dpp = np.full((B, n), -1, np.int32), np.zeros((B, n), np.float64), np.zeros(B, np.int32)
    if C == 0:
        return sel, gain, n_dpp
    qdev = upload(dev, qh)
    sel_d, gain_d, nd_d = (torch.empty(B * n, dtype=torch.int32, device=dev), torch.empty(B * n, dtype=torch.float64, device=dev),
                           torch.empty(B, dtype=torch.int32, device=dev))
    done = np.zeros(B, bool)
    for b0, b1, ld, r0, rows, block, base in _blocks(lib, dev, v, cand_img_dev, per, start, None, None):
        lib.vc_dpp_select_f64(_stream(), b1 - b0, P(cand_img_dev) + 4 * b0, int(per[b0:b1].max()), base, ld, P(qdev), n, P(sel_d) + 4 * b0 * n,
                              P(gain_d) + 8 * b0 * n, P(nd_d) + 4 * b0)
        done[b0:b1] = True
    if done.any():   # (images of a chunk without captions keep -1 / 0 / 0: the kernel's own answer for n_b = 0)
        sel[done], gain[done], n_dpp[done] = (sel_d.cpu().numpy().reshape(B, n)[done], gain_d.cpu().numpy().reshape(B, n)[done],
                                              nd_d.cpu().numpy()[done])
    return sel, gain, n_dpp


class CiderGram(object):
    """lib_or_engine: the C-ABI library (abi.load()) or a CaptionEngine (its library and device).  corpus_captions_per_image: per
    image a list of token lists, the document frequencies' corpus (scst.corpus_df).  df_table = (df_keys, idf, n_df, idf_unseen) hands
    in a df / idf table that already lives on the device (CaptionEvaluator passes its own); the corpus is then not needed."""

    def __init__(self, lib_or_engine, corpus_captions_per_image, bos, eos, vocab_size=None, df_table=None):
        self.lib, self.dev = library_and_device(lib_or_engine)
        self.bos, self.eos = int(bos), int(eos)
        if df_table is not None:
            self.df_keys, self.idf, self.n_df, self.idf_unseen = df_table
            self.D = None
            return
        from .scst import corpus_df
        df_keys, idf, self.idf_unseen = corpus_df(corpus_captions_per_image, bos, eos, vocab_size)
        self.D = len(corpus_captions_per_image)
        self.n_df = int(df_keys.size)
        self.df_keys = upload(self.dev, df_keys.view(np.int64) if self.n_df else np.zeros(1, np.int64))
        self.idf = upload(self.dev, idf if self.n_df else np.zeros(1, np.float32))

    def _rows(self, candidates_per_image):
        """host side of the caption table: -> (per: captions per image, cand_img [B + 1], flat: the captions in table order, W, L: their
        word rows), limits checked"""
        B = len(candidates_per_image)
        per = np.fromiter((len(c) for c in candidates_per_image), np.int64, B)
        if B and per.max() > DIVERSE_MAX_DRAWS:
            raise ValueError("at most %d candidates per image (DIVERSE_MAX_DRAWS; got %d)" % (DIVERSE_MAX_DRAWS, per.max()))
        cand_img = np.zeros(B + 1, np.int64)
        cand_img[1:] = np.cumsum(per)
        image_of = np.repeat(np.arange(B), per)
        flat = [c for cs in candidates_per_image for c in cs]
        W, L = word_rows(flat, self.bos, self.eos, owner=lambda i: "candidate %d of image %d" % (i - cand_img[image_of[i]], image_of[i]))
        return per, cand_img, flat, W, L

    def _vectors(self, cand_img, W, L):
        """the idf-weighted ngram_vectors table of the word rows; v.head = the device cand_img"""
        return ngram_vectors(self.lib, self.dev, W, L, self.bos, self.eos, self.df_keys, self.idf, self.n_df, self.idf_unseen, head=cand_img)

    def gram(self, candidates_per_image, weights=None):
        """candidates_per_image: per image a list of token lists (<= 256); weights: per image a list of one number per caption (None:
        uniform).  -> (G, mbr): per image a float32 [n_b, n_b] array, G[i][j] = CIDEr-D(caption i, reference caption j), and a float64
        [n_b] array, mbr[i] = sum_j w_j G[i][j] / sum_j w_j (0.0 when the weights sum to 0).  An empty list gives (0, 0) / (0,) arrays."""
        per, cand_img, flat, W, L = self._rows(candidates_per_image)
        wh = None
        if weights is not None:
            if len(weights) != len(per) or any(len(w) != n for w, n in zip(weights, per)):
                raise ValueError("weights must hold one number per caption of every image")
            wh = np.fromiter((float(x) for w in weights for x in w), np.float64, len(flat))
        if not flat:
            return gram_of_table(self.lib, self.dev, None, None, per)
        v = self._vectors(cand_img, W, L)
        return gram_of_table(self.lib, self.dev, v, v.head, per, wh)

    def rerank(self, diverse_result, weights=None, n_best=None):
        """diverse_result: per image [(tokens, score, count), ...] in likelihood order.  -> per image [(tokens, score, count, mbr), ...]
        by mbr, highest first (exact ties keep the likelihood order), the first n_best of them (None: all).  weights=None: an entry's
        weight is its count -- the evidence is all K draws, not the distinct captions."""
        if weights is None:
            weights = [[float(e[2]) for e in entries] for entries in diverse_result]
        _, mbr = self.gram([[e[0] for e in entries] for entries in diverse_result], weights)
        return [rerank_entries(entries, m, n_best) for entries, m in zip(diverse_result, mbr)]

    def select(self, diverse_result, n, quality=1.0, keys=None, weights=None):
        """DPP selection (DESIGN.md "DPP selection"): n of every image's captions chosen jointly for quality and for difference from each
        other by vc_dpp_select_f64 over the image's in-set CIDEr-D matrix, which stays on the device.
        diverse_result: per image its ranked entries (tokens, score, ...), at most 256.  An entry's key is the value its list is ordered
        by (`list_keys`: entry[1], or the fourth field of an entry that a `rerank` extended) unless `keys` gives one number per caption
        of every image; its quality is dpp_quality(the image's keys, quality).  `weights` (per image one finite positive number per caption) gives
        the qualities themselves, in place of keys and quality.
        -> (selected: per image the chosen entries in selection order, each extended by its gain -- at most n, fewer for a shorter
        list; n_dpp: per image how many of them the greedy steps chose, the rest being the fill in list order with gain 0)."""
        B = len(diverse_result)
        if keys is not None and weights is not None:
            raise ValueError("give keys or weights, not both")
        given = weights if weights is not None else keys
        if given is not None and (len(given) != B or any(len(g) != len(e) for g, e in zip(given, diverse_result))):
            raise ValueError("%s must hold one number per caption of every image" % ("weights" if weights is not None else "keys"))
        if weights is not None:
            qs = [np.asarray(w, np.float64).reshape(-1) for w in weights]
        else:
            if keys is None:
                keys = [list_keys(entries) for entries in diverse_result]
            qs = [dpp_quality(k, quality) for k in keys]
        per, cand_img, flat, W, L = self._rows([[e[0] for e in entries] for entries in diverse_result])
        q = np.concatenate(qs) if qs else np.zeros(0, np.float64)
        v = self._vectors(cand_img, W, L) if flat else None
        sel, gain, n_dpp = select_of_table(self.lib, self.dev, v, v.head if flat else None, per, q, n)
        out = [[tuple(entries[j]) + (float(g),) for j, g in zip(row.tolist(), gr.tolist()) if j >= 0] for entries, row, gr in zip(diverse_result, sel, gain)]
        return out, [int(x) for x in n_dpp]
