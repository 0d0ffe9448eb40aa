"""Consensus re-ranking of diverse captions (Devlin et al., 2015, "Exploring Nearest Neighbor Approaches for Image Captioning").

`CaptionGenerator.diverse()` ranks an image's candidate captions by length-normalised log-likelihood, which favours short, generic
captions.  A `ConsensusIndex` holds the training images (fc2 feature row + human captions) and re-ranks the candidates on the GPU:

1. the query image's k nearest index images by cosine of their fc2 features (ties: lower index first);
2. their human captions, pooled in neighbour order;
3. each candidate scored by the float64 mean of its m' = min(m, |pool|) largest CIDEr-D values against the pool (coco-caption's
   CIDEr-D with one reference, sigma = 6, document frequencies over the index IMAGES); highest first, exact ties keep the likelihood
   order.

Words are token ids without <BOS>, <EOS> and PAD (0), at most 64 per caption, ids <= 65535; an n-gram (n = 1..4) is the 64-bit key
of its ids packed 16 bits each, last word in the low bits.  The df / idf table is built here with numpy (idf = log D - log max(1, df)
in float64, stored float32; unseen n-grams get log D); everything else runs in csrc/consensus.hip and vc_gemm_f32.
"""
import itertools
import types

import numpy as np
import torch

from .abi import ptr as P
from .engine import _stream
from .generate import DIVERSE_MAX_DRAWS

MAX_K = 256          # neighbours per query (vc_topk_rows_wide_f32, vc_consensus_score)
MAX_POOL = 2048      # pool captions per query (vc_consensus_score stages them in LDS)
MAX_WORDS = 64       # words per caption (vc_ngram_vectors: one wave per caption)
MAX_ID = 65535       # token ids fit 16 bits of a key
BLOCK_BYTES = 1 << 30   # the [queries, D] f32 similarity block of one pass stays under this


def check_limits(k, m):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError("consensus k must be 1..%d (got %d)" % (MAX_K, k))
    if int(m) < 1:
        raise ValueError("consensus m must be >= 1 (got %d)" % m)


def ngram_key(ids):
    """64-bit key of an n-gram (1 <= n <= 4 ids, each 1..65535): 16 bits per id, the last id in the low bits."""
    if not 1 <= len(ids) <= 4:
        raise ValueError("n-grams have 1..4 words")
    key = 0
    for w in ids:
        if not 1 <= int(w) <= MAX_ID:
            raise ValueError("token id %d outside 1..%d" % (w, MAX_ID))
        key = (key << 16) | int(w)
    return key


def unpack_key(key):
    """ids of an n-gram key (inverse of ngram_key)"""
    key, out = int(key), []
    while key:
        out.append(key & 0xFFFF)
        key >>= 16
    return out[::-1]


def capacity(words):
    """key slots of captions with `words` words: sum over n = 1..4 of max(0, L - n + 1)"""
    L = np.asarray(words, np.int64)
    return sum(np.maximum(0, L - n + 1) for n in range(1, 5))


def word_rows(seqs, bos, eos, owner=None):
    """Token lists -> (W [n, Lw] int32 words left-aligned and 0-padded, L [n] words per row).  Words drop <BOS>, <EOS> and PAD.
    owner(i): the name of row i in error messages.  Raises ValueError for ids above 65535 and captions of more than 64 words."""
    n = len(seqs)
    lens = np.fromiter(map(len, seqs), np.int64, n)
    T = np.zeros((n, max(1, int(lens.max()) if n else 1)), np.int64)
    T[np.arange(T.shape[1])[None, :] < lens[:, None]] = np.fromiter(itertools.chain.from_iterable(seqs), np.int64, int(lens.sum()))
    keep = (T != 0) & (T != int(bos)) & (T != int(eos))
    bad = keep & ((T > MAX_ID) | (T < 0))
    if bad.any():
        r = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError("token id %d outside 1..%d (a vocabulary of at most 65535 ids): %s"
                         % (T[r][bad[r]][0], MAX_ID, owner(r) if owner else "row %d" % r))
    L = keep.sum(axis=1)
    if n and L.max() > MAX_WORDS:
        i = int(np.argmax(L))
        raise ValueError("%s has %d words (at most %d)" % (owner(i) if owner else "row %d" % i, L[i], MAX_WORDS))
    W = np.zeros((n, max(1, int(L.max()) if n else 1)), np.int32)
    W[np.arange(W.shape[1])[None, :] < L[:, None]] = T[keep]     # (row-major on both sides: each row's words in order)
    return W, L


def ngram_keys(W, L, chunk=65536):
    """-> (keys uint64, row) of every n-gram occurrence (n = 1..4) of the rows of W, row-major (rows ascending)."""
    ks, rs = [], []
    for r0 in range(0, W.shape[0], chunk):
        w = W[r0:r0 + chunk].astype(np.uint64)
        lc = L[r0:r0 + chunk]
        parts, valid = [], []
        for n in range(1, 5):
            width = w.shape[1] - n + 1
            if width <= 0:
                continue
            key = np.zeros((w.shape[0], width), np.uint64)
            for j in range(n):
                key = (key << np.uint64(16)) | w[:, j:j + width]
            parts.append(key)
            valid.append(np.arange(width)[None, :] < (lc[:, None] - n + 1))
        K, V = np.concatenate(parts, axis=1), np.concatenate(valid, axis=1)
        ks.append(K[V])
        rs.append(np.broadcast_to(np.arange(r0, r0 + w.shape[0])[:, None], K.shape)[V])
    if not ks:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    return np.concatenate(ks), np.concatenate(rs)


def df_table(W, L, image_of_row, D):
    """Sorted distinct n-gram keys of the index and their idf = log D - log max(1, df) (float64, stored float32), df = the number of
    index IMAGES with the n-gram in at least one of their captions."""
    keys, rows = ngram_keys(W, L)
    img = np.asarray(image_of_row, np.int64)[rows]
    order = np.lexsort((img, keys))
    ks, im = keys[order], img[order]
    new = np.ones(ks.size, bool)
    new[1:] = (ks[1:] != ks[:-1]) | (im[1:] != im[:-1])
    pk = ks[new]                                     # one entry per (n-gram, image)
    first = np.ones(pk.size, bool)
    first[1:] = pk[1:] != pk[:-1]
    starts = np.flatnonzero(first)
    df = np.diff(np.append(starts, pk.size))
    idf = (np.log(float(D)) - np.log(np.maximum(1, df).astype(np.float64))).astype(np.float32)
    return pk[first], idf


def host_index(captions, bos, eos, vocab_size=None):
    """Host half of an index build: the words of every caption (W, L), per image caption offsets, and the df / idf table.
    captions: per image a list of token lists (at least one).  Every limit is checked here, before anything reaches the device."""
    if vocab_size is not None and int(vocab_size) > MAX_ID + 1:
        raise ValueError("vocabulary of %d ids: consensus keys hold ids up to %d (a vocabulary of at most %d)" % (vocab_size, MAX_ID, MAX_ID + 1))
    D = len(captions)
    if D == 0:
        raise ValueError("the consensus index needs at least one image")
    per = np.fromiter((len(c) for c in captions), np.int64, D)
    if per.min() < 1:
        raise ValueError("index image %d has no caption" % int(np.argmin(per)))
    img_cap = np.zeros(D + 1, np.int64)
    img_cap[1:] = np.cumsum(per)
    image_of = np.repeat(np.arange(D), per)
    flat = [c for caps in captions for c in caps]
    W, L = word_rows(flat, bos, eos, owner=lambda i: "caption %d of index image %d" % (i - img_cap[image_of[i]], image_of[i]))
    df_keys, idf = df_table(W, L, image_of, D)
    return types.SimpleNamespace(D=D, W=W, L=L, img_cap=img_cap, per_image=per, df_keys=df_keys, idf=idf,
                                 idf_unseen=np.float32(np.log(float(D))))


def upload(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ngram_vectors(lib, dev, W, L, bos, eos, df_keys, idf, n_df, idf_unseen, head=None):
    """n-gram vectors of word rows (vc_ngram_vectors), CSR by capacity(L), weighted by the device df / idf table given (n_df = 0: every
    n-gram gets idf_unseen).  The host inputs go up in one copy; head: an int32 array sent along (v.head is its device copy).  The
    uploaded word rows stay reachable: v.tok [n, v.ld] int32 and v.len [n] (what vc_lcs_overlap reads)."""
    n = int(W.shape[0])
    cap = capacity(L)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(cap)
    if off[-1] >= 2 ** 31:
        raise ValueError("%d n-gram slots: more than an int32 CSR offset holds" % off[-1])
    head = np.zeros(0, np.int32) if head is None else np.asarray(head, np.int32)
    h, o1, o2 = head.size, head.size + n + 1, head.size + 2 * n + 1
    up = upload(dev, np.concatenate([head, off.astype(np.int32), np.asarray(L, np.int32), W.astype(np.int32).reshape(-1)]))
    total = max(1, int(off[-1]))
    v = types.SimpleNamespace(n=n, head=up[:h], off=up[h:o1], keys=torch.empty(total, dtype=torch.int64, device=dev),
                              w=torch.empty(total, dtype=torch.float32, device=dev),
                              nnz=torch.empty(max(1, n), dtype=torch.int32, device=dev),
                              norm=torch.empty((max(1, n), 4), dtype=torch.float32, device=dev),
                              words=torch.empty(max(1, n), dtype=torch.int32, device=dev),
                              tok=up[o2:], ld=int(W.shape[1]), len=up[o1:o2])
    if n:
        lib.vc_ngram_vectors(_stream(), P(up[o2:]), n, int(W.shape[1]), P(up[o1:o2]), int(bos), int(eos), P(df_keys), P(idf), int(n_df),
                             float(idf_unseen), P(v.off), P(v.keys), P(v.w), P(v.nnz), P(v.norm), P(v.words))
    return v


def library_and_device(lib_or_engine):
    """(library, device) of the C-ABI library (abi.load(): the current device) or of a CaptionEngine"""
    if hasattr(lib_or_engine, "lib") and hasattr(lib_or_engine, "dev"):
        return lib_or_engine.lib, lib_or_engine.dev
    return lib_or_engine, torch.device("cuda", torch.cuda.current_device())


def rerank_entries(entries, consensus, n_best=None):
    """(tokens, score, count) entries in likelihood order + their consensus scores -> (tokens, score, count, consensus) by consensus,
    highest first; exact ties keep the likelihood order.  n_best: keep the first n_best (None: all)."""
    c = np.asarray(consensus, np.float64)
    order = np.argsort(-c, kind="stable").tolist()
    cl = c.tolist()
    out = [(entries[j][0], entries[j][1], entries[j][2], cl[j]) for j in order]
    return out if n_best is None else out[:int(n_best)]


def _training_names(gen):
    """base file names of the training images of a Batch_Generator: `_iterable` without the held-out `unused_cap_in` images"""
    held = set(gen.unused_cap_in or ())
    return [name.split("/")[-1] for name in gen._iterable if name not in held]


def captions_from_generator(gen):
    """per training image of a Batch_Generator its token lists, looked up through `_lookup` so that repartitioned validation images
    come from val_captions; no features are read.  Host only."""
    return [[list(c) for c in gen._lookup(gen.captions or {}, gen.val_captions, base)] for base in _training_names(gen)]


def index_data_from_generator(gen):
    """(features [D, F] float32, captions: per image its token lists) of the training images of a Batch_Generator: `_iterable`
    walked through `_lookup`, so repartitioned validation images come from val_feature_dict / val_captions.  The held-out
    `unused_cap_in` images are never included.  Host only."""
    if not gen.feature_dict:
        raise ValueError("the consensus index needs precomputed fc2 features (a Batch_Generator with a feature_dict)")
    feats = [np.asarray(gen._lookup(gen.feature_dict, gen.val_feature_dict, base), np.float32).reshape(-1) for base in _training_names(gen)]
    return np.stack(feats), captions_from_generator(gen)


def references_from_generator(gen):
    """{image id: EVERY human caption (token list) of the image} for the images a Batch_Generator iterates over, keyed by the ids
    next_val_batch(get_image_ids=True) yields.  (The batches themselves carry ONE randomly drawn caption per image.)  Host only."""
    out = {}
    for name in gen._iterable:
        base = name.split("/")[-1]
        out[gen._imid([name])[0]] = [list(c) for c in gen._lookup(gen.captions or {}, gen.val_captions, base)]
    return out


class ConsensusIndex(object):
    """Index of D images for consensus re-ranking.  lib_or_engine: the C-ABI library (abi.load()) or a CaptionEngine (its library
    and device).  features [D, F] (host array or device tensor); captions: per image a list of token lists."""

    def __init__(self, lib_or_engine, features, captions, bos, eos, k=90, m=125, vocab_size=None):
        self.lib, self.dev = library_and_device(lib_or_engine)
        check_limits(k, m)
        self.k, self.m, self.bos, self.eos = int(k), int(m), int(bos), int(eos)
        if len(features) != len(captions):
            raise ValueError("features has %d rows for %d images of captions" % (len(features), len(captions)))
        h = host_index(captions, bos, eos, vocab_size)
        if self.k > h.D:
            raise ValueError("consensus k = %d exceeds the %d index images" % (self.k, h.D))
        if self.k * int(h.per_image.max()) > MAX_POOL:
            raise ValueError("pool limit: k = %d neighbours with up to %d captions each can exceed %d pool captions"
                             % (self.k, h.per_image.max(), MAX_POOL))
        self.D = h.D
        self.block_bytes = BLOCK_BYTES
        st = _stream()
        f = self._dev_f32(features)
        self.F = int(f.shape[1])
        self.feat = torch.empty((self.D, self.F), dtype=torch.float32, device=self.dev)
        self.lib.vc_l2_normalize_rows_f32(st, P(f), self.D, self.F, self.F, P(self.feat), self.F)
        del f
        self.n_df = int(h.df_keys.size)
        self.df_keys = self._up(h.df_keys.view(np.int64) if self.n_df else np.zeros(1, np.int64))
        self.idf = self._up(h.idf if self.n_df else np.zeros(1, np.float32))
        self.idf_unseen = float(h.idf_unseen)
        self.img_cap = self._up(h.img_cap.astype(np.int32))
        self.caps = self._vectors(h.W, h.L)
        self.n_captions = int(h.L.size)

    # ------------------------------------------------------------------ plumbing
    def _up(self, a):
        return upload(self.dev, a)

    def _dev_f32(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(self.dev, torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)

    def _vectors(self, W, L, head=None):
        """n-gram vectors of word rows under the index's df / idf table (ngram_vectors above)"""
        return ngram_vectors(self.lib, self.dev, W, L, self.bos, self.eos, self.df_keys, self.idf, self.n_df, self.idf_unseen, head)

    def _exclude(self, exclude, B):
        if exclude is None:
            return None
        ex = np.asarray(exclude.cpu() if isinstance(exclude, torch.Tensor) else exclude, np.int64).reshape(-1)
        if ex.size != B or ex.min() < -1 or ex.max() >= self.D:
            raise ValueError("exclude must hold one index row (or -1) per query")
        if (ex >= 0).any() and self.k > self.D - 1:
            raise ValueError("consensus k = %d exceeds the %d index images left after the exclusion" % (self.k, self.D - 1))
        return self._up(ex.astype(np.int32))

    def _neighbours_dev(self, features, exclude=None):
        lib, st = self.lib, _stream()
        q = self._dev_f32(features)
        if q.dim() != 2 or q.shape[1] != self.F:
            raise ValueError("query features must be [B, %d]" % self.F)
        B, D, F, k = int(q.shape[0]), self.D, self.F, self.k
        ex = self._exclude(exclude, B)
        ids = torch.empty((B, k), dtype=torch.int32, device=self.dev)
        cos = torch.empty((B, k), dtype=torch.float32, device=self.dev)
        if B == 0:
            return ids, cos
        qn = torch.empty_like(q)   # (q may be the caller's own tensor)
        lib.vc_l2_normalize_rows_f32(st, P(q), B, F, F, P(qn), F)
        q = qn
        Dp = (D + 3) // 4 * 4
        rows = max(1, min(B, self.block_bytes // (4 * Dp)))
        if rows < B and rows >= 128:
            rows = rows // 128 * 128   # full passes of whole 128-row tiles: every full pass runs the same GEMM plan
        S = torch.empty((rows, Dp), dtype=torch.float32, device=self.dev)
        gws = max(lib.vc_gemm_workspace_bytes(rows, D, F), lib.vc_gemm_workspace_bytes(B - (B - 1) // rows * rows, D, F))
        tws = lib.vc_topk_rows_wide_workspace_bytes(rows, D, k)
        ws = torch.empty(max(1, (gws + tws + 255) // 4 + 64), dtype=torch.float32, device=self.dev)
        gp, tp = P(ws), P(ws) + (gws + 255) // 256 * 256
        for q0 in range(0, B, rows):
            n = min(rows, B - q0)
            lib.vc_gemm_f32(st, 0, 1, n, D, F, P(q) + q0 * F * 4, F, P(self.feat), F, P(S), Dp, None, 0, gp, gws)
            lib.vc_topk_rows_wide_f32(st, P(S), n, D, Dp, k, P(ex) + q0 * 4 if ex is not None else None, P(cos) + q0 * k * 4,
                                      P(ids) + q0 * k * 4, tp, tws)
        return ids, cos

    # ------------------------------------------------------------------ public
    def neighbours(self, features, exclude=None):
        """-> (ids int32 [B, k], cos float32 [B, k]): the k nearest index images of each query under (cosine descending, index
        ascending); cosine 0 for zero feature rows.  exclude[b] (-1: none) drops that index row for query b."""
        ids, cos = self._neighbours_dev(features, exclude)
        return ids.cpu().numpy(), cos.cpu().numpy()

    def score(self, features, candidates, exclude=None):
        """candidates: per query image a list of token lists (<= 256).  -> per image a float64 array: each candidate's consensus,
        the mean of its m' = min(m, |pool|) largest CIDEr-D values against the captions of the image's k neighbours."""
        B = len(candidates)
        if int(features.shape[0]) != B:
            raise ValueError("%d feature rows for %d images of candidates" % (features.shape[0], B))
        per = np.fromiter((len(c) for c in candidates), np.int64, B)
        if B and per.max() > DIVERSE_MAX_DRAWS:
            raise ValueError("at most %d candidates per image (DIVERSE_MAX_DRAWS; got %d)" % (DIVERSE_MAX_DRAWS, per.max()))
        cand_img = np.zeros(B + 1, np.int64)
        cand_img[1:] = np.cumsum(per)
        image_of = np.repeat(np.arange(B), per)
        flat = [c for cs in candidates for c in cs]
        W, L = word_rows(flat, self.bos, self.eos, owner=lambda i: "candidate %d of image %d" % (i - cand_img[image_of[i]], image_of[i]))
        ids, _ = self._neighbours_dev(features, exclude)
        if not flat:
            return [np.zeros(0, np.float64) for _ in range(B)]
        cv, rv = self._vectors(W, L, head=cand_img), self.caps
        out = torch.empty(len(flat), dtype=torch.float64, device=self.dev)
        self.lib.vc_consensus_score(_stream(), B, self.k, P(ids), P(self.img_cap), P(rv.off), P(rv.nnz), P(rv.keys), P(rv.w), P(rv.norm),
                                    P(rv.words), P(cv.head), int(per.max()), P(cv.off), P(cv.nnz), P(cv.keys),
                                    P(cv.w), P(cv.norm), P(cv.words), self.m, P(out))
        s = out.cpu().numpy()
        return [s[cand_img[b]:cand_img[b + 1]].copy() for b in range(B)]

    def rerank(self, features, diverse_result, exclude=None, n_best=None):
        """diverse_result: CaptionGenerator.diverse() output (per image [(tokens, score, count), ...] in likelihood order).  -> per
        image [(tokens, score, count, consensus), ...] by consensus, highest first (exact ties keep the likelihood order), the first
        n_best of them (None: all)."""
        cons = self.score(features, [[e[0] for e in entries] for entries in diverse_result], exclude)
        return [rerank_entries(entries, c, n_best) for entries, c in zip(diverse_result, cons)]
