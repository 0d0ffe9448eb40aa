"""Float64 reference of consensus re-ranking (tests only), written from the definitions: words = token ids without <BOS>, <EOS> and
PAD; n-grams n = 1..4; df over index IMAGES; idf = log D - log max(1, df) in float64 stored float32 (unseen: log D); v_n(s)[g] =
count * idf in f32; CIDEr-D(c, r) = 10 exp(-(L(c) - L(r))^2 / 72) / 4 sum_n sum_g min(c_g, r_g) r_g / (|c_n| |r_n|); consensus = mean of
the m' largest CIDEr-D over the pool of the k nearest index images' captions (cosine descending, index ascending)."""
import math
from collections import Counter

import numpy as np


def words(tokens, bos, eos):
    return [int(t) for t in tokens if int(t) not in (0, bos, eos)]


def key(gram):
    k = 0
    for w in gram:
        k = (k << 16) | int(w)
    return k


def ngram_counts(ws):
    """{n: Counter(key -> count)} for n = 1..4"""
    return {n: Counter(key(ws[i:i + n]) for i in range(len(ws) - n + 1)) for n in range(1, 5)}


def df_idf(captions, bos, eos):
    """captions: per image its token lists -> ({key: float32 idf}, float32 idf of an unseen n-gram)"""
    D = len(captions)
    df = Counter()
    for caps in captions:
        seen = set()
        for c in caps:
            for cnt in ngram_counts(words(c, bos, eos)).values():
                seen.update(cnt)
        df.update(seen)
    idf = {g: np.float32(math.log(D) - math.log(max(1, d))) for g, d in df.items()}
    return idf, np.float32(math.log(D))


def vector(tokens, bos, eos, idf, unseen):
    """-> (L, {n: {key: float32 weight}}, [|v_n| float64])"""
    ws = words(tokens, bos, eos)
    vec = {n: {g: np.float32(c) * idf.get(g, unseen) for g, c in cnt.items()} for n, cnt in ngram_counts(ws).items()}
    norms = [math.sqrt(sum(float(w) ** 2 for w in vec[n].values())) for n in range(1, 5)]
    return len(ws), vec, norms


def cider_d(c, r):
    """c, r: outputs of vector()"""
    (lc, vc, nc), (lr, vr, nr) = c, r
    s = 0.0
    for n in range(1, 5):
        if nc[n - 1] == 0 or nr[n - 1] == 0:
            continue
        s += sum(min(float(vc[n].get(g, 0.0)), float(w)) * float(w) for g, w in vr[n].items()) / (nc[n - 1] * nr[n - 1])
    return 10.0 * math.exp(-((lc - lr) ** 2) / 72.0) * s / 4.0


def consensus(cand_vecs, pool_vecs, m):
    out = []
    for c in cand_vecs:
        sc = sorted((cider_d(c, r) for r in pool_vecs), reverse=True)
        mm = min(m, len(sc))
        out.append(float(np.mean(sc[:mm])) if mm else 0.0)
    return np.array(out, np.float64)


def cosines(Q, X):
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    nq, nx = np.linalg.norm(Q, axis=1), np.linalg.norm(X, axis=1)
    C = Q @ X.T
    den = nq[:, None] * nx[None, :]
    return np.where(den > 0, C / np.where(den > 0, den, 1.0), 0.0)


def topk_order(row, k, exclude=-1):
    """indices of the first k entries under (value descending, index ascending), column `exclude` dropped"""
    idx = np.arange(row.size)
    keep = idx != exclude
    idx, vals = idx[keep], row[keep]
    o = np.lexsort((idx, -vals))
    return idx[o[:k]]
