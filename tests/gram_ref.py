"""Float64 reference of the in-set CIDEr-D matrix, its weighted means and Self-CIDEr (tests only), written from the definitions of
vae_captioning_amd/mbr.py on top of consensus_ref's vectors and pair score.

G[i][j] = CIDEr-D(hypothesis = caption i, reference = caption j of the same image); mbr[i] = sum_j w_j G[i][j] / sum_j w_j (0 when the
weights sum to 0); self_cider(G) = -log_m(sqrt(max lam) / sum sqrt(lam)) over the eigenvalues lam of (G + G^T) / 20, negative ones
and those within eps * m * max lam of zero set to 0."""
import math

import numpy as np

from . import consensus_ref as cref
from . import eval_ref


def gram(caps, idf, unseen, bos=1, eos=2):
    """caps: one image's token lists; idf / unseen: consensus_ref.df_idf's table -> float64 [n, n]"""
    vec = [cref.vector(c, bos, eos, idf, unseen) for c in caps]
    G = np.zeros((len(caps), len(caps)), np.float64)
    for i, h in enumerate(vec):
        for j, r in enumerate(vec):
            G[i, j] = cref.cider_d(h, r)
    return G


def gram_rows(caps, rows, idf, unseen, bos=1, eos=2):
    """the given rows of gram() only (a 256-caption image costs 65 536 pairs in full)"""
    vec = [cref.vector(c, bos, eos, idf, unseen) for c in caps]
    return np.array([[cref.cider_d(vec[i], r) for r in vec] for i in rows], np.float64).reshape(len(rows), len(caps))


def orders(caption, idf, unseen, bos=1, eos=2):
    """the number of orders n = 1..4 in which the caption's vector has a non-zero norm"""
    return sum(1 for n in cref.vector(caption, bos, eos, idf, unseen)[2] if n > 0)


def mbr(G, weights=None):
    G = np.asarray(G, np.float64)
    w = np.ones(G.shape[0]) if weights is None else np.asarray(weights, np.float64)
    total = math.fsum(w.tolist())
    if G.shape[0] == 0 or total == 0:
        return np.zeros(G.shape[0], np.float64)
    return np.array([math.fsum((w * row).tolist()) / total for row in G], np.float64)


def self_cider(G):
    G = np.asarray(G, np.float64)
    m = G.shape[0]
    if m == 0:
        return float("nan")
    if m == 1:
        return 0.0
    lam = np.linalg.eigvalsh((G + G.T) / 20.0)
    lam[lam <= np.finfo(np.float64).eps * m * max(lam.max(), 0.0)] = 0.0     # negative values, and the solver's roundings of a zero
    s = np.sqrt(lam)
    if s.sum() == 0 or s.max() >= s.sum():
        return 0.0
    return float(-math.log(s.max() / s.sum()) / math.log(m))


def eigenvalues(G):
    """ascending eigenvalues of the symmetrised matrix (what a test inspects to keep away from small non-structural ones)"""
    G = np.asarray(G, np.float64)
    return np.linalg.eigvalsh((G + G.T) / 20.0)


def evaluate(candidates, references, bos, eos):
    """the two set metrics of CaptionEvaluator.evaluate(self_cider=True): idf over the references (as eval_ref.cider_scores), uniform
    weights, the first maximum of mbr.  -> dict(self_cider, mbr_cider_d, per_image=dict(self_cider, mbr_choice, caption_mbr, gram))"""
    idf, unseen = cref.df_idf(references, bos, eos)
    cider = eval_ref.cider_scores(candidates, references, bos, eos)
    Gs = [gram(cs, idf, unseen, bos, eos) for cs in candidates]
    mb = [mbr(G) for G in Gs]
    sc = np.array([self_cider(G) for G in Gs], np.float64)
    choice = np.array([int(np.argmax(m)) if len(m) else -1 for m in mb])
    have = [b for b, cs in enumerate(candidates) if cs]
    return dict(self_cider=float(np.mean(sc[have])) if have else 0.0,
                mbr_cider_d=float(np.mean([cider[b][choice[b]] for b in have])) if have else 0.0,
                per_image=dict(self_cider=sc, mbr_choice=choice, caption_mbr=mb, gram=Gs))
