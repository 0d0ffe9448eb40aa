"""Plain-Python reference of caption-set evaluation (tests only), written from the definitions: words = token ids without <BOS>, <EOS>
and PAD; n-grams n = 1..4 as tuples in Counters.  For hypothesis counts c_g and m_g = the largest count of g over the references:
total_n = sum c_g, match_n = sum min(c_g, m_g), distinct_n = |{g}|, unseen_n = |{g: m_g = 0}|, ref_len = the reference length minimising
(|L_r - L_c|, L_r) (0 without references).  BLEU_n = BP * exp(mean_{i <= n} log(sum match_i / sum total_i)), BP = 1 if C >= R else
exp(1 - R / C), 0.0 when a p_i is 0 or C is 0.  CIDEr-D comes from tests/consensus_ref.py.  Nothing here imports the product's arithmetic."""
import functools
import math
from collections import Counter

import numpy as np

from . import consensus_ref as cref

words = cref.words


@functools.lru_cache(maxsize=1 << 16)
def _grams(ws, n):
    return Counter(ws[i:i + n] for i in range(len(ws) - n + 1))


def grams(ws, n):
    """Counter of the n-grams (tuples) of a word list; cached per word sequence, so never change the result"""
    return _grams(tuple(ws), n)


def overlap(hyp, refs):
    """hyp: a word list, refs: word lists -> dict(total, match, distinct, unseen: lists of 4 ints; ref_len: int)"""
    out = dict(total=[], match=[], distinct=[], unseen=[], ref_len=0)
    for n in range(1, 5):
        c = grams(hyp, n)
        rc = [grams(r, n) for r in refs]
        m = {g: max([r[g] for r in rc] or [0]) for g in c}
        out["total"].append(sum(c.values()))
        out["match"].append(sum(min(v, m[g]) for g, v in c.items()))
        out["distinct"].append(len(c))
        out["unseen"].append(sum(1 for g in c if m[g] == 0))
    if refs:
        out["ref_len"] = min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]
    return out


def corpus_bleu(match, total, hyp_len, ref_len):
    """match, total: the four sums over the hypotheses; -> [BLEU_1 .. BLEU_4]"""
    if hyp_len == 0:
        return [0.0] * 4
    bp = 1.0 if hyp_len >= ref_len else math.exp(1.0 - ref_len / hyp_len)
    out, logs = [], []
    for n in range(4):
        if total[n] == 0 or match[n] == 0:
            logs.append(None)
        else:
            logs.append(math.log(match[n] / total[n]))
        out.append(0.0 if None in logs else bp * math.exp(sum(logs) / (n + 1)))
    return out


def bleu_of(pairs):
    """pairs: (hypothesis words, reference word lists) -> corpus [BLEU_1 .. BLEU_4]"""
    match, total, C, R = [0] * 4, [0] * 4, 0, 0
    for h, refs in pairs:
        o = overlap(h, refs)
        for n in range(4):
            match[n] += o["match"][n]
            total[n] += o["total"][n]
        C += len(h)
        R += o["ref_len"]
    return corpus_bleu(match, total, C, R)


def cider_scores(candidates, references, bos, eos):
    """per image a float64 array: each candidate's mean over the image's references of consensus_ref.cider_d, idf over the references"""
    idf, unseen = cref.df_idf(references, bos, eos)
    out = []
    for cands, refs in zip(candidates, references):
        rv = [cref.vector(r, bos, eos, idf, unseen) for r in refs]
        out.append(np.array([np.mean([cref.cider_d(cref.vector(c, bos, eos, idf, unseen), r) for r in rv]) for c in cands], np.float64))
    return out


def _mean(x):
    return float(np.mean(x)) if len(x) else 0.0


def evaluate(candidates, references, bos, eos, train_captions=None, cider=True):
    """The metrics of CaptionEvaluator.evaluate from the definitions (cider=False leaves the three CIDEr-D keys out)."""
    cw = [[words(c, bos, eos) for c in cs] for cs in candidates]
    rw = [[words(r, bos, eos) for r in rs] for rs in references]
    res = {}
    bleu = bleu_of([(cs[0], rs) for cs, rs in zip(cw, rw) if cs])
    for n in range(4):
        res["bleu_%d" % (n + 1)] = bleu[n]
    if cider:
        sc = cider_scores(candidates, references, bos, eos)
        res["cider_d"] = _mean([s[0] for s in sc if len(s)])
        res["oracle_cider_d"] = _mean([s.max() for s in sc if len(s)])
        res["mean_cider_d"] = _mean([v for s in sc for v in s])
    res["distinct"] = _mean([len(set(map(tuple, cs))) / len(cs) for cs in cw if cs])
    for n in (1, 2):
        res["div_%d" % n] = _mean([len(set(g for c in cs for g in grams(c, n))) / sum(map(len, cs)) for cs in cw if sum(map(len, cs))])
    res["mbleu_4"] = bleu_of([(c, cs[:i] + cs[i + 1:]) for cs in cw if len(cs) >= 2 for i, c in enumerate(cs)])[3]
    res["novel"] = None
    if train_captions is not None:
        train = set(tuple(words(t, bos, eos)) for t in train_captions)
        flat = [tuple(c) for cs in cw for c in cs]
        res["novel"] = sum(c not in train for c in flat) / len(flat) if flat else 0.0
    return res
