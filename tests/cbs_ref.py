"""Constrained beam search in numpy / Python: the checker of vc_beam_update_constrained and CaptionGenerator.constrained_beam_search
(test infrastructure, never the product path).  Anderson et al., EMNLP 2017, on the TopN / Beam classes and the decoder step of
oracle.decode.  An image has C <= 3 constraints; constraint j is a set of word ids, satisfied once ANY of them has been emitted.  A
state is the bit mask s of satisfied constraints; every state has its own pair of heaps partial[s], complete[s], each TopN(w):

    old = [partial[s].extract() for s in 0..S-1]        # heap ARRAY order; every partial[s] reset
    for t in 0..S-1:                                    # target bank
        for s in [t] + [t without bit j, j ascending over the bits of t]:
            for i, beam in enumerate(old[s]):
                s == t: cand = the first w of the row's kc most probable words (descending, stable) in no set j with bit j NOT in s
                else  : cand = the words >= 0 of set j (the bit t has and s lacks), in table order, all of them
                for v in cand: p = float32 softmax probability of v in the beam's row; skip if p < 1e-12
                    lp = beam.logprob + float64(float32 log p)
                    v == eos: complete[t].push(score = lp / len**len_norm_f)     else: partial[t].push(logprob = lp, score = lp)
"""
import numpy as np

from oracle import decode as od
from oracle.decode import Beam, TopN

from .dbs_ref import CASES, CASE_IDS, model_inputs   # noqa: F401  (the small model and images of the generation parity tests)


def constraints(seed, B, V, C, Wc):
    """[B, C, Wc] int32: per image C disjoint sets of Wc words from [3, V), drawn image after image from one generator.  For C >= 2 the
    LAST image's last set is emptied (-1): an image with fewer constraints than the call's C."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, C, max(Wc, 1)), np.int32)
    if C == 0:
        return out
    for b in range(B):
        out[b] = rng.choice(np.arange(3, V), C * Wc, replace=False).reshape(C, Wc)
    if C >= 2:
        out[B - 1, C - 1] = -1
    return out


def sets_of(cons_img, V=None):
    """the rows of one image's table as lists of present words (entries outside [0, V) count as absent)"""
    a = np.asarray(cons_img)
    return [[int(x) for x in row if x >= 0 and (V is None or x < V)] for row in (a.reshape(a.shape[0], -1) if a.size else [[]] * a.shape[0])]


def full_mask(cons_img, V=None):
    return sum(1 << j for j, st in enumerate(sets_of(cons_img, V)) if st)


def n_words(cons, V=None):
    """NW of a call: the largest number of constraint words any image has"""
    return max([sum(len(st) for st in sets_of(ci, V)) for ci in cons] + [0])


def cbs_round(partial, complete, rows, sets, w, kc, eos, len_norm_f):
    """One round of one image.  partial / complete: lists of S TopN; sets: the image's C word lists; rows(s, i, beam) -> (probs, state):
    the float probabilities [V] of the i-th live beam of bank s and the state its continuations carry."""
    S, C = len(partial), len(sets)
    old = [p.extract() for p in partial]
    for p in partial:
        p.reset()
    cache = {}

    def row(s, i, beam):
        if (s, i) not in cache:
            cache[(s, i)] = rows(s, i, beam)
        return cache[(s, i)]

    for t in range(S):
        for s in [t] + [t ^ (1 << j) for j in range(C) if (t >> j) & 1]:
            barred = {v for j in range(C) if not (s >> j) & 1 for v in sets[j]}
            for i, beam in enumerate(old[s]):
                probs, state = row(s, i, beam)
                if s == t:
                    listed = np.argsort(-probs, kind="stable")[:kc]
                    cand = [int(v) for v in listed if int(v) not in barred][:w]
                else:
                    cand = list(sets[(t ^ s).bit_length() - 1])
                for v in cand:
                    p = probs[v]
                    if p < 1e-12:
                        continue
                    lp = beam.logprob + float(np.log(np.float32(p)))   # decoder.py:282: float32 log, float64 sum
                    sent = beam.sentence + [v]
                    if v == eos:
                        score = lp / len(sent) ** len_norm_f if len_norm_f > 0 else lp
                        complete[t].push(Beam(sent, state, lp, score))
                    else:
                        partial[t].push(Beam(sent, state, lp, lp))


def start(S, w, bos, state=0):
    partial, complete = [TopN(w) for _ in range(S)], [TopN(w) for _ in range(S)]
    partial[0].push(Beam([bos], state, 0.0, 0.0))
    return partial, complete


def table_rounds(tables, cons, B, C, w, kc, bos, eos, len_norm_f):
    """The kernel test's reference: tables = [probs [B*S*w, V], ...] per round (row (b*S + s)*w + i is the i-th live beam of bank s of
    image b); cons [B, C, Wc].  A new beam's .state is its source row s*w + i within its image.  Yields after every round (partial,
    complete): per image the lists of S TopN."""
    S = 1 << C
    V = tables[0].shape[1]
    heaps = [start(S, w, bos) for _ in range(B)]
    sets = [sets_of(cons[b], V) if C else [] for b in range(B)]
    for probs in tables:
        with np.errstate(divide="ignore"):
            for b in range(B):
                rows = lambda s, i, beam, b=b: (probs[(b * S + s) * w + i], s * w + i)
                cbs_round(heaps[b][0], heaps[b][1], rows, sets[b], w, kc, eos, len_norm_f)
        yield [h[0] for h in heaps], [h[1] for h in heaps]


def bank_order(full):
    """the submasks of `full`: more satisfied constraints first, then the smaller mask"""
    subs = [s for s in range(full + 1) if s & ~full == 0]
    return sorted(subs, key=lambda s: (-bin(s).count("1"), s))


def select(banks, full, eos):
    """The default result from the per-bank lists [(sentences, scores), ...] (each bank: its complete captions if it has any, else its
    live beams): the first bank in bank_order(full) with a complete caption, else the first with live beams -> ((sentences, scores), state)."""
    order = bank_order(full)
    done = lambda s: len(banks[s][0]) > 0 and banks[s][0][0][-1] == eos
    for s in order:
        if done(s):
            return banks[s], s
    for s in order:
        if len(banks[s][0]) > 0:
            return banks[s], s
    return ([], []), 0


def constrained_beam_search(P, cfg, feature, c_v_row, eps, bos, eos, cons_img, c_means=None, beam_size=2, max_len=30, len_norm_f=0.7,
                            kc=None):
    """One image, end to end, in the precision of P / feature / eps.  cons_img [C, Wc]; kc: listed words per row (None: the whole
    vocabulary).  Returns the S banks' (sentences, scores), descending: a bank's complete captions if it has any, else its live beams."""
    w = int(beam_size)
    C = len(cons_img)
    S = 1 << C
    state = od.initial_state(P, cfg, feature, c_v_row, eps, c_means, std=getattr(cfg, "std", 0.1))
    _, state = od.step(P, bos, state)   # decoder.py:230-236: <BOS> consumed twice, probabilities discarded
    partial, complete = start(S, w, bos, state)
    V = P["decoder/rnn_logits/bias"].shape[-1]
    sets = sets_of(cons_img, V) if C else []

    def rows(s, i, beam):
        probs, st = od.step(P, beam.sentence[-1], beam.state)
        return probs.ravel(), st

    for _ in range(max_len - 1):
        with np.errstate(divide="ignore"):
            cbs_round(partial, complete, rows, sets, w, V if kc is None else min(kc, V), eos, len_norm_f)
        if all(p.size() == 0 for p in partial):
            break
    out = []
    for s in range(S):
        beams = (complete[s] if complete[s].size() else partial[s]).extract(sort=True)
        out.append(([b.sentence for b in beams], [b.score for b in beams]))
    return out


def reference(p, P0, feats, cv, eps, cm, bos, eos, cons, dtype=np.float64, kc=None, **kw):
    """constrained_beam_search above for every image of model_inputs, computed in `dtype`: per image the list of S (sentences, scores).
    kc="call": the product's rule min(V, w + NW)."""
    Pd = {k: v.astype(dtype) for k, v in P0.items()}
    cmd = cm.astype(dtype) if cm is not None else None
    if kc == "call":
        kc = kw.get("beam_size", 2) + n_words(cons, P0["decoder/rnn_logits/bias"].shape[-1])
    return [constrained_beam_search(Pd, p, feats[b].astype(dtype), cv[b].astype(dtype), eps[:, b:b + 1].astype(dtype), bos, eos, cons[b],
                                    c_means=cmd, kc=kc, **kw) for b in range(feats.shape[0])]


def barred_beam_search(P, cfg, feature, c_v_row, eps, bos, eos, barred, c_means=None, beam_size=2, max_len=30, len_norm_f=0.7):
    """oracle.decode.beam_search over the vocabulary without the words `barred` (each row's first beam_size words that are not barred)"""
    state = od.initial_state(P, cfg, feature, c_v_row, eps, c_means, std=getattr(cfg, "std", 0.1))
    _, state = od.step(P, bos, state)
    partial, complete = TopN(beam_size), TopN(beam_size)
    partial.push(Beam([bos], state, 0.0, 0.0))
    barred = set(int(v) for v in barred)
    for _ in range(max_len - 1):
        plist = partial.extract()
        partial.reset()
        for pc in plist:
            probs, st = od.step(P, pc.sentence[-1], pc.state)
            probs = probs.ravel()
            words = [int(v) for v in np.argsort(-probs, kind="stable") if int(v) not in barred][:beam_size]
            for v in words:
                if probs[v] < 1e-12:
                    continue
                sent = pc.sentence + [v]
                lp = pc.logprob + float(np.log(np.float32(probs[v])))
                if v == eos:
                    complete.push(Beam(sent, st, lp, lp / len(sent) ** len_norm_f if len_norm_f > 0 else lp))
                else:
                    partial.push(Beam(sent, st, lp, lp))
        if partial.size() == 0:
            break
    beams = (complete if complete.size() else partial).extract(sort=True)
    return [b.sentence for b in beams], [b.score for b in beams]
