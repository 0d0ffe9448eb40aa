"""Marginal decoding in numpy float64: the checker of vc_mixture_topk_f32 / vc_mixture_advance_f32 and of
CaptionGenerator.marginal_greedy / marginal_beam_search (test infrastructure, never the product path).

A hypothesis group owns K rows of logits, one per latent draw.  Per row: M = max x, S = sum exp(x - M), lsm(v) = (x_v - M) - log S.
logw[k] = log p(prefix | z_k); the draws' weights are softmax_k(logw); the mixture is q(v) = sum_k w_k exp(x_kv - M_k) / S_k, k
ascending.  Chain rule: sum_t log q_t(y_t) = logsumexp_k sum_t lsm_kt(y_t) - log K when logw starts at 0.

The decoders run on oracle.decode's initial_state / step; the beam decoder mirrors oracle.decode.beam_search (TopN, p < 1e-12 skipped,
the np.float32(p) log, <BOS> consumed twice) with a hypothesis that carries K states and its logw vector."""
import numpy as np

from oracle import decode as od
from oracle.decode import Beam, TopN


def row_stats(x):
    """x [..., V] -> (M, log S)"""
    x = np.asarray(x, np.float64)
    M = x.max(axis=-1)
    return M, np.log(np.exp(x - M[..., None]).sum(axis=-1))


def weights(logw):
    """softmax over the last axis (the draws of a group)"""
    logw = np.asarray(logw, np.float64)
    w = np.exp(logw - logw.max(axis=-1, keepdims=True))
    return w / w.sum(axis=-1, keepdims=True)


def mix(probs, logw):
    """probs [K, V] (each row a distribution), logw [K] -> q [V], summed over k in ascending order"""
    w = weights(logw)
    q = np.zeros(probs.shape[1], np.float64)
    for k in range(probs.shape[0]):
        q += w[k] * probs[k]
    return q


def mixture_topk(logits, V, K, logw, kc):
    """logits [G*K, ld] (columns >= V ignored), logw [G*K] -> top_p, top_i [G, kc] under (value descending, index ascending),
    stat [G*K, 2] = (M, log S), q [G, V]"""
    x = np.asarray(logits, np.float64)[:, :V]
    G = x.shape[0] // K
    M, logS = row_stats(x)
    sm = np.exp(x - M[:, None] - logS[:, None])
    q = np.stack([mix(sm[g * K:(g + 1) * K], np.asarray(logw, np.float64)[g * K:(g + 1) * K]) for g in range(G)])
    top_i = np.stack([np.argsort(-q[g], kind="stable")[:kc] for g in range(G)])
    return np.take_along_axis(q, top_i, 1), top_i, np.stack([M, logS], 1), q


def advance(logits, V, K, parent, tok, logw_in, eos=None, done=None, seq=None, length=None):
    """vc_mixture_advance_f32: -> (logw_out, parent_rows, tok_rows) and, in the greedy form (done / seq / length given: copies are
    updated and returned too), (done, seq, length).  seq [Gn, Lmax]."""
    x = np.asarray(logits, np.float64)[:, :V]
    M, logS = row_stats(x)
    Gn = len(tok)
    logw_in = np.asarray(logw_in, np.float64)
    logw_out, parent_rows, tok_rows = np.zeros(Gn * K), np.zeros(Gn * K, np.int32), np.zeros(Gn * K, np.int32)
    greedy = done is not None
    if greedy:
        done, seq, length = np.array(done), np.array(seq), np.array(length)
    for g in range(Gn):
        live = True
        if greedy:
            live = done[g] == 0 and length[g] < seq.shape[1]
        for k in range(K):
            src = (parent[g] if parent is not None else g) * K + k
            term = (x[src, tok[g]] - M[src]) - logS[src]
            logw_out[g * K + k] = logw_in[src] + (term if live else 0.0)
            parent_rows[g * K + k], tok_rows[g * K + k] = src, tok[g]
        if greedy and done[g] == 0:
            if live:
                seq[g, length[g]] = tok[g]
                length[g] += 1
            done[g] = int(tok[g] == eos)
    return (logw_out, parent_rows, tok_rows) + ((done, seq, length) if greedy else ())


def _states(P, cfg, feature, c_v_row, eps, c_means):
    """the K initial decoder states of one image: eps [K, S, 1, L]"""
    return [od.initial_state(P, cfg, feature, c_v_row, eps[k], c_means, std=getattr(cfg, "std", 0.1)) for k in range(eps.shape[0])]


def marginal_greedy(P, cfg, feature, c_v_row, eps, bos, eos, c_means=None, max_len=30):
    """One image.  -> (tokens, logw float64 [K], marginal, the smallest log q1 - log q2 over the steps)"""
    states = _states(P, cfg, feature, c_v_row, eps, c_means)
    K = len(states)
    logw, tok, out, gap = np.zeros(K), bos, [], np.inf
    for _ in range(max_len):
        res = [od.step(P, tok, s) for s in states]
        probs, states = np.stack([r[0].ravel() for r in res]), [r[1] for r in res]
        q = mix(probs, logw)
        order = np.argsort(-q, kind="stable")
        gap = min(gap, float(np.log(q[order[0]]) - np.log(q[order[1]])))
        tok = int(order[0])
        logw = logw + np.log(probs[:, tok])
        out.append(tok)
        if tok == eos:
            break
    return out, logw, float(np.logaddexp.reduce(logw) - np.log(K)), gap


def marginal_beam_search(P, cfg, feature, c_v_row, eps, bos, eos, c_means=None, beam_size=2, max_len=30, len_norm_f=0.7):
    """oracle.decode.beam_search over the mixture, one image.  A Beam's state is (the K states, logw [K]).
    -> (sentences, scores, the smallest adjacent log-gap among the first beam_size + 1 words of any expanded hypothesis)"""
    states = [od.step(P, bos, s)[1] for s in _states(P, cfg, feature, c_v_row, eps, c_means)]   # decoder.py:230-236, probs discarded
    K = len(states)
    partial = TopN(beam_size)
    partial.push(Beam([bos], (states, np.zeros(K)), 0.0, 0.0))
    complete = TopN(beam_size)
    gap = np.inf
    for _ in range(max_len - 1):
        plist = partial.extract()
        partial.reset()
        for pc in plist:
            sts, logw = pc.state
            res = [od.step(P, pc.sentence[-1], s) for s in sts]
            probs, new = np.stack([r[0].ravel() for r in res]), [r[1] for r in res]
            q = mix(probs, logw)
            w_probs = list(enumerate(q))
            w_probs.sort(key=lambda x: -x[1])  # stable: ties -> lower index first
            with np.errstate(divide="ignore"):
                lq = np.log(np.array([p for _, p in w_probs[:beam_size + 1]]))
            if len(lq) > 1:
                gap = min(gap, float(np.min(lq[:-1] - lq[1:])))
            for w, p in w_probs[:beam_size]:
                if p < 1e-12:
                    continue
                sentence = pc.sentence + [w]
                logprob = pc.logprob + float(np.log(np.float32(p)))
                score = logprob
                st = (new, logw + np.log(probs[:, w]))
                if w == eos:
                    if len_norm_f > 0:
                        score /= len(sentence) ** len_norm_f
                    complete.push(Beam(sentence, st, logprob, score))
                else:
                    partial.push(Beam(sentence, st, logprob, score))
        if partial.size() == 0:
            break
    if not complete.size():
        complete = partial
    beams = complete.extract(sort=True)
    return [b.sentence for b in beams], [b.score for b in beams], gap
