"""The fp64 checker of caption scoring (generate.py: CaptionGenerator.score, diverse(rerank="marginal")): a numpy restatement on the
oracle's per-image decoder (oracle/decode.py: initial_state, step).  TEST INFRASTRUCTURE -- the product never imports it.

log p(caption | z_k, image) = sum_t log softmax(logits_t)[token_t] with the caption teacher-forced from <BOS>; the marginal over K
draws is log 1/K sum_k p(caption | z_k, image); corpus perplexity = exp(-sum marginal / sum tokens)."""
import math

import numpy as np

from oracle import decode as od


def strip_bos(tokens, bos):
    t = [int(w) for w in tokens]
    return t[1:] if t and t[0] == bos else t


def logprob_from_step_probs(step_probs, tokens):
    """step_probs [T][V]: the model's distribution at every step of ONE draw -> sum_t log p_t[tokens[t]]"""
    return float(sum(math.log(float(step_probs[t][w])) for t, w in enumerate(tokens)))


def marginal(logprob):
    """log 1/K sum_k exp(logprob[k]), max-shifted"""
    lp = np.asarray(logprob, np.float64)
    m = lp.max()
    return float(m + np.log(np.exp(lp - m).sum()) - np.log(lp.size))


def perplexity(marginals, tokens):
    return math.exp(-float(np.sum(marginals)) / float(np.sum(tokens)))


def caption_logprob(P64, p, feat, cv_row, eps_b, cm, tokens, bos):
    """One caption under ONE draw of one image: eps_b [S, 1, L] (None for --no_encoder); tokens without <BOS>"""
    state = od.initial_state(P64, p, feat, cv_row, eps_b, cm, std=p.std)
    tok, lp = bos, 0.0
    for w in tokens:
        probs, state = od.step(P64, tok, state)
        lp += float(np.log(probs[w]))
        tok = w
    return lp


def score(P64, p, feats, cv, eps, cm, captions, bos):
    """What CaptionGenerator.score returns, per image and caption: eps [K, S, B, L] (None: --no_encoder, one draw)"""
    K = 1 if eps is None else len(eps)
    out = []
    for b, caps in enumerate(captions):
        rows = []
        for t in caps:
            t = strip_bos(t, bos)
            lp = [caption_logprob(P64, p, feats[b].astype(np.float64), None if cv is None else cv[b].astype(np.float64),
                                  None if eps is None else np.asarray(eps[k])[:, b:b + 1].astype(np.float64), cm, t, bos) for k in range(K)]
            rows.append({"logprob": np.array(lp), "marginal": marginal(lp), "tokens": len(t)})
        out.append(rows)
    return out


def rerank_rule(entries, marginals, eos, len_norm_f=0.7):
    """One image's distinct captions [(tokens, score, count), ...] in likelihood order and their marginals -> [(tokens, new score, count,
    marginal), ...]: new score = marginal / (1 + n)**len_norm_f; <EOS>-ended captions first, then the new score descending, exact ties in
    the order they came in."""
    rows = []
    for i, ((t, _, n), m) in enumerate(zip(entries, marginals)):
        ended = len(t) > 0 and t[-1] == eos
        rows.append((0 if ended else 1, -(m / (1.0 + len(t)) ** len_norm_f), i, t, n, m))
    rows.sort(key=lambda r: r[:3])
    return [(t, -neg, n, m) for _, neg, _, t, n, m in rows]
