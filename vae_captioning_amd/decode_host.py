"""The host half of caption generation, free of torch and of the engine (generate.py re-exports every name): the layouts of the decoders'
flat result buffers, the parsers of their host copies, the argument checks that need no device, the re-ranking and merging rules."""
import numpy as np


def beams_from_host(ints, dbls, io, B, n, L, last):
    """The kept beams of B images from a slice's result buffers (host copies): per image the list of (sentence, score), descending.
    ints: the int32 fields at the offsets `io` (pcount / ccount [B], p_len / c_len / c_slot [B, n], sent0 / sent1 [B, n, L],
    c_sent [B, n + 1, L]); dbls: p_score [B, n] then c_score [B, n]; last: which of sent0 / sent1 the last round wrote.
    vae_model/decoder.py:295-320: the complete captions if an image has any, else its live beams -- never mixed -- sorted by
    TopN.extract(sort=True), i.e. list.sort(reverse=True) on the heap array: descending score, equal scores in array order.
    Python lists come from whole buffers (one tolist each; slicing lists is ~5x cheaper than a numpy view + tolist per beam), and of
    the two sentence stores only what the slice needs: the pool of complete captions, the live beams, or both."""
    M = B * n
    small, sc = ints[:io["sent0"]].tolist(), dbls.tolist()
    pc, cc = small[io["pcount"]:io["pcount"] + B], small[io["ccount"]:io["ccount"] + B]
    pl, cl, csl = small[io["p_len"]:io["p_len"] + M], small[io["c_len"]:io["c_len"] + M], small[io["c_slot"]:io["c_slot"] + M]
    o = io["sent%d" % last]
    pf = None if all(cc) else ints[o:o + M * L].tolist()
    cf = ints[io["c_sent"]:io["c_sent"] + B * (n + 1) * L].tolist() if any(cc) else None
    res = []
    for b in range(B):
        r0 = b * n
        if cc[b]:
            k_, s_ = cc[b], sc[M + r0:M + r0 + cc[b]]
            rows = [(b * (n + 1) + csl[r0 + j]) * L for j in range(k_)]
            ln, src = cl[r0:r0 + k_], cf
        else:
            k_, s_ = pc[b], sc[r0:r0 + pc[b]]
            rows = [(r0 + j) * L for j in range(k_)]
            ln, src = pl[r0:r0 + k_], pf
        order = sorted(range(k_), key=s_.__getitem__, reverse=True) if k_ > 1 else range(k_)
        res.append([(src[rows[j]:rows[j] + ln[j]], s_[j]) for j in order])
    return res


class FieldLayout(object):
    """Named fields packed back to back in ONE flat buffer (no padding): fields = [(name, size), ...] in buffer order, off[name] = where
    a field starts, total = the buffer's length, views(buf) = {name: its slice of buf}.  The device fills the fields, one copy brings
    the buffer back, the host reads by offset."""
    def __init__(self, fields):
        self.fields, self.off, self.total = list(fields), {}, 0
        for name, n in self.fields:
            self.off[name], self.total = self.total, self.total + n

    def views(self, buf):
        return {name: buf[self.off[name]:self.off[name] + n] for name, n in self.fields}


def beam_fields(B, n, L):
    """(name, size) of the int32 result buffer of a beam-search slice of B images x n beams, sentences of <= L tokens, in buffer order
    (what beams_from_host reads).  The float64 buffer holds p_score, c_score, p_logprob, c_logprob, [B, n] each."""
    M = B * n
    return [("pcount", B), ("ccount", B), ("p_len", M), ("c_len", M), ("c_slot", M), ("sent0", M * L), ("sent1", M * L), ("c_sent", B * (n + 1) * L)]


DIVERSE_MAX_DRAWS = 256   # vc_diverse_rank: one workgroup of 256 lanes per image, one lane per draw


def diverse_fields(B, K, L):
    """(name, size) of the int32 result buffer of a diverse-captioning pass over B images x K draws, candidates of <= L tokens, in
    buffer order (rows r = b*K + k).  The float64 buffer holds score [B, K] (rank order) then logprob [B*K] (row order)."""
    M = B * K
    return [("n_distinct", B), ("rep", M), ("count", M), ("ended", M), ("len", M), ("seq", M * L)]


def diverse_from_host(ints, dbls, io, B, K, L, n_best=None, candidates=False):
    """Per image the ranked distinct captions [(tokens, score, count), ...] of a pass from its result buffers (host copies).
    ints: the int32 fields of diverse_fields at the offsets `io`: n_distinct [B]; rep / count [B, K] in rank order (rep = the draw whose
    tokens represent the entry); ended / len [B*K] and seq [B*K, L] per candidate row.  dbls: score [B, K] in rank order, then logprob
    [B*K] per row.  n_best: keep the first n_best entries of each image (None: all).  candidates=True also returns per image the K
    candidates (tokens, logprob, ended) in draw order."""
    M = B * K
    small = ints[:io["seq"]].tolist()
    nd = small[io["n_distinct"]:io["n_distinct"] + B]
    rep, cnt = small[io["rep"]:io["rep"] + M], small[io["count"]:io["count"] + M]
    ln, en = small[io["len"]:io["len"] + M], small[io["ended"]:io["ended"] + M]
    seq = ints[io["seq"]:io["seq"] + M * L].tolist()
    sc = dbls[:M].tolist()
    res = []
    for b in range(B):
        n = nd[b] if n_best is None else min(nd[b], int(n_best))
        out = []
        for j in range(n):
            r = b * K + rep[b * K + j]
            out.append((seq[r * L:r * L + ln[r]], sc[b * K + j], cnt[b * K + j]))
        res.append(out)
    if not candidates:
        return res
    lp = dbls[M:2 * M].tolist()
    cands = [[(seq[r * L:r * L + ln[r]], lp[r], bool(en[r])) for r in range(b * K, (b + 1) * K)] for b in range(B)]
    return res, cands


SCORE_MAX_TOKENS = 256   # score(): tokens scored per caption (human captions may be longer than gen_max_len)


def rerank_by_marginal(entries, marginals, eos, len_norm_f):
    """diverse(rerank="marginal"): entries [(tokens, score, count), ...] in likelihood order and their marginals ->
    [(tokens, marginal / (1 + n)**len_norm_f, count, marginal), ...]: <EOS>-ended before cut captions, then the new score descending;
    exact ties keep the likelihood order (a stable sort)."""
    new = [(t, m / (1 + len(t)) ** len_norm_f, n, m) for (t, _, n), m in zip(entries, marginals)]
    return sorted(new, key=lambda x: (not (len(x[0]) > 0 and x[0][-1] == eos), -x[1]))


def sbs_weights(logprobs, kappa):
    """Importance weights of a stochastic beam search's captions (Kool et al. 2019, section 4.2), float64: with phi their
    log-probabilities and kappa the (n+1)-th largest perturbed score, q_i = P(perturbed_i > kappa) = -expm1(-exp(phi_i - kappa)) (kappa =
    -inf: 1), w_i = exp(phi_i) / q_i, norm_i = w_i / sum_j w_j.  Returns (w, norm)."""
    phi = np.asarray(logprobs, np.float64)
    with np.errstate(over="ignore"):
        q = -np.expm1(-np.exp(phi - float(kappa)))
    w = np.exp(phi) / q
    return w, w / w.sum()


def merge_groups(groups):
    """diverse_beam_search's per-image result (a list of G lists of (tokens, score)) as ONE ranked list of distinct captions:
    [(tokens, score, [groups that produced it]), ...], equal token sequences merged under their best score, score descending (ties
    keep the order of first appearance: group by group, each best first)."""
    best, order = {}, []
    for g, beams in enumerate(groups):
        for toks, score in beams:
            key = tuple(toks)
            if key not in best:
                best[key] = [list(toks), score, [g]]
                order.append(key)
            else:
                ent = best[key]
                ent[1] = max(ent[1], score)
                if g not in ent[2]:
                    ent[2].append(g)
    return sorted((tuple(best[k]) for k in order), key=lambda x: -x[1])


def check_truncation(top_k, top_p, method="sample"):
    """(top_k, top_p) of truncated sampling as (int, float); ValueError for values outside top_k >= 0, 0 < top_p <= 1 and for a
    truncation asked of a greedy decode (it has no draw to truncate).  (0, 1.0) = off."""
    if isinstance(top_k, bool) or int(top_k) != top_k or int(top_k) < 0:
        raise ValueError("top_k must be an integer >= 0 (0 = off; got %r)" % (top_k,))
    top_p = float(top_p)
    if not (0.0 < top_p <= 1.0):
        raise ValueError("top_p must be in (0, 1] (1 = off; got %r)" % (top_p,))
    if top_p < 1.0 and float(np.float32(top_p)) >= 1.0:
        raise ValueError("top_p = %r is 1 in float32: pass 1.0 for no nucleus cut" % (top_p,))
    if method != "sample" and (int(top_k) != 0 or top_p != 1.0):
        raise ValueError("top_k / top_p truncate the draw of method='sample'; method=%r has none" % (method,))
    return int(top_k), top_p


def check_typical(typical_p, min_p, eta, method="sample", top_k=0, top_p=1.0):
    """(typical_p, min_p, eta) of typical / min-p / eta sampling as floats; ValueError for values outside 0 < typical_p <= 1,
    0 <= min_p <= 1, 0 <= eta < 1, for a cut asked of a greedy decode (it has no draw to cut) and for a cut together with top_k / top_p
    (the two families would need a stated order of renormalisation: DESIGN.md "Typical / min-p / eta sampling").  (1.0, 0.0, 0.0) = off."""
    typical_p, min_p, eta = float(typical_p), float(min_p), float(eta)
    if not (0.0 < typical_p <= 1.0):
        raise ValueError("typical_p must be in (0, 1] (1 = off; got %r)" % (typical_p,))
    if typical_p < 1.0 and float(np.float32(typical_p)) >= 1.0:
        raise ValueError("typical_p = %r is 1 in float32: pass 1.0 for no typical cut" % (typical_p,))
    if not (0.0 <= min_p <= 1.0):
        raise ValueError("min_p must be in [0, 1] (0 = off; got %r)" % (min_p,))
    if not (0.0 <= eta < 1.0) or float(np.float32(eta)) >= 1.0:
        raise ValueError("eta must be in [0, 1) (0 = off; got %r)" % (eta,))
    if typical_p != 1.0 or min_p != 0.0 or eta != 0.0:
        if method != "sample":
            raise ValueError("typical_p / min_p / eta cut the draw of method='sample'; method=%r has none" % (method,))
        if int(top_k) != 0 or float(top_p) != 1.0:
            raise ValueError("typical_p / min_p / eta do not combine with top_k / top_p: give one family of cuts")
    return typical_p, min_p, eta


CBS_MAX_SETS, CBS_MAX_WORDS = 3, 4  # constrained beam search: constraints per image, words per constraint (vc_beam_update_constrained)


def check_constraints(constraints, B, V, bos, eos, beam_size):
    """constrained_beam_search's `constraints` (per image a list of at most 3 lists of 1..4 token ids) as the call's table:
    (C, Wc, cons [B, C, Wc] int32 padded with -1, NW = the largest number of constraint words of an image).  C and Wc are the call's
    largest; an image with fewer sets has all -1 sets behind its own.  ValueError for more than 3 sets, a set of more than 4 words or of
    none, overlapping sets, ids outside [0, V), a set holding bos or eos, or beam_size << C > 16."""
    if len(constraints) != B:
        raise ValueError("constrained_beam_search: %d constraint lists for %d images" % (len(constraints), B))
    w = int(beam_size)
    C = Wc = NW = 0
    for b, sets in enumerate(constraints):
        if len(sets) > CBS_MAX_SETS:
            raise ValueError("constrained_beam_search: image %d has %d constraints (at most %d)" % (b, len(sets), CBS_MAX_SETS))
        seen = set()
        for st in sets:
            st = list(st)
            if not 1 <= len(st) <= CBS_MAX_WORDS:
                raise ValueError("constrained_beam_search: image %d has a constraint of %d words (1..%d)" % (b, len(st), CBS_MAX_WORDS))
            for v in st:
                if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < V:
                    raise ValueError("constrained_beam_search: image %d: word id %r outside [0, %d)" % (b, v, V))
                if int(v) in (int(bos), int(eos)):
                    raise ValueError("constrained_beam_search: image %d: a constraint holds <BOS> or <EOS> (%d)" % (b, int(v)))
                if int(v) in seen:
                    raise ValueError("constrained_beam_search: image %d: word %d appears twice in its constraints (sets must be disjoint)" % (b, int(v)))
                seen.add(int(v))
            Wc = max(Wc, len(st))
        C, NW = max(C, len(sets)), max(NW, len(seen))
    if w < 1 or (w << C) > 16:
        raise ValueError("constrained_beam_search: beam_size << constraints must be 1..16, got %d << %d" % (w, C))
    cons = np.full((B, C, max(Wc, 1)), -1, np.int32)
    for b, sets in enumerate(constraints):
        for j, st in enumerate(sets):
            cons[b, j, :len(st)] = [int(v) for v in st]
    return C, max(Wc, 1), cons, NW


def select_bank(banks, full, eos):
    """constrained_beam_search's default result from an image's per-state lists of (sentence, score): the submasks of `full` (the
    image's accepting state) with more satisfied constraints first, then the smaller mask; the first bank with a complete caption
    gives the result, else the first with live beams.  -> (beams, state)."""
    order = sorted((s for s in range(full + 1) if s & ~full == 0), key=lambda s: (-bin(s).count("1"), s))
    for s in order:   # (a bank's list is its complete captions if it has any -- they end in <EOS> -- else its live beams, which never do)
        if banks[s] and banks[s][0][0][-1] == eos:
            return banks[s], s
    for s in order:
        if banks[s]:
            return banks[s], s
    return [], 0


def marginal_greedy_from_host(ints, dbls, io, B, K, L, steps):
    """Per image {"tokens", "marginal", "logprob" float64 [K]} of a marginal_greedy pass from its result buffers (host copies) after
    `steps` rounds.  ints: len [B] and seq [B, L] at the offsets `io`; dbls: logw0 then logw1 [B*K] -- round r reads logw[r & 1] and
    writes the other, so the draws' log-probabilities are in logw[steps & 1].  marginal = logsumexp_k logprob - log K."""
    M = B * K
    lw = dbls[(steps % 2) * M:(steps % 2 + 1) * M].reshape(B, K).copy()
    mx = lw.max(axis=1)
    marg = mx + np.log(np.exp(lw - mx[:, None]).sum(axis=1)) - np.log(K)
    ln, seq = ints[io["len"]:io["len"] + B].tolist(), ints[io["seq"]:io["seq"] + B * L].tolist()
    return [{"tokens": seq[b * L:b * L + ln[b]], "marginal": float(marg[b]), "logprob": lw[b]} for b in range(B)]


def sbs_from_host(ints, dbls, io, B, n, L, steps, eos):
    """Per image {"kappa", "captions": [(words without <BOS>, logprob, perturbed, ended, weight, norm_weight), ...]} of a stochastic beam
    search from its result buffers (host copies) after `steps` rounds.  ints: count [B], len [B*n], sent0 / sent1 [B*n, L] at the offsets
    `io` (an image's first count[b] rows are its entries, in rank order; len counts the <BOS>; round r reads sent[r & 1] and writes the
    other, so the sentences are in sent[steps & 1]); dbls: phi, G [B*n] then kappa [B].  The weights are sbs_weights' over the entries."""
    M = B * n
    cnt, ln = ints[io["count"]:io["count"] + B].tolist(), ints[io["len"]:io["len"] + M].tolist()
    o = io["sent%d" % (steps & 1)]
    words = ints[o:o + M * L].tolist()
    ph, Gs, kap = dbls[:M].tolist(), dbls[M:2 * M].tolist(), dbls[2 * M:2 * M + B].tolist()
    res = []
    for b in range(B):
        rows = range(b * n, b * n + cnt[b])
        w, nw = sbs_weights([ph[r] for r in rows], kap[b])
        caps = []
        for j, r in enumerate(rows):
            s = words[r * L + 1:r * L + ln[r]]
            caps.append((s, ph[r], Gs[r], bool(s) and s[-1] == eos, float(w[j]), float(nw[j])))
        res.append({"kappa": kap[b], "captions": caps})
    return res
