"""Stochastic beam search (Kool, van Hoof, Welling, ICML 2019) in float64 numpy: the checker of vc_sbs_expand_f32 / vc_sbs_update and
CaptionGenerator.stochastic_beam_search (test infrastructure, never the product path).

One beam per image, width n; an entry is (sentence, phi, G, done).  A round, for every live unfinished entry i of an image:

    lsm_i(v) = log-softmax of its logits row          key_i(v) = lsm_i(v) + g_i(v)         the kc best words, (key desc, index asc)
    Gt = phi_i + key      Z = max Gt      t = G_i - Gt + log1mexp(Gt - Z)      G' = G_i - max(0, t) - log1p(exp(-|t|))

a finished entry is one candidate, itself; the new beam is the best n candidates under (G' desc, parent asc, word asc); kappa is the
running maximum of the best G' NOT taken.  The state mirrors the device's arrays (count, phi, G, len, done, sent, kappa, parent, tok).
`lsm` selects the log-softmax: lsm64 (the reference proper) or lsm32 (float32 with the kernel's expressions), which the host test uses to
prove the committed parity cases safe: same selections, and every decision taken with a margin no float32 rounding can cross."""
import numpy as np

LN2 = float(np.log(2.0))


def lsm64(x):
    x = np.asarray(x, np.float64)
    m = x.max()
    return (x - m) - np.log(np.exp(x - m).sum())


def lsm32(x):
    """(x - M) - log S, M = max x, S = sum exp(x - M): every operation rounded to float32 (vc_decode_pick_f32's expressions)"""
    x = np.asarray(x, np.float32)
    m = x.max()
    s = np.exp(x - m, dtype=np.float32).sum(dtype=np.float32)
    return ((x - m) - np.log(s, dtype=np.float32)).astype(np.float32)


def log1mexp(x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.where(x > -LN2, np.log(-np.expm1(x)), np.log1p(-np.exp(x)))


def conditioned(G_i, Gt, Z):
    """G' of children with perturbed scores Gt, conditioned on their maximum Z being the parent's G_i (the arg-max child: G_i exactly)"""
    Gt = np.asarray(Gt, np.float64)
    x = Gt - Z
    with np.errstate(all="ignore"):
        t = G_i - Gt + log1mexp(x)
        out = G_i - np.maximum(0.0, t) - np.log1p(np.exp(-np.abs(t)))
    return np.where(x == 0.0, G_i, out)


def gumbel_from_words(w):
    """the documented Philox convention: u = (w + 0.5) * 2^-32 in (0, 1), g = -log(-log(u)), float64"""
    u = (np.asarray(w, np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32
    return -np.log(-np.log(u))


def expand_row(x, g, kc, lsm=lsm64):
    """the first kc words of a row under (key descending, index ascending): (key [kc] float64, lsm [kc], index [kc]) and the smallest
    gap between neighbours among the first kc + 1 (what an exact comparison of the kc indices rests on)"""
    l = lsm(x)
    key = l.astype(np.float64) + np.asarray(g, np.float64)
    key = np.where(np.isnan(key), -np.inf, key)
    order = np.lexsort((np.arange(key.size), -key))
    top = key[order[:kc + 1]]
    gap = float(np.min(top[:-1] - top[1:])) if top.size > 1 else np.inf
    idx = order[:kc]
    return key[idx], l[idx], idx.astype(np.int32), gap


def init_state(B, n, L, bos):
    st = dict(count=np.ones(B, np.int32), phi=np.zeros((B, n)), G=np.zeros((B, n)), len=np.ones((B, n), np.int32),
              done=np.ones((B, n), np.int32), sent=np.full((B, n, L), bos, np.int32), kappa=np.full(B, -np.inf),
              parent=np.arange(B * n, dtype=np.int32), tok=np.full(B * n, bos, np.int32))
    st["done"][:, 0] = 0
    return st


def live_rows(st):
    """[B, n] bool: the rows a round expands"""
    n = st["phi"].shape[1]
    return (np.arange(n)[None, :] < st["count"][:, None]) & (st["done"] == 0)


def round_(st, logits, gumbel, kc, bos, eos, lsm=lsm64):
    """One round from logits / gumbel [B*n, V].  Returns (new state, info); info: cand_key / cand_lsm / cand_idx [B*n, kc] (rows not
    expanded: untouched zeros), live [B*n], and the round's margins -- boundary (worst taken G' minus best untaken), order (smallest gap
    between taken neighbours), row (smallest neighbour gap inside any row's first kc + 1 keys) -- plus carried / evicted: finished
    entries kept in the beam, and finished entries that lost their place to live ones."""
    B, n = st["phi"].shape
    L = st["sent"].shape[2]
    new = init_state(B, n, L, bos)
    new["kappa"] = st["kappa"].copy()
    new["sent"] = np.zeros_like(st["sent"])
    ck, cl, ci = np.zeros((B * n, kc)), np.zeros((B * n, kc), np.float32), np.zeros((B * n, kc), np.int32)
    live = live_rows(st).reshape(-1)
    info = dict(boundary=np.inf, order=np.inf, row=np.inf, carried=0, evicted=0)
    for b in range(B):
        cands = []   # (G', parent, word, phi', finished)
        for i in range(int(st["count"][b])):
            r = b * n + i
            if st["done"][b, i]:
                cands.append((float(st["G"][b, i]), i, int(eos), float(st["phi"][b, i]), True))
                continue
            key, l, idx, gap = expand_row(logits[r], gumbel[r], kc, lsm)
            ck[r], cl[r], ci[r] = key, l, idx
            info["row"] = min(info["row"], gap)
            Gt = st["phi"][b, i] + key
            Gp = conditioned(st["G"][b, i], Gt, Gt[0])
            Gp = np.where(np.isnan(Gp), -np.inf, Gp)
            for c in range(kc):
                cands.append((float(Gp[c]), i, int(idx[c]), float(st["phi"][b, i] + np.float64(l[c])), False))
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        m = min(n, len(cands))
        new["count"][b] = m
        if len(cands) > n:
            new["kappa"][b] = max(new["kappa"][b], cands[n][0])
            info["boundary"] = min(info["boundary"], cands[m - 1][0] - cands[n][0])
            info["evicted"] += sum(1 for t in cands[n:] if t[4])
        for j in range(m):
            Gp, i, word, phi, fin = cands[j]
            if j:
                info["order"] = min(info["order"], cands[j - 1][0] - Gp)
            ln = int(st["len"][b, i])
            new["phi"][b, j], new["G"][b, j] = phi, Gp
            new["sent"][b, j, :ln] = st["sent"][b, i, :ln]
            if fin:
                new["len"][b, j], new["done"][b, j] = ln, 1
                info["carried"] += 1
            else:
                new["sent"][b, j, ln] = word
                new["len"][b, j] = ln + 1
                new["done"][b, j] = 1 if (word == eos or ln + 1 >= L) else 0
            new["parent"][b * n + j], new["tok"][b * n + j] = b * n + i, (eos if fin else word)
    info.update(cand_key=ck, cand_lsm=cl, cand_idx=ci, live=live)
    return new, info


def search(logits_fn, noise_fn, B, n, V, L, bos, eos, lsm=lsm64, rounds=None):
    """A whole search: logits_fn(state) -> [B*n, V] logits of the state's rows; noise_fn(round) -> [B*n, V] Gumbel noise.  Runs until
    every entry of every image is finished (or `rounds` rounds).  Returns the final state."""
    st = init_state(B, n, L, bos)
    kc = min(n + 1, V)
    it = 0
    while live_rows(st).any() and (rounds is None or it < rounds):
        st, _ = round_(st, logits_fn(st), noise_fn(it), kc, bos, eos, lsm)
        it += 1
    return st


def sbs_weights(logprobs, kappa):
    """Kool et al. section 4.2, float64: q = -expm1(-exp(phi - kappa)) (kappa = -inf: 1), w = exp(phi) / q, norm = w / sum w"""
    phi = np.asarray(logprobs, np.float64)
    with np.errstate(over="ignore"):
        q = -np.expm1(-np.exp(phi - float(kappa)))
    w = np.exp(phi) / q
    return w, w / w.sum()


def results(st, eos):
    """per image (kappa, [(words without <BOS>, phi, G, ended, weight, norm_weight), ...]) in rank order"""
    out = []
    for b in range(st["phi"].shape[0]):
        m = int(st["count"][b])
        w, nw = sbs_weights(st["phi"][b, :m], st["kappa"][b])
        caps = []
        for j in range(m):
            s = st["sent"][b, j, 1:st["len"][b, j]].tolist()
            caps.append((s, float(st["phi"][b, j]), float(st["G"][b, j]), bool(s and s[-1] == eos), float(w[j]), float(nw[j])))
        out.append((float(st["kappa"][b]), caps))
    return out


# ---------------------------------------------------------------- the table model of the statistical tests
T_V, T_LEN, T_BOS, T_EOS = 4, 3, 1, 2   # four words, <EOS> among them, captions of at most three words: 1 + 3 + 9 * 4 = 40 captions


def table_model(seed=5):
    """A history-dependent model: logits [4] / [4, 4] / [4, 4, 4] of the first / second / third word given the words before"""
    rng = np.random.default_rng(seed)
    return [rng.normal(0.0, 0.35, (T_V,) * (d + 1)).astype(np.float32) for d in range(T_LEN)]   # (every caption expects >= 17 first ranks in 4096 searches: the chi-square approximation holds)


def table_logits(tables, sent, lens):
    """logits [rows, 4] of rows whose sentences (position 0 = <BOS>) are sent [rows, L] with lens words; rows that cannot be expanded
    get the first table"""
    sent, lens = np.asarray(sent), np.asarray(lens)
    out = np.empty((sent.shape[0], T_V), np.float32)
    for r in range(sent.shape[0]):
        d = int(lens[r]) - 1
        out[r] = tables[d][tuple(sent[r, 1:1 + d])] if 0 <= d < T_LEN else tables[0]
    return out


def table_captions(tables):
    """every complete caption (words without <BOS>) with its float64 probability, in a fixed order"""
    caps = []

    def walk(prefix, lp):
        l = lsm64(tables[len(prefix)][tuple(prefix)])
        for v in range(T_V):
            s = prefix + [v]
            if v == T_EOS or len(s) == T_LEN:
                caps.append((tuple(s), lp + l[v]))
            else:
                walk(s, lp + l[v])
    walk([], 0.0)
    return [c for c, _ in caps], np.exp(np.array([lp for _, lp in caps]))


def inclusion_n2(p):
    """exact inclusion probabilities of sampling two items without replacement: pi_b = p_b + sum_{a != b} p_a p_b / (1 - p_a)"""
    p = np.asarray(p, np.float64)
    tot = (p / (1.0 - p)).sum()
    return p + p * (tot - p / (1.0 - p))


def table_stats(results_, caps, p):
    """(chi-square of the first-ranked caption against p, largest |inclusion count - expectation| in standard deviations, per-search
    weighted estimates of E[len]) from the results of many searches of width 2"""
    pos = {c: k for k, c in enumerate(caps)}
    N = len(results_)
    first, incl, est = np.zeros(len(caps)), np.zeros(len(caps)), np.zeros(N)
    for s, (_, cl) in enumerate(results_):
        first[pos[tuple(cl[0][0])]] += 1
        for c in cl:
            incl[pos[tuple(c[0])]] += 1
            est[s] += c[5] * len(c[0])
    chi2 = float((((first - N * p) ** 2) / (N * p)).sum())
    pi = inclusion_n2(p)
    dev = float(np.max(np.abs(incl - N * pi) / np.sqrt(N * pi * (1.0 - pi))))
    return chi2, dev, est


# ---------------------------------------------------------------- the parity cases of tests/test_gpu_sbs.py
# name -> (B, n, V, Lmax, rounds, eos bias, seed): injected float32 logits and float64 Gumbel noise from default_rng(seed).  The seeds
# were chosen by find_seed below; tests/test_sbs_host.py asserts that each has the property case_margins checks.
CASES = {
    "n1": (1, 1, 5, 6, 5, 0.0, 0),
    "kc-is-V": (3, 2, 3, 6, 5, 0.0, 0),
    "n5-V70": (2, 5, 70, 8, 7, 0.0, 0),
    "widest-beam-kc33": (2, 32, 40, 6, 5, 0.0, 2),
    "one-past-a-1024-chunk": (5, 4, 1025, 6, 4, 0.0, 0),
    "workload-V": (2, 3, 10000, 5, 3, 0.0, 0),
    "longer-than-a-wave": (2, 2, 9, 80, 70, -8.0, 0),
    "finished-carried-then-evicted": (3, 3, 12, 9, 7, 2.5, 3),
}
BOUNDARY_GAP = 1e-3   # between every taken G' and the best untaken one
# Decisions inside the taken set (rank order) and inside a row (which kc words): the two references differ by float32 roundings of lsm,
# <= 2 ulp of |x - M| + |log S| < 32, i.e. < 8e-6 per term, and of their float64 sums over <= 70 rounds in the longest case, whose
# terms' errors are independent roundings: a few 1e-5 at most.  A row's order rests on one term only (M and log S are shared).
ORDER_GAP, ROW_GAP = 1e-4, 1e-5
BOS, EOS = 1, 2


def case_inputs(name, seed=None):
    B, n, V, L, rounds, bias, s0 = CASES[name]
    rng = np.random.default_rng(s0 if seed is None else seed)
    logits = (2.0 * rng.standard_normal((rounds, B * n, V))).astype(np.float32)
    logits[:, :, EOS] += np.float32(bias)
    gumbel = rng.gumbel(size=(rounds, B * n, V))
    return logits, gumbel


def case_rounds(name, lsm=lsm64, seed=None):
    """the case's states and infos after every round"""
    B, n, V, L, rounds, _, _ = CASES[name]
    logits, gumbel = case_inputs(name, seed)
    st, out = init_state(B, n, L, BOS), []
    for it in range(rounds):
        st, info = round_(st, logits[it], gumbel[it], min(n + 1, V), BOS, EOS, lsm)
        out.append((st, info))
    return out


def case_margins(name, seed=None):
    """(safe, facts): safe = the float32-lsm and float64 references select the same candidates in every round (every row's kc words in
    order, every entry's parent and word) and every decision has its margin; facts = the smallest margins and the carried / evicted counts"""
    a, b = case_rounds(name, lsm64, seed), case_rounds(name, lsm32, seed)
    same = all(np.array_equal(x[1]["cand_idx"], y[1]["cand_idx"]) and np.array_equal(x[0]["parent"], y[0]["parent"])
               and np.array_equal(x[0]["tok"], y[0]["tok"]) and np.array_equal(x[0]["sent"], y[0]["sent"]) for x, y in zip(a, b))
    facts = {k: min(min(x[1][k], y[1][k]) for x, y in zip(a, b)) for k in ("boundary", "order", "row")}
    facts["carried"], facts["evicted"] = sum(x[1]["carried"] for x in a), sum(x[1]["evicted"] for x in a)
    facts["finished"] = int(sum(x[0]["done"].sum() for x in a[-1:]))
    safe = same and facts["boundary"] >= BOUNDARY_GAP and facts["order"] >= ORDER_GAP and facts["row"] >= ROW_GAP
    return safe, facts


def find_seed(name, tries=2000, want=lambda facts: True):
    for seed in range(tries):
        safe, facts = case_margins(name, seed)
        if safe and want(facts):
            return seed, facts
    raise LookupError(name)
