"""Contrastive search in numpy / Python, float64: the checker of vc_contrastive_pick_f32 and of CaptionGenerator.contrastive_search
(test infrastructure, never the product path).  The definition is DESIGN.md "Contrastive search" / include/vaecap.h.

pick_rows is one round's pick over rows (the kernel's contract); contrastive_search decodes one image with oracle.decode's init chain,
controls_ref.step_logits and process_row.  Both report how close their decisions were: a decision between the best score s and the
second best is SAFE when the gap exceeds SAFE_MARGIN * (ATOL + RTOL * |s of the rejected|) (controls_ref's constants and Margin); a
float32 decoder whose scores are within ATOL + RTOL * |s| of these then makes the same choices."""
import numpy as np

from oracle import decode as od

from . import controls_ref
from .controls_ref import ATOL, RTOL, SAFE_MARGIN, Margin, process_row, softmax, step_logits  # noqa: F401 (re-exported)

LMAX = 30   # the kernel cases' sentence capacity: hist holds LMAX + 1 vectors per row


def unit(v):
    n = np.sqrt((v * v).sum())
    return v / n if n > 0 else v


def scores(h, p, hist, alpha):
    """s [k] of the candidates' states h [k, H] and probabilities p [k] against the unit vectors hist [n, H] (n may be 0)"""
    h, p, hist = np.asarray(h, np.float64), np.asarray(p, np.float64), np.asarray(hist, np.float64)
    norm = np.sqrt((h * h).sum(1))
    sim = np.zeros(h.shape[0])
    if hist.shape[0]:
        best = (h @ hist.T).max(1)
        ok = norm > 0
        sim[ok] = best[ok] / norm[ok]
    return (1.0 - alpha) * p - alpha * sim


def decide(s, all_zero=False):
    """(pick, gap in tolerance units): the largest s, ties to the lower rank; the gap to the best of the others (inf for k = 1).
    all_zero: alpha = 1 over an empty history, where every s is (1 - 1) * p - 1 * 0 = 0 exactly in float32 as in float64 -- a tie that
    no rounding can break, so rank 0 is a safe pick."""
    pick = int(np.argmax(s))   # (the first maximum)
    if s.shape[0] == 1 or all_zero:
        return pick, float("inf")
    rest = np.delete(s, pick).max()
    return pick, float(s[pick] - rest) / (ATOL + RTOL * abs(float(rest)))


def pick_rows(h2, cand_tok, cand_p, hist, lens, done, seq, logprob, alpha, eos, emit):
    """One launch of vc_contrastive_pick_f32 on copies of its buffers: h2 [rows * k, H], cand_tok / cand_p [rows, k], hist
    [rows, Lmax + 1, H], lens / done [rows], seq [rows, Lmax], logprob [rows].  Returns a dict of the buffers after the launch (hist, len,
    done, seq, logprob as float64 arrays / ints), of h_sel, parent, pick, score for the rows that ran (NaN / -1 elsewhere), `ran` [rows]
    bool and `gap` [rows] (tolerance units; inf where nothing was decided)."""
    rows, k = cand_tok.shape
    H, Lmax = h2.shape[1], seq.shape[1]
    out = dict(hist=np.array(hist, np.float64), len=np.array(lens), done=np.array(done), seq=np.array(seq), logprob=np.array(logprob, np.float64),
               h_sel=np.full((rows, H), np.nan), parent=np.full(rows * k, -1, np.int64), pick=np.full(rows, -1, np.int64),
               score=np.full((rows, k), np.nan), ran=np.zeros(rows, bool), gap=np.full(rows, np.inf))
    for r in range(rows):
        n = int(lens[r]) + (1 if emit else 0)
        if done[r] != 0 or lens[r] < 0 or n > Lmax:
            continue
        h = np.asarray(h2[r * k:(r + 1) * k], np.float64)
        s = scores(h, cand_p[r], np.asarray(hist[r, :n], np.float64), alpha)
        pk, gap = decide(s, all_zero=(n == 0 and alpha == 1.0))
        out["ran"][r], out["gap"][r], out["pick"][r], out["score"][r] = True, gap, pk, s
        out["h_sel"][r] = h[pk]
        out["hist"][r, n] = unit(h[pk])
        out["parent"][r * k:(r + 1) * k] = r * k + pk
        if emit:
            w = int(cand_tok[r, pk])
            out["seq"][r, lens[r]] = w
            out["len"][r] = lens[r] + 1
            with np.errstate(divide="ignore"):
                out["logprob"][r] += float(np.log(np.float32(cand_p[r, pk])))   # f32 log of the f32 probability, f64 sum
            out["done"][r] = 1 if w == eos else 0
    return out


def contrastive_search(P, cfg, feature, c_v_row, eps, bos, eos, k, alpha, controls, c_means=None, max_len=30):
    """One image -> (tokens, logprob, margin).  The margin is the smallest decision gap in tolerance units over the rounds: best against
    second-best s, and the k-th against the (k+1)-th probability (what the candidate list is cut at; two words of probability exactly 0
    are ordered by their index on either side)."""
    state = od.initial_state(P, cfg, feature, c_v_row, eps, c_means, std=getattr(cfg, "std", 0.1))
    logits, state = step_logits(P, bos, state)
    hist, out, lp, margin = [unit(state[1][0])], [], 0.0, Margin()
    for _ in range(max_len):
        probs = softmax(process_row(logits, out, controls, eos))
        order = np.argsort(-probs, kind="stable")
        kk = min(int(k), probs.size)
        cands = order[:kk]
        if kk < probs.size and not (probs[order[kk - 1]] == 0 and probs[order[kk]] == 0):
            margin.see(probs[order[kk - 1]], probs[order[kk]])
        nexts = [step_logits(P, int(v), state) for v in cands]
        h = np.stack([st[1][0] for _, st in nexts])
        s = scores(h, probs[cands], np.stack(hist), alpha)
        pk, gap = decide(s)
        margin.value = min(margin.value, gap)
        tok = int(cands[pk])
        with np.errstate(divide="ignore"):
            lp += float(np.log(np.float32(probs[tok])))
        out.append(tok)
        logits, state = nexts[pk]
        hist.append(unit(h[pk]))
        if tok == eos:
            break
    return out, lp, margin.value


# ------------------------------------------------------------------ the kernel cases (CPU: the share of unsafe rows; GPU: equal)
ROWS, KS, HISTS, HS, ALPHAS = (1, 3, 130), (1, 2, 5, 16), (0, 1, 2, LMAX), (32, 36, 512), (0.0, 0.6, 1.0)
KERNEL_GRID = [(rows, k, n, H, a) for rows in ROWS for k in KS for n in HISTS for H in HS for a in ALPHAS]
KERNEL_EOS, KERNEL_V = 2, 1000
_KCACHE = {}


def kernel_seed(rows, k, n, H, alpha):
    return 1000003 * rows + 10007 * k + 101 * n + 7 * H + int(10 * alpha) + RESEED.get((rows, k, n, H, alpha), 0)


def kernel_case(rows, k, n, H, alpha):
    """Seeded, junk-filled inputs of one launch with history length n (n = 0: the emit = 0 round, len = 0; else emit = 1, len = n - 1):
    candidates correlated with a history vector, h = noise / sqrt(H) + c * hist[j], so that the similarities are not all near 0.  About
    a tenth of the rows of a launch of >= 3 rows are done.  -> (dict of float32 / int32 / float64 arrays, emit)"""
    key = (rows, k, n, H, alpha)
    if key in _KCACHE:
        return _KCACHE[key]
    rng = np.random.default_rng(kernel_seed(*key))
    emit = 1 if n > 0 else 0
    hist = np.full((rows, LMAX + 1, H), 7777.0, np.float32)
    g = rng.standard_normal((rows, n, H))
    hist[:, :n] = (g / np.sqrt((g * g).sum(-1, keepdims=True))).astype(np.float32)
    h2 = rng.standard_normal((rows, k, H)) / np.sqrt(H)
    if n:
        j = rng.integers(0, n, (rows, k))
        h2 = h2 + rng.uniform(0.0, 1.5, (rows, k, 1)) * hist[np.arange(rows)[:, None], j]
    h2 = (h2 * rng.uniform(0.5, 2.0, (rows, k, 1))).astype(np.float32).reshape(rows * k, H)
    x = rng.standard_normal((rows, 4 * k + 4)) * 1.5
    p = np.exp(x - x.max(1, keepdims=True))
    p = (-np.sort(-(p / p.sum(1, keepdims=True)), axis=1)[:, :k]).astype(np.float32)
    tok = np.stack([rng.choice(np.arange(3, KERNEL_V), k, replace=False) for _ in range(rows)]).astype(np.int32)
    ends = rng.random(rows) < 0.3   # a third of the rows have <EOS> among their candidates
    tok[ends, rng.integers(0, k, rows)[ends]] = KERNEL_EOS
    done = (rng.random(rows) < 0.1).astype(np.int32) if rows >= 3 else np.zeros(rows, np.int32)
    if rows >= 3:
        done[0], done[1] = 0, 1
    case = dict(h2=h2, tok=tok, p=p, hist=hist, len=np.full(rows, n - emit, np.int32), done=done,
                seq=rng.integers(3, KERNEL_V, (rows, LMAX)).astype(np.int32), logprob=rng.standard_normal(rows) * 3.0)
    _KCACHE[key] = (case, emit)
    return _KCACHE[key]


def kernel_reference(rows, k, n, H, alpha):
    """pick_rows of kernel_case (cached: the tests share it and leave it unchanged) -> (result dict, safe [rows] bool)"""
    key = ("ref", rows, k, n, H, alpha)
    if key not in _KCACHE:
        c, emit = kernel_case(rows, k, n, H, alpha)
        res = pick_rows(c["h2"], c["tok"], c["p"], c["hist"], c["len"], c["done"], c["seq"], c["logprob"], alpha, KERNEL_EOS, emit)
        _KCACHE[key] = (res, res["gap"] > SAFE_MARGIN)
    return _KCACHE[key]


# kernel cases whose first seed leaves more than 2 % of their rows unsafe take the next ones (chosen on the CPU: the first offset that
# passes; tests/test_contrastive_host.py asserts the share for every case)
RESEED = {(3, 16, 2, 32, 1.0): 1, (3, 16, LMAX, 512, 0.6): 1}


# ------------------------------------------------------------------ the cases of the end-to-end tests (CPU: safe; GPU: equal)
BOS, EOS, MAX_LEN = controls_ref.BOS, controls_ref.EOS, controls_ref.MAX_LEN
SETTINGS = {"plain": (5, 0.6, None), "wide": (16, 0.6, None), "likelihood_off": (5, 1.0, None), "all": (5, 0.6, "all")}   # name -> (k, alpha, controls_ref setting)
_CACHE = {}


def run_image(case, name, i, k=None, alpha=None):
    """The float64 reference of image i of controls_ref's pool of prior case `case` under setting `name` (k / alpha override it) ->
    ((tokens, logprob), margin).  Cached."""
    k0, a0, ctl_name = SETTINGS[name]
    k, alpha = (k0 if k is None else k), (a0 if alpha is None else alpha)
    key = (case, ctl_name, i, k, alpha)
    if key not in _CACHE:
        from vae_captioning_amd.controls import DecodeControls
        ctl = controls_ref.settings()[ctl_name] if ctl_name is not None else DecodeControls()
        p, P0, feats, cv, eps, cm, _ = controls_ref.pool(case)
        if ("P64", case) not in _CACHE:
            _CACHE[("P64", case)] = {kk: v.astype(np.float64) for kk, v in P0.items()}
        toks, lp, m = contrastive_search(_CACHE[("P64", case)], p, feats[i].astype(np.float64), cv[i].astype(np.float64),
                                         eps[:, i:i + 1].astype(np.float64), BOS, EOS, k, alpha, ctl, c_means=cm, max_len=MAX_LEN)
        _CACHE[key] = ((toks, lp), m)
    return _CACHE[key]


def image_margin(case, name, i):
    """what a case's image must exceed SAFE_MARGIN in: its own decisions and, for the settings without controls, those of greedy decoding
    (alpha = 0 and k = 1 are compared with greedy() on the same images)"""
    m = run_image(case, name, i)[1]
    if SETTINGS[name][2] is None:
        m = min(m, run_image(case, name, i, alpha=0.0)[1], run_image(case, name, i, k=1)[1])
    return m


def run_case(case, name):
    """the six images IMAGES[(case, name)] -> (per image (tokens, logprob), the smallest margin)"""
    idx = IMAGES[(case, name)]
    return [run_image(case, name, i)[0] for i in idx], min(image_margin(case, name, i) for i in idx)


def case_inputs(case, name):
    """what the decoder gets for the case: (features [6, F], cluster vectors, eps [S, 6, L])"""
    _, _, feats, cv, eps, _, _ = controls_ref.pool(case)
    idx = list(IMAGES[(case, name)])
    return feats[idx], cv[idx], eps[:, idx]


def choose_images(case, name, n=6):
    """the first n pool images, in pool order, whose margin exceeds SAFE_MARGIN (how IMAGES was made)"""
    out = []
    for i in range(controls_ref.POOL):
        if image_margin(case, name, i) > SAFE_MARGIN:
            out.append(i)
            if len(out) == n:
                break
    return tuple(out)


# (prior case, setting) -> its six pool images, chosen on the CPU by choose_images; tests/test_contrastive_host.py asserts that every
# case is safe
IMAGES = {
    (0, "plain"): (2, 3, 4, 5, 7, 9),
    (1, "plain"): (1, 2, 3, 5, 10, 11),
    (2, "plain"): (0, 2, 3, 4, 5, 6),
    (3, "plain"): (1, 2, 4, 6, 7, 8),
    (1, "wide"): (0, 1, 3, 6, 12, 17),
    (2, "likelihood_off"): (0, 1, 2, 4, 5, 6),
    (3, "all"): (0, 1, 4, 5, 6, 7),
}
