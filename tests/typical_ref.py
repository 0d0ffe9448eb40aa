"""Host reference of typical / min-p / eta sampling (vc_decode_pick_typical_f32; DESIGN.md "Typical / min-p / eta sampling"): numpy
float64 on the f32 scaled logits, plus the inputs that tests/test_typical_host.py (CPU) and tests/test_gpu_typical.py share.

One row x[0..V), temperature t > 0, 0 < tau <= 1, 0 <= min_p <= 1, 0 <= eta < 1, uniform u in [0, 1):
  y = fl32(x * fl32(1 / t)); p = softmax(y) over the full row; H = -sum p log p (a word of zero mass adds 0);
  typical set = d = |-log p - H| ascending, equal d by lower index: the shortest prefix whose mass is >= tau, at least one word (tau = 1: all);
  floor set = p >= max(min_p * p_max, min(eta, sqrt(eta) * exp(-H)));  kept = typical AND floor, never a word of zero mass; empty: the first
  maximum of y;  draw = the lowest-index kept word whose running kept mass (index order) exceeds u * (kept mass), else the last kept word.
A row is `safe` when f32 arithmetic cannot flip the reference's decisions: one word kept, or all of
  * the cumulative shares on both sides of the typical cut are >= MARGIN away from tau (trunc_ref's budget of the masses),
  * no word with d != d_cut has |d - d_cut| < DMARGIN * (1 + H),
  * no word has |p / floor - 1| < DMARGIN * (1 + H),
  * the target is >= MARGIN * (kept mass) away from both edges of the chosen word's interval.
DMARGIN = 2e-5: the masses are good to ~8e-6 relative (trunc_ref), |dH| <= eps * sum p |log p + 1| <= eps * (1 + H), and the factor 2.5
over that covers d's own rounding.  The device's entropy[] is held to the same DMARGIN * (1 + H).
`wide_set` = the kept set plus every word inside those margins (and the first maximum): an unsafe row's token must lie in it."""
import numpy as np

from .trunc_ref import MARGIN, MAX_UNSAFE, PAD, ROWS, SHAPES, log_softmax64, scaled  # noqa: F401  (shared with the truncation's tests)

DMARGIN = 2e-5
FLT_MAX = float(np.finfo(np.float32).max)
SETTINGS = [(0.9, 0.0, 0.0, 1.0), (0.2, 0.0, 0.0, 1.0), (1.0, 0.05, 0.0, 0.8), (1.0, 0.0, 3e-3, 1.0), (0.9, 0.02, 1e-3, 0.7)]   # (tau, min_p, eta, t)
SETTING_IDS = ["tau%g-m%g-eta%g-t%g" % s for s in SETTINGS]
# [shape][setting]: for each case the first seed of 2000 + 100 * shape + 10 * setting + 1000 * n whose rows stay within the unsafe-row cap
# (tests/test_typical_host.py asserts the cap for every case; `python -m tests.typical_ref` repeats the search)
SEEDS = [[2000 + 100 * i + 10 * j for j in range(5)] for i in range(5)]
SEEDS[3][0], SEEDS[4][0] = 15300, 20400   # (tau = 0.9 at V >= 10 000: one to three random rows in 64 sit inside a margin)
BANNED_ROW, BANNED = 13, 20   # the row with words at -FLT_MAX (what the decoding controls write for a banned word), and how many


def entropy_of(y):
    """(p, log p, H) of one scaled row in float64; log p = -inf and p = 0 where the mass underflows or y = -inf."""
    y = np.asarray(y, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = y - y.max()
        w = np.exp(g)
        z = w.sum()
        p = w / z
        logp = np.where(p > 0, g - np.log(z), -np.inf)
        h = -np.sum(np.where(p > 0, p * logp, 0.0))
    return p, logp, float(h)


def typical_row(x, t, tau, min_p, eta, u):
    """-> dict(token, kept, safe, kept_set (sorted indices), wide_set (sorted indices), H)."""
    x = np.asarray(x, np.float32)
    V = x.shape[0]
    with np.errstate(over="ignore"):   # (-FLT_MAX / t overflows to -inf at t < 1: the row's point)
        y = scaled(x, t).astype(np.float64)
    p, logp, H = entropy_of(y)
    tau, min_p, eta = float(np.float32(tau)), float(np.float32(min_p)), float(np.float32(eta))
    live = p > 0
    first_max = int(np.argmax(y))
    dm = DMARGIN * (1.0 + H)
    safe = True
    # ---- typical set
    typ = live.copy()
    typ_wide = live.copy()
    if tau < 1.0:
        with np.errstate(invalid="ignore"):
            d = np.where(live, np.abs(-logp - H), np.inf)
        order = np.argsort(d, kind="stable")
        cum = np.cumsum(p[order])
        hit = cum >= tau
        n = int(np.argmax(hit)) + 1 if hit.any() else int(live.sum())
        typ = np.zeros(V, bool)
        typ[order[:n]] = True
        d_cut = d[order[n - 1]]
        below = cum[n - 2] if n >= 2 else -np.inf
        near = live & (d != d_cut) & (np.abs(d - d_cut) < dm)
        share_ok = (cum[n - 1] - tau >= MARGIN) and (tau - below >= MARGIN)
        safe = safe and share_ok and not near.any()
        typ_wide = typ | near
        if n < V and live[order[n]]:
            typ_wide[order[n]] = True   # (the next word of the order: what a cut one word later adds)
    # ---- floor set
    fl = max(min_p * p.max(), min(eta, np.sqrt(eta) * np.exp(-H)))
    flo = live.copy()
    flo_wide = live.copy()
    if fl > 0.0:
        flo = live & (p >= fl)
        near = live & (np.abs(p / fl - 1.0) < dm)
        safe = safe and not near.any()
        flo_wide = flo | near
    keep = typ & flo
    if not keep.any():
        keep = np.zeros(V, bool)
        keep[first_max] = True
    wide = typ_wide & flo_wide
    wide |= keep
    wide[first_max] = True
    kept = np.nonzero(keep)[0]
    n = int(kept.size)
    w = np.exp(y - y.max())
    cdf = np.cumsum(w[kept])
    z = cdf[-1]
    target = float(np.float32(u)) * z
    hit = np.nonzero(cdf > target)[0]
    i = int(hit[0]) if hit.size else n - 1
    lo = cdf[i - 1] if i > 0 else 0.0
    safe = safe and (target - lo >= MARGIN * z) and (cdf[i] - target >= MARGIN * z)
    if n == 1:
        safe = True
    return dict(token=int(kept[i]), kept=n, safe=bool(safe), kept_set=kept, wide_set=np.nonzero(wide)[0], H=H)


def typical_rows(x, t, tau, min_p, eta, u):
    return [typical_row(x[r], t, tau, min_p, eta, u[r]) for r in range(x.shape[0])]


def typical_probs(x, t, tau, min_p, eta):
    """The renormalised distribution over the kept set of one row (float64 [V])."""
    r = typical_row(x, t, tau, min_p, eta, 0.5)
    with np.errstate(over="ignore"):
        y = scaled(x, t).astype(np.float64)
    w = np.exp(y - y.max())
    out = np.zeros_like(w)
    out[r["kept_set"]] = w[r["kept_set"]]
    return out / out.sum()


def make_case(shape_i, setting_i, seed=None):
    """The inputs of one (shape, setting) case: (x [ROWS, ld] f32 with PAD in the padding columns, V, ld, tau, min_p, eta, t, u [ROWS] f32).
    Planted rows: 3 rounded logits (exact ties in y and hence in d), 5 one logit raised by 50 (one word holds all the mass), 7 all-equal
    logits (every d equal: the cut is by index), 9 u = 0, 11 u = 0.999999 (both on an edge of their word's interval: unsafe by the rule
    unless one word is kept), 13 BANNED words (fewer at V = 7) at -FLT_MAX, which t < 1 scales to -inf."""
    V, ld = SHAPES[shape_i]
    tau, min_p, eta, t = SETTINGS[setting_i]
    rng = np.random.default_rng(SEEDS[shape_i][setting_i] if seed is None else seed)
    x = np.full((ROWS, ld), PAD, np.float32)
    x[:, :V] = (rng.standard_normal((ROWS, V)) * 4.0).astype(np.float32)
    u = rng.random(ROWS).astype(np.float32)
    x[3, :V] = np.round(x[3, :V])
    x[5, int(rng.integers(V))] += 50.0
    x[7, :V] = 1.25
    u[9] = 0.0
    u[11] = 0.999999
    x[BANNED_ROW, rng.choice(V, size=min(BANNED, V // 2), replace=False)] = -FLT_MAX
    return x, V, ld, tau, min_p, eta, t, u


def unsafe_rows(shape_i, setting_i, seed=None):
    x, V, ld, tau, min_p, eta, t, u = make_case(shape_i, setting_i, seed)
    ref = typical_rows(x[:, :V], t, tau, min_p, eta, u)
    return [r for r in range(ROWS) if not ref[r]["safe"]]


if __name__ == "__main__":   # the seed search behind SEEDS
    for i in range(len(SHAPES)):
        row = []
        for j in range(len(SETTINGS)):
            s = 2000 + 100 * i + 10 * j
            while len(unsafe_rows(i, j, s)) > MAX_UNSAFE * ROWS:
                s += 1000
            row.append(s)
        print(row)
