"""Host reference of truncated sampling (vc_decode_pick_trunc_f32; DESIGN.md "Truncated sampling"): numpy float64 on the f32 scaled
logits, plus the inputs that tests/test_trunc_host.py (CPU) and tests/test_gpu_trunc.py share.

One row x[0..V), temperature t > 0, top_k >= 0, 0 < top_p <= 1, uniform u in [0, 1):
  y = fl32(x * fl32(1 / t)); order = y descending, equal y by lower index; top-k = the first top_k words of the order (0 or >= V: all);
  w = exp(y - max y); nucleus = the shortest prefix of the top-k set whose mass is >= top_p * (the set's mass), at least one word;
  draw = the lowest-index kept word whose running kept mass (index order) exceeds u * (kept mass), else the last kept word.
A row is `safe` when f32 arithmetic cannot flip the reference's decisions: one word kept, or the cumulative shares on both sides of the
nucleus cut are >= MARGIN away from top_p and the target is >= MARGIN * (kept mass) away from both edges of the chosen word's interval.
MARGIN = 1e-5: chunked f32 sums of <= 13 000 positive terms err by < 4e-6 relative, the device exponential and the rounding of its argument
add about 2e-6, masses held as multiples of 2^-32 add < 2e-6.  Top-k membership needs no margin (exact f32 keys and index order)."""
import numpy as np

MARGIN = 1e-5
MAX_UNSAFE = 0.05   # share of a case's rows that may be unsafe

SHAPES = [(7, 7), (40, 40), (1001, 1008), (10000, 10000), (13000, 13000)]   # (V, ld); 13 000 is wider than the staged width
SETTINGS = [(0, 0.9, 1.0), (40, 1.0, 0.7), (50, 0.95, 0.8), (0, 0.3, 1.0), (-5, 1.0, 1.0)]   # (top_k, top_p, t); top_k < 0: V - top_k
ROWS = 64
SEEDS = [[1000 + 10 * i + j for j in range(5)] for i in range(5)]   # [shape][setting]
SEEDS[3][0], SEEDS[4][0] = 1630, 1140   # (the first seeds of 1030 + 100 n / 1040 + 100 n whose random rows are all safe)
PAD = 77.0


def scaled(x, t):
    inv_t = np.float32(1.0) / np.float32(t)
    return (np.asarray(x, np.float32) * inv_t).astype(np.float32)   # one rounded f32 multiply per word


def order_of(y):
    return np.argsort(-y.astype(np.float64), kind="stable")   # descending, equal values (-0 == +0 too) by lower index


def trunc_row(x, t, top_k, top_p, u):
    """-> dict(token, kept, safe, kept_set (sorted indices), wide_set (kept set + the next word of the order, inside the top-k set))."""
    x = np.asarray(x, np.float32)
    V = x.shape[0]
    y = scaled(x, t).astype(np.float64)
    order = order_of(y)
    k = V if (top_k == 0 or top_k >= V) else int(top_k)
    w = np.exp(y - y.max())
    ws = w[order[:k]]
    cum = np.cumsum(ws)
    zk = cum[-1]
    p = float(np.float32(top_p))
    safe = True
    if p >= 1.0:
        n = k
    else:
        n = int(np.argmax(cum >= p * zk)) + 1 if (cum >= p * zk).any() else k
        below = cum[n - 2] / zk if n >= 2 else -np.inf
        safe = (cum[n - 1] / zk - p >= MARGIN) and (p - below >= MARGIN)
    kept = np.sort(order[:n])
    cdf = np.cumsum(w[kept])
    z = cdf[-1]
    target = float(np.float32(u)) * z
    hit = np.nonzero(cdf > target)[0]
    i = int(hit[0]) if hit.size else n - 1
    lo = cdf[i - 1] if i > 0 else 0.0
    safe = safe and (target - lo >= MARGIN * z) and (cdf[i] - target >= MARGIN * z)
    if n == 1:
        safe = True
    return dict(token=int(kept[i]), kept=n, safe=bool(safe), kept_set=kept, wide_set=np.sort(order[:min(k, n + 1)]))


def trunc_rows(x, t, top_k, top_p, u):
    return [trunc_row(x[r], t, top_k, top_p, u[r]) for r in range(x.shape[0])]


def truncated_probs(x, t, top_k, top_p):
    """The renormalised truncated distribution of one row (float64 [V])."""
    r = trunc_row(x, t, top_k, top_p, 0.5)
    y = scaled(x, t).astype(np.float64)
    w = np.exp(y - y.max())
    out = np.zeros_like(w)
    out[r["kept_set"]] = w[r["kept_set"]]
    return out / out.sum()


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def make_case(shape_i, setting_i):
    """The inputs of one (shape, setting) case: (x [ROWS, ld] f32 with PAD in the padding columns, V, ld, top_k, top_p, t, u [ROWS] f32).
    Planted rows: 3 rounded logits (many exact ties across both cuts, -0.0 beside +0.0: np.round keeps the sign), 5 one logit raised
    by 50 (one word kept), 7 all-equal logits, 9 u = 0, 11 u = 0.999999.  The last two sit on an edge of their word's interval and are
    unsafe by the rule unless one word is kept, as is the all-equal row where top_p * V is a whole number: SEEDS gives each case random
    rows that leave it within MAX_UNSAFE (tests/test_trunc_host.py checks every case)."""
    V, ld = SHAPES[shape_i]
    top_k, top_p, t = SETTINGS[setting_i]
    if top_k < 0:
        top_k = V - top_k
    rng = np.random.default_rng(SEEDS[shape_i][setting_i])
    x = np.full((ROWS, ld), PAD, np.float32)
    x[:, :V] = (rng.standard_normal((ROWS, V)) * 4.0).astype(np.float32)
    u = rng.random(ROWS).astype(np.float32)
    x[3, :V] = np.round(x[3, :V])
    x[5, int(rng.integers(V))] += 50.0
    x[7, :V] = 1.25
    u[9] = 0.0
    u[11] = 0.999999
    return x, V, ld, top_k, top_p, t, u
