"""Float64 reference of the DPP selection (tests only), written from the definition in include/vaecap.h ("DPP selection"): the greedy
MAP of a determinantal point process over an image's in-set CIDEr-D matrix.

S_ij = min(1, max(0, (G_ij + G_ji) / 20)) off the diagonal, S_ii = 1; L = diag(q) S diag(q); d_i = q_i^2.  Per step: a caption is live
if it is untaken and d_i > DPP_EPS q_i^2; the pick is the live caption with the largest d (equal values: the lower index); every
untaken i gets e = (L_ji - sum_t c_t[j] c_t[i]) / sqrt(d_j), the sum subtracted term by term in ascending t, c_k[i] = e, d_i -= e^2.
`select` is the procedure; `replay` follows a GIVEN sequence of picks and reports at every step the live set and every live candidate's
d, which lets a test accept any pick that the definition's own rounding cannot tell from the best one."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vaecap.h")
DPP_EPS = float(re.search(r"^#define\s+DPP_EPS\s+(\S+)\s*$", open(HEADER).read(), flags=re.M).group(1))   # defined once, in the header


def similarity(G):
    """float64 [m, m]: the symmetrised, clipped matrix with its diagonal set to 1"""
    G = np.asarray(G, np.float64)
    S = np.minimum(1.0, np.maximum(0.0, (G + G.T) / 20.0))
    np.fill_diagonal(S, 1.0)
    return S


def kernel_matrix(G, q):
    q = np.asarray(q, np.float64)
    return q[:, None] * similarity(G) * q[None, :]


class _State(object):
    def __init__(self, G, q):
        self.S = similarity(G)
        self.q = np.asarray(q, np.float64).reshape(-1)
        self.m = int(self.q.size)
        self.d = self.q * self.q
        self.taken = np.zeros(self.m, bool)
        self.c = []   # c_t: float64 [m] per step done

    def live(self):
        return ~self.taken & (self.d > DPP_EPS * self.q * self.q)

    def take(self, j):
        dj = self.d[j]
        self.taken[j] = True
        acc = (self.q[j] * self.S[j]) * self.q            # every i at once; per element the definition's own sequence of operations
        for c in self.c:                                  # ascending t, one subtraction per step done
            acc = acc - c[j] * c
        e = np.where(self.taken, 0.0, acc / np.sqrt(dj))
        self.c.append(e)
        self.d = np.where(self.taken, self.d, self.d - e * e)
        return dj


def _finish(st, n, sel, gain):
    chosen = len(sel)
    want = min(n, st.m)
    rest = np.flatnonzero(~st.taken)[:want - chosen].tolist()
    sel, gain = sel + rest, gain + [0.0] * len(rest)
    pad = n - len(sel)
    return np.array(sel + [-1] * pad, np.int32), np.array(gain + [0.0] * pad, np.float64), chosen


def select(G, q, n):
    """-> (sel int32 [n], gain float64 [n], n_dpp)"""
    st = _State(G, q)
    sel, gain = [], []
    while len(sel) < min(n, st.m):
        live = st.live()
        if not live.any():
            break
        j = int(np.argmax(np.where(live, st.d, -1.0)))   # the first maximum: equal values go to the lower index
        sel.append(j)
        gain.append(float(st.take(j)))
    return _finish(st, n, sel, gain)


def replay(G, q, n, picks):
    """Follow `picks` (indices within the image, at most min(n, m) of them) through the definition.  -> (steps, tail): steps[k] =
    dict(live: bool [m], taken: bool [m], d: float64 [m] -- all BEFORE pick k is taken) and tail = (sel, gain, n_dpp) as `select` would end after
    exactly these picks: whether a further caption is live (the loop would go on), then the fill and the -1 / 0 slots."""
    st = _State(G, q)
    steps, gain = [], []
    for j in picks:
        steps.append(dict(live=st.live(), taken=st.taken.copy(), d=st.d.copy()))
        gain.append(float(st.take(int(j))))
    more = bool(st.live().any()) and len(picks) < min(n, st.m)
    sel, g, chosen = _finish(st, n, [int(j) for j in picks], gain)
    return steps, dict(sel=sel, gain=g, n_dpp=chosen, more=more, ratios=st.d[~st.taken] / (st.q[~st.taken] ** 2))


def quality(keys, weight):
    """mbr.dpp_quality's definition: r = (key - min) / (max - min) over the finite keys (0 when they are all equal, 0 for a non-finite
    key), q = exp(weight * r)"""
    k = np.asarray(keys, np.float64).reshape(-1)
    fin = np.isfinite(k)
    r = np.zeros(k.size, np.float64)
    if fin.any():
        lo, hi = k[fin].min(), k[fin].max()
        if hi > lo:
            r[fin] = (k[fin] - lo) / (hi - lo)
    return np.exp(float(weight) * r)
