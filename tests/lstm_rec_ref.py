"""The H = 512 recurrence kernels of csrc/lstm.hip, restated for the tests (numpy only, no GPU, no call into the library):

  * the dispatch arithmetic of rec_fwd / rec8_fwd / rec_bwd: which instantiation a row count runs, how many rows a workgroup
    gets, how many passes it takes over them and how many rows its last workgroup is left with;
  * case tables: row counts on each side of every boundary of that arithmetic, as functions of the CU count, each with the
    path it must land on (tests/test_lstm_rec_cases.py checks the tables themselves, tests/test_gpu_lstm_rec.py runs them);
  * the fp64 back-propagation through time with everything the device call leaves behind: dG of every step, d hs[1] (dH_run on
    exit) and d cs[0] (dC_run on exit), next to the oracle's reductions of dG."""
from collections import namedtuple

import numpy as np

from oracle import ops as O

SENTINEL = np.float32(-7.25)   # guard rows around every output buffer: they must be left alone
GUARD = 3                      # guard rows on each side
BWD_CT2_ROWS = 600             # VC_LSTM_BWD_CT2_ROWS


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- dispatch arithmetic (csrc/lstm.hip)
def row_groups(N, UG, cus):
    """rec_row_groups: one workgroup per CU over UG column slices, at least 16 rows per group"""
    return min(max(cus // UG, 1), cdiv(N, 16))


BwdPath = namedtuple("BwdPath", "CT RT RG rows passes last_group_rows")


def bwd_path(N, cus):
    """rec_bwd -> lstm_rec_bwd_kernel<RT, BX, CT>: CT = 2 column tiles (32 units, 16 column slices) from 600 rows on, else CT = 1
    (32 slices); RG row groups of `rows` rows; RT = 5 row tiles per pass when a group has more than 48 rows, else 3; the kernel
    loops over passes of 16 RT rows.  last_group_rows: what the last workgroup that has any row is left with"""
    CT, UG = (2, 16) if N >= BWD_CT2_ROWS else (1, 32)
    RG = row_groups(N, UG, cus)
    rows = cdiv(N, RG)
    RT = 5 if rows > 48 else 3
    return BwdPath(CT, RT, RG, rows, cdiv(rows, 16 * RT), N - (cdiv(N, rows) - 1) * rows)


def fwd_path(N, cus):
    """the sequence forward at H = 512 -> (kernel, rows per workgroup, passes): rec8_fwd above 400 rows (80-row passes), else
    rec_fwd with RT = 5 row tiles when a workgroup has more than 48 rows (16 RT-row passes), RT = 3 otherwise"""
    if N > 400:
        rows = cdiv(N, row_groups(N, 32, cus))
        return "rec8", rows, cdiv(rows, 80)
    rows = cdiv(N, row_groups(N, 64, cus))
    rt = 5 if rows > 48 else 3
    return "rec-rt%d" % rt, rows, cdiv(rows, 16 * rt)


def g4(cus):
    return max(cus // 64, 1)


def g8(cus):
    return max(cus // 32, 1)


def g16(cus):
    return max(cus // 16, 1)


# (id, N from the CU count, check of bwd_path(N, cus)); on 256 CUs: 1, 16, 17, 384, 385, 599, 600, 768, 769, 997, 1280, 1281, 1700
BWD_CASES = [
    ("ct1-rt3-1row", lambda cus: 1, lambda p: (p.CT, p.RT) == (1, 3) and p.rows == 1),
    ("ct1-rt3-one-tile", lambda cus: 16, lambda p: (p.CT, p.RT) == (1, 3) and p.rows == 16),
    ("ct1-rt3-2groups", lambda cus: 17, lambda p: (p.CT, p.RT) == (1, 3) and p.RG == 2 and p.rows == 9),
    ("ct1-rt3-48rows", lambda cus: 48 * g8(cus), lambda p: (p.CT, p.RT) == (1, 3) and p.rows == 48 and p.passes == 1),
    ("ct1-rt5-49rows", lambda cus: 48 * g8(cus) + 1, lambda p: (p.CT, p.RT) == (1, 5) and p.rows == 49),
    ("ct1-rt5-599", lambda cus: 599, lambda p: (p.CT, p.RT) == (1, 5) and p.last_group_rows % 16 != 0),
    ("ct2-rt3-600", lambda cus: 600, lambda p: (p.CT, p.RT) == (2, 3)),
    ("ct2-rt3-48rows", lambda cus: 48 * g16(cus), lambda p: (p.CT, p.RT) == (2, 3) and p.rows == 48),
    ("ct2-rt5-49rows", lambda cus: 48 * g16(cus) + 1, lambda p: (p.CT, p.RT) == (2, 5) and p.rows == 49),
    ("ct2-rt5-prime", lambda cus: 997, lambda p: (p.CT, p.RT) == (2, 5)),
    ("ct2-rt5-1pass-full", lambda cus: 80 * g16(cus), lambda p: (p.CT, p.RT) == (2, 5) and p.rows == 80 and p.passes == 1),
    ("ct2-rt5-2pass", lambda cus: 80 * g16(cus) + 1, lambda p: (p.CT, p.RT) == (2, 5) and p.rows == 81 and p.passes == 2),
    ("ct2-rt5-2pass-ragged", lambda cus: 1700, lambda p: (p.CT, p.RT) == (2, 5) and p.passes >= 2 and p.last_group_rows % 16 != 0),
]
# what bwd_path gives for each case on the 256 CUs of an MI355X
BWD_ON_256 = {
    "ct1-rt3-1row": (1, BwdPath(1, 3, 1, 1, 1, 1)),
    "ct1-rt3-one-tile": (16, BwdPath(1, 3, 1, 16, 1, 16)),
    "ct1-rt3-2groups": (17, BwdPath(1, 3, 2, 9, 1, 8)),
    "ct1-rt3-48rows": (384, BwdPath(1, 3, 8, 48, 1, 48)),
    "ct1-rt5-49rows": (385, BwdPath(1, 5, 8, 49, 1, 42)),
    "ct1-rt5-599": (599, BwdPath(1, 5, 8, 75, 1, 74)),
    "ct2-rt3-600": (600, BwdPath(2, 3, 16, 38, 1, 30)),
    "ct2-rt3-48rows": (768, BwdPath(2, 3, 16, 48, 1, 48)),
    "ct2-rt5-49rows": (769, BwdPath(2, 5, 16, 49, 1, 34)),
    "ct2-rt5-prime": (997, BwdPath(2, 5, 16, 63, 1, 52)),
    "ct2-rt5-1pass-full": (1280, BwdPath(2, 5, 16, 80, 1, 80)),
    "ct2-rt5-2pass": (1281, BwdPath(2, 5, 16, 81, 2, 66)),
    "ct2-rt5-2pass-ragged": (1700, BwdPath(2, 5, 16, 107, 2, 95)),
}


def bwd_case_ct(name):
    """the column-tile count a backward case is about (its id says so)"""
    return int(name[2])


def bwd_case_skip_reason(name, N, cus):
    """None, or why the case cannot run on this CU count: its N lies on the other side of the 600-row threshold there"""
    want, got = bwd_case_ct(name), bwd_path(N, cus).CT
    if want == got:
        return None
    return "%s: N = %d on %d CUs is %s the %d-row CT = 2 threshold, the case needs CT = %d" % (
        name, N, cus, "below" if got == 1 else "at or above", BWD_CT2_ROWS, want)


# (id, N from the CU count, check of (kernel, rows, passes)) for the split-bf16 forward; on 256 CUs: 1, 16, 17, 192, 193, 320, 321,
# 400, 401, 640, 641, 997, 1281
FWD_BX_CASES = [
    ("rec-rt3-1row", lambda cus: 1, lambda k, r, p: k == "rec-rt3" and r == 1),
    ("rec-rt3-one-tile", lambda cus: 16, lambda k, r, p: k == "rec-rt3" and r == 16),
    ("rec-rt3-2groups", lambda cus: 17, lambda k, r, p: k == "rec-rt3" and r == 9),
    ("rec-rt3-48rows", lambda cus: 48 * g4(cus), lambda k, r, p: k == "rec-rt3" and r == 48 and p == 1),
    ("rec-rt5-49rows", lambda cus: 48 * g4(cus) + 1, lambda k, r, p: k == "rec-rt5" and r == 49 and p == 1),
    ("rec-rt5-1pass-full", lambda cus: 80 * g4(cus), lambda k, r, p: k == "rec-rt5" and r == 80 and p == 1),
    ("rec-rt5-2pass", lambda cus: 80 * g4(cus) + 1, lambda k, r, p: k == "rec-rt5" and p == 2),
    ("rec-rt5-400rows", lambda cus: 400, lambda k, r, p: k == "rec-rt5" and p >= 2),
    ("rec8-401rows", lambda cus: 401, lambda k, r, p: k == "rec8"),
    ("rec8-1pass-full", lambda cus: 80 * g8(cus), lambda k, r, p: k == "rec8" and r == 80 and p == 1),
    ("rec8-2pass", lambda cus: 80 * g8(cus) + 1, lambda k, r, p: k == "rec8" and p >= 2),
    ("rec8-prime", lambda cus: 997, lambda k, r, p: k == "rec8" and p >= 2),
    ("rec8-1281rows", lambda cus: 1281, lambda k, r, p: k == "rec8" and p >= 2),
]
FWD_BX_NS_ON_256 = [1, 16, 17, 192, 193, 320, 321, 400, 401, 640, 641, 997, 1281]


# ----------------------------------------------------------------------------- inputs
def make_lens(rng, N, T):
    """effective lengths in [0, T]: the first and the last row run every step, row 1 none and row 2 one (when there are that many)"""
    lens = rng.integers(0, T + 1, size=N).astype(np.int32)
    lens[0] = T
    lens[N - 1] = T
    if N > 3:
        lens[1], lens[2] = 0, 1
    return lens


def _f32(a):
    return np.asarray(a).astype(np.float32)


def make_fwd_problem(N, T, E, H, seed):
    """a sequence from a NON-zero initial state (with zeros, step 0 multiplies zeros and tests nothing of the recurrent product):
    f32 inputs and the fp64 forward on exactly those values"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, N, E), dtype=np.float32)
    W = rng.standard_normal((E + H, 4 * H), dtype=np.float32) * np.float32(1.0 / np.sqrt(E + H))
    b = rng.standard_normal(4 * H, dtype=np.float32) * np.float32(0.1)
    c0 = rng.standard_normal((N, H), dtype=np.float32)
    h0 = _f32(np.tanh(rng.standard_normal((N, H))))
    lens = make_lens(rng, N, T)
    cache = O.lstm_seq_fwd(X.astype(np.float64), lens, W.astype(np.float64), b.astype(np.float64), c0=c0.astype(np.float64),
                           h0=h0.astype(np.float64))
    return dict(T=T, N=N, E=E, H=H, X=X, W=W, b=b, c0=c0, h0=h0, lens=lens, cache=cache)


def make_bwd_problem(N, T, E, H, seed, with_ext=True):
    """a backward problem whose device inputs ARE the reference's forward values: the fp64 forward from a non-zero state, its act /
    cs / hs rounded once to f32 and put back into the cache, so that only the backward is under test.  Non-zero dH_run and dC_run on
    entry, an external gradient on hs[1..T] (index T comes on top of dH_run; index 0 is never read) unless with_ext is False."""
    p = make_fwd_problem(N, T, E, H, seed)
    cache = p["cache"]
    for k in ("act", "cs", "hs"):
        p[k] = _f32(cache[k])
        cache[k] = p[k].astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    p["dH0"] = _f32(rng.standard_normal((N, H)) * 0.1)
    p["dC0"] = _f32(rng.standard_normal((N, H)) * 0.1)
    ext = _f32(rng.standard_normal((T + 1, N, H)) * 0.1)
    ext[0] = SENTINEL    # never read: a kernel that did read it would show
    p["dhs_ext"] = ext if with_ext else None
    dhs = np.zeros((T + 1, N, H))
    dhs[T] = p["dH0"].astype(np.float64)
    if with_ext:
        dhs[1:] += ext[1:].astype(np.float64)
    p["ref"] = bptt_ref(cache, dhs, p["dC0"].astype(np.float64), p["lens"], cache["W"][E:])
    for v in list(p.values()) + list(p["ref"].values()) + list(cache.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)   # shared between tests: nobody changes it
    return p


# ----------------------------------------------------------------------------- fp64 back-propagation through time
def bptt_ref(cache, dhs, dc_last, lens, Wh):
    """The oracle's loop (oracle/ops.py lstm_seq_bwd) restated to keep what it only returns reductions of.  dhs [T+1,N,H]: gradient
    w.r.t. every hs[t] (index T includes what dH_run holds on entry), dc_last: gradient w.r.t. cs[T].
    -> dict: dG [T,N,4H], dh1 (gradient w.r.t. hs[1]: what dH_run holds on exit), dc0 (w.r.t. cs[0]: dC_run on exit), and the
    oracle's own dX, dW, db.  The restated loop is held to the oracle through dc0 (1e-12)."""
    act, cs = cache["act"], cache["cs"]
    T, N, H = act.shape[0], act.shape[1], cs.shape[2]
    lens = np.asarray(lens)
    dG = np.zeros((T, N, 4 * H))
    dh, dc = dhs[T].copy(), dc_last.copy()
    for t in range(T - 1, -1, -1):
        i, j, f, o = (act[t][:, k * H:(k + 1) * H] for k in range(4))
        m = (t < lens)[:, None]
        tc = np.tanh(cs[t + 1])
        dct = dc + dh * o * (1 - tc * tc)
        g = np.concatenate([dct * j * i * (1 - i), dct * i * (1 - j * j), dct * cs[t] * f * (1 - f), dh * tc * o * (1 - o)], 1)
        dG[t] = np.where(m, g, 0)
        dc = np.where(m, dct * f, dc)
        if t > 0:
            dh = np.where(m, dG[t] @ Wh.T, dh) + dhs[t]
    rdX, rdW, rdb, rdc, _ = O.lstm_seq_bwd(cache, dhs, dc_last=dc_last)
    err = np.abs(dc - rdc).max()
    assert err <= 1e-12 * np.abs(rdc).max() + 1e-30, "restated loop != oracle (dc0): %.3e" % err
    return dict(dG=dG, dh1=dh, dc0=dc, dX=rdX, dW=rdW, db=rdb)
