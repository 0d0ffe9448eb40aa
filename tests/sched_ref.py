"""Host reference of scheduled sampling (vc_sched_mix_f32, csrc/sched.hip; DESIGN.md "Scheduled sampling"): float64 numpy written from
the definition, no product code.

    eligible  position (t, n) of the time-major [T, N] decoder inputs iff 1 <= t < lens[n]
    selected  an eligible position iff coin[t, n] < rate (strict)
    the word  of a selected position comes from logits row (t - 1) * N + n: the inverse-CDF draw of softmax(x / temperature) with
              u[t, n] (the first word whose cumulative probability exceeds u), or the first maximum when u is None
    the rest  copies cap_dec_t
"""
import math

import numpy as np

SCHEDULES = ("constant", "linear", "sigmoid")


def sched_rate(step, schedule, rate_max, ramp_steps):
    """rate of global step `step` (0 = the first optimiser step): constant R; linear R * min(1, s / K); sigmoid
    R * (1 - K / (K + exp(s / K))) (Bengio et al. 2015, eq. 3, as a sampling rate)"""
    name = SCHEDULES[schedule] if isinstance(schedule, (int, np.integer)) else schedule
    s, k = float(max(step, 0)), float(ramp_steps)
    if name == "constant":
        return float(rate_max)
    if name == "linear":
        return float(rate_max) * min(1.0, s / k)
    assert name == "sigmoid", schedule
    x = s / k
    e = math.exp(x) if x < 700.0 else float("inf")
    return float(rate_max) * (1.0 - k / (k + e))


def eligible(T, N, lens):
    t = np.arange(T)[:, None]
    return (t >= 1) & (t < np.asarray(lens).reshape(1, N))


def cdf64(row, temperature):
    """cumulative softmax(row / temperature) in float64, normalised to end at exactly 1"""
    y = np.asarray(row, np.float64) / float(temperature)
    e = np.exp(y - y.max())
    c = np.cumsum(e)
    return c / c[-1]


def mix(logits, cap_dec_t, lens, coin, u, temperature, rate):
    """-> (tokens [T, N] int32, {(t, n): float64 CDF [V] of the row a selected position draws from}).  logits: [T * N, V] (only the
    rows of selected positions are read); u None = argmax.  rate is compared with the float32 coins as a float32 (the kernel's)."""
    cap = np.asarray(cap_dec_t)
    T, N = cap.shape
    lg = np.asarray(logits).reshape(T * N, -1)
    sel = eligible(T, N, lens) & (np.asarray(coin, np.float32).reshape(T, N) < np.float32(rate))
    out = cap.astype(np.int32).copy()
    cdfs = {}
    for t, n in zip(*np.nonzero(sel)):
        row = lg[(t - 1) * N + n]
        if u is None:
            out[t, n] = int(np.argmax(row))   # the first maximum
            continue
        c = cdf64(row, temperature)
        cdfs[(int(t), int(n))] = c
        out[t, n] = min(int(np.searchsorted(c, np.float64(np.asarray(u).reshape(T, N)[t, n]), side="right")), row.size - 1)
    return out, cdfs


def delta(V):
    """What the kernel's float32 sums may move a CDF value by: chunk sums of <= ceil(V / 256) terms, the 256-term serial sum and the
    final comparison lose at most one ulp per addition, __expf a few ulp per term; twice their sum."""
    return (math.ceil(V / 256) + 256 + 8) * 2.0 ** -23


def accepts(cdf, w, u):
    """the kernel's word w for uniform u is right iff cdf[w - 1] - delta <= u < cdf[w] + delta"""
    d = delta(cdf.size)
    lo = cdf[w - 1] if w > 0 else 0.0
    return 0 <= w < cdf.size and lo - d <= float(u) < cdf[w] + d
