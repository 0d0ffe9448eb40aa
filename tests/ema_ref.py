"""Weight averaging in numpy float64 (the reference of tests/test_ema_host.py and tests/test_gpu_ema.py).

    w_t = max(1 - decay, 9 / (10 + t))  (t = updates including this one; a constant 1 - decay without the warm-up)
    e_t = e_{t-1} + w_t (p_t - e_{t-1})

The weight is computed as the kernels compute it, in float32 (one add, one correctly rounded divide, one max), and then used in
float64; the recurrence itself runs in float64 over the float32 parameter history."""
import numpy as np

# one subtract and one fused multiply-add per step, each within half an ulp (2^-24 relative) of operands no larger than
# M = max(|p|, |e|): |p - e| <= 2 M, its rounding error is scaled by w <= 1, the fma adds another 2^-24 M -- at most 3 * 2^-24 * M per
# step, carried through a recurrence whose factor 1 - w is at most 1
ULP_BOUND = 3.0 * 2.0 ** -24


def weight(omd, t=None):
    """float32 weight of the new value at update t (None: constant decay)"""
    omd = np.float32(omd)
    if t is None:
        return omd
    return np.maximum(omd, np.float32(9.0) / (np.float32(10.0) + np.float32(t)))


def ema_steps(e0, history, omd, first_t=1, warmup=True):
    """-> (averages after the last step [float64], M = elementwise max over the steps of max(|p_t|, |e_t|, |e_{t-1}|))"""
    e = np.asarray(e0, np.float64).copy()
    M = np.abs(e)
    for k, p in enumerate(history):
        w = np.float64(weight(omd, first_t + k if warmup else None))
        p = np.asarray(p, np.float64)
        e = e + w * (p - e)
        M = np.maximum(M, np.maximum(np.abs(p), np.abs(e)))
    return e, M


def bound(M, n_steps):
    return ULP_BOUND * n_steps * M


def assert_within_bound(got, e0, history, omd, first_t=1, warmup=True, msg=""):
    ref, M = ema_steps(e0, history, omd, first_t, warmup)
    err = np.abs(np.asarray(got, np.float64) - ref)
    tol = bound(M, len(history))
    worst = np.unravel_index(np.argmax(err - tol), err.shape) if err.size else ()
    at = np.unravel_index(np.argmax(err), err.shape) if err.size else ()
    print("%s: max err %.3e (bound there %.3e)" % (msg, err[at] if err.size else 0.0, tol[at] if err.size else 0.0))
    assert np.isfinite(np.asarray(got)).all(), "%s: non-finite average" % msg
    assert (err <= tol).all(), "%s: err %.3e > bound %.3e at %s (%d / %d elements off)" % (msg, err[worst], tol[worst], worst, int((err > tol).sum()), err.size)
