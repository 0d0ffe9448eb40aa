"""-m gpu: the H = 512 recurrence kernels of csrc/lstm.hip at every launch boundary, in both precisions, against fp64.

Backward: the eight instantiations of lstm_rec_bwd_kernel<RT, BX, CT> through vc_lstm_seq_bwd_data_f32, at the row counts of
tests/lstm_rec_ref.py BWD_CASES (each side of the 600-row CT threshold, of the 48-rows-per-workgroup RT threshold and of the
one-pass limit of 80 rows, with whole and ragged last row blocks).  Each case asserts first that the dispatch arithmetic, restated in
lstm_rec_ref.py, puts its N on the variant its id names on this device's CU count.  The call starts from non-zero dH_run AND dC_run,
takes an external gradient on every state, and everything it leaves behind is compared: dG of every step, dX, dH_run (d hs[1]) and
dC_run (d cs[0]); then vc_lstm_seq_bwd_weights_f32 on that dG, and the fused vc_lstm_seq_bwd_f32 bit for bit against the two calls.
Forward: lstm_rec_fwd_kernel<3|5, true> and lstm_rec8_fwd_kernel<true> through vc_lstm_seq_fwd_f32 from a non-zero state.
Every output sits between guard rows that must come back untouched, and starts out as sentinels so that an element left unwritten
shows.

Tolerances (of the tensor maximum, gpu_util.assert_close) are the project's: f32 2e-5 on states and activations and 5e-5 on
gradients (tests/test_gpu_ops.py), split-bf16 four times those (tests/test_gpu_bf16x3.py)."""
import functools

import numpy as np
import pytest
import torch

from . import lstm_rec_ref as R
from .gpu_util import P, assert_close, dev, empty_bytes, host, stream

pytestmark = pytest.mark.gpu
H = 512
FLAGS = {"f32": 4, "bf16x3": 4 | 0x10}                     # VC_LSTM_KERNELS(3) [| VC_LSTM_BF16X3]
TOL = {"f32": (2e-5, 5e-5), "bf16x3": (8e-5, 2e-4)}        # (states / activations, gradients)
SENTINEL, GUARD = R.SENTINEL, R.GUARD


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded(object):
    """a device array of rows, all sentinels unless `init` is given, with GUARD sentinel rows before the first and after the last;
    .ptr is the interior (guard rows are whole rows, so it stays 16-byte aligned)"""

    def __init__(self, shape, init=None):
        self.shape, self.width = tuple(shape), shape[-1]
        self.rows = int(np.prod(shape[:-1]))
        full = np.full((self.rows + 2 * GUARD, self.width), SENTINEL, np.float32)
        if init is not None:
            full[GUARD:GUARD + self.rows] = np.asarray(init, np.float32).reshape(self.rows, self.width)
        self.t = dev(full)
        self.ptr = self.t.data_ptr() + GUARD * self.width * 4
        assert self.ptr % 16 == 0
        self.full = None

    def fetch(self):
        self.full = host(self.t)
        return self

    @property
    def value(self):
        return self.full[GUARD:GUARD + self.rows].reshape(self.shape)

    def guards_intact(self):
        return bool((self.full[:GUARD] == SENTINEL).all() and (self.full[GUARD + self.rows:] == SENTINEL).all())


def up(a):
    """upload a copy (the shared problems are read-only arrays)"""
    return dev(np.array(a))


def check(got, ref, tol, msg):
    """assert_close, with the figure printed first (max error over the tensor maximum)"""
    scale = np.abs(ref).max()
    print("%-44s %.3e of max (bound %.1e)" % (msg, np.abs(np.asarray(got, np.float64) - ref).max() / (scale + 1e-300), tol))
    assert_close(got, ref, tol, msg=msg)


# ----------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=2)
def bwd_problem(N, T=3, E=8, with_ext=True):
    """inputs and fp64 reference, computed once per row count and shared by both precisions (read-only)"""
    return R.make_bwd_problem(N, T, E, H, seed=7 * N + 1, with_ext=with_ext)


def run_bwd(lib, p, flags, fused):
    """the backward on fresh device copies of the problem's inputs: vc_lstm_seq_bwd_data_f32 then vc_lstm_seq_bwd_weights_f32 on the dG
    it left, or the fused vc_lstm_seq_bwd_f32 -> the fetched output buffers by name"""
    T, N, E = p["T"], p["N"], p["E"]
    ws = empty_bytes(lib.vc_lstm_seq_workspace_bytes(T, N, E, H))
    wsb = ws.numel() * 4
    tX, tW, tl, tact, tcs, ths = up(p["X"]), up(p["W"]), up(p["lens"]), up(p["act"]), up(p["cs"]), up(p["hs"])
    text = None if p["dhs_ext"] is None else up(p["dhs_ext"])
    out = dict(dG=Guarded((T, N, 4 * H)), dX=Guarded((T, N, E)), dH=Guarded((N, H), p["dH0"]), dC=Guarded((N, H), p["dC0"]),
               dW=Guarded((E + H, 4 * H)), db=Guarded((1, 4 * H)))
    o = out
    if fused:
        lib.vc_lstm_seq_bwd_f32(stream(), T, N, E, H, P(tX), P(tW), P(tl), P(tact), P(tcs), P(ths), P(text), o["dH"].ptr, o["dC"].ptr,
                                o["dG"].ptr, o["dX"].ptr, o["dW"].ptr, o["db"].ptr, P(ws), wsb, flags)
    else:
        lib.vc_lstm_seq_bwd_data_f32(stream(), T, N, E, H, P(tW), P(tl), P(tact), P(tcs), P(text), o["dH"].ptr, o["dC"].ptr, o["dG"].ptr,
                                     o["dX"].ptr, P(ws), wsb, flags)
        lib.vc_lstm_seq_bwd_weights_f32(stream(), T, N, E, H, P(tX), P(ths), o["dG"].ptr, o["dW"].ptr, o["db"].ptr, P(ws), wsb, flags)
    for g in out.values():
        g.fetch()
    return out


def check_bwd(p, out, tol, what):
    ref, lens, E = p["ref"], p["lens"], p["E"]
    W64 = p["cache"]["W"]
    for name, g in out.items():
        assert g.guards_intact(), "%s: rows outside %s were written" % (what, name)
    check(out["dG"].value, ref["dG"], tol, "%s dG" % what)
    check(out["dX"].value, ref["dG"] @ W64[:E].T, tol, "%s dX" % what)
    check(out["dH"].value, ref["dh1"], tol, "%s dH_run (d hs[1])" % what)
    check(out["dC"].value, ref["dc0"], tol, "%s dC_run (d cs[0])" % what)
    never = lens == 0
    assert (out["dG"].value[:, never] == 0).all(), "%s: dG of rows that never run must be exactly 0" % what
    assert np.array_equal(out["dC"].value[never], p["dC0"][never]), "%s: dC_run of rows that never run must be carried bit for bit" % what
    check(out["dW"].value, ref["dW"], tol, "%s dW" % what)
    check(out["db"].value[0], ref["db"], tol, "%s db" % what)


def bwd_case(lib, name, N, precision, with_ext=True):
    p = bwd_problem(N, with_ext=with_ext)
    what = "%s N=%d %s%s" % (name, N, precision, "" if with_ext else " no-ext")
    two = run_bwd(lib, p, FLAGS[precision], fused=False)
    check_bwd(p, two, TOL[precision][1], what)
    one = run_bwd(lib, p, FLAGS[precision], fused=True)
    for k in two:   # the fused entry is the two calls on one stream: any difference is a race or a read of unwritten memory
        assert np.array_equal(one[k].full, two[k].full), "%s: fused call differs from data + weights calls in %s" % (what, k)


BWD_PARAMS = [pytest.param(c, prec, id="%s-%s" % (c[0], prec)) for c in R.BWD_CASES for prec in ("f32", "bf16x3")]


@pytest.mark.parametrize("case,precision", BWD_PARAMS)
def test_seq_bwd_at_every_launch_boundary(lib, case, precision):
    """Every (CT, RT) variant of lstm_rec_bwd_kernel, f32 and split-bf16 (module docstring).  dG, dH_run and dC_run of the split-bf16
    kernels are held to the same 2e-4 as its dX."""
    name, n_of, want = case
    N = n_of(cus())
    reason = R.bwd_case_skip_reason(name, N, cus())
    if reason:
        pytest.skip(reason)
    path = R.bwd_path(N, cus())
    assert want(path), "case %s: N = %d lands on %s on %d CUs" % (name, N, path, cus())
    bwd_case(lib, name, N, precision)


def test_seq_bwd_without_external_gradients(lib):
    """dhs_ext = NULL (the encoder's call): ct1-rt5-49rows once more, f32"""
    name, n_of, want = next(c for c in R.BWD_CASES if c[0] == "ct1-rt5-49rows")
    N = n_of(cus())
    assert want(R.bwd_path(N, cus()))
    bwd_case(lib, name, N, "f32", with_ext=False)


# ----------------------------------------------------------------------------- forward, split-bf16
def run_fwd(lib, p, flags):
    T, N, E = p["T"], p["N"], p["E"]
    ws = empty_bytes(lib.vc_lstm_seq_workspace_bytes(T, N, E, H))
    state = lambda s0: np.concatenate([s0[None], np.full((T, N, H), SENTINEL, np.float32)])
    out = dict(act=Guarded((T, N, 4 * H)), cs=Guarded((T + 1, N, H), state(p["c0"])), hs=Guarded((T + 1, N, H), state(p["h0"])))
    lib.vc_lstm_seq_fwd_f32(stream(), T, N, E, H, P(up(p["X"])), P(up(p["W"])), P(up(p["b"])), P(up(p["lens"])), out["act"].ptr,
                            out["cs"].ptr, out["hs"].ptr, P(ws), ws.numel() * 4, flags)
    for g in out.values():
        g.fetch()
    return out


def check_fwd(p, out, tol, what):
    cache, lens = p["cache"], p["lens"]
    for name, g in out.items():
        assert g.guards_intact(), "%s: rows outside %s were written" % (what, name)
    hs, cs = out["hs"].value, out["cs"].value
    assert np.array_equal(hs[0], p["h0"]) and np.array_equal(cs[0], p["c0"]), "%s: the initial state was written" % what
    check(hs, cache["hs"], tol, "%s hs" % what)
    check(cs, cache["cs"], tol, "%s cs" % what)
    check(out["act"].value, cache["act"], tol, "%s gate activations" % what)
    for t in range(p["T"]):
        idle = lens <= t
        assert np.array_equal(hs[t + 1][idle], hs[t][idle]) and np.array_equal(cs[t + 1][idle], cs[t][idle]), \
            "%s: rows inactive at step %d must carry their state unchanged" % (what, t)


@pytest.mark.parametrize("case", R.FWD_BX_CASES, ids=[c[0] for c in R.FWD_BX_CASES])
def test_seq_fwd_bf16x3_at_every_launch_boundary(lib, case):
    """lstm_rec_fwd_kernel<3, true>, <5, true> and lstm_rec8_fwd_kernel<true>: two steps from a non-zero state"""
    name, n_of, want = case
    N = n_of(cus())
    path = R.fwd_path(N, cus())
    assert want(*path), "case %s: N = %d lands on %s on %d CUs" % (name, N, path, cus())
    p = R.make_fwd_problem(N, 2, 16, H, seed=5 * N + 2)
    if N > 3:
        assert (p["lens"] == 0).any() and (p["lens"] == 1).any()
    check_fwd(p, run_fwd(lib, p, FLAGS["bf16x3"]), TOL["bf16x3"][0], "fwd bf16x3 %s N=%d" % (path[0], N))
