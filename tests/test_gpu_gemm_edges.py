"""-m gpu: vc_gemm_f32 / vc_gemm_bf16x3_f32 (csrc/gemm.hip, gemm_core.h, gemm_bf16x3_core.h) at every plan, tile and alignment edge of their
dispatch, through the C ABI against a float64 product in numpy (tests/gemm_edges_ref.py).  No kernel of the library serves as a reference.

Rules of every run:
  * two kinds of input: "exact" (small integers; every partial sum is an integer below 2**24, asserted before the call, so the result must
    EQUAL the reference in BOTH precisions, however K is tiled, split or shifted) and "random" (standard normal: the project's
    2e-6 sqrt(K) + 2e-6 of the tensor maximum in f32; 6e-5 of the maximum and the element-wise 2**-16 |A| |B| + 1e-6 in split-bf16);
  * a case of the table runs in the four storage orders; its flags go round by case index and order, its bias comes and goes with them;
    the split-bf16 mode is entered through vc_gemm_bf16x3_f32 (ta = 0) and through VC_GEMM_BF16X3 on vc_gemm_f32 (ta = 1);
  * C enters as NaN (as C0 with VC_GEMM_ACCUMULATE) inside a sentinel frame, and the WHOLE buffer is compared: padding columns, the float in
    front (offset dress) and the guard band behind; the padding of A and B and what follows `bias` is NaN;
  * the workspace is exactly vc_gemm_workspace_bytes long, enters as NaN and is followed by a sentinel band that must come back intact;
  * the tile a case reaches is NOT observed here: tests/test_gemm_edges_host.py pins the planner transcription to the library's
    workspace query and asserts the plan of every row."""
import numpy as np
import pytest
import torch

from . import gemm_edges_ref as R
from .gpu_util import P, assert_close, dev, host, stream

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from vae_captioning_amd import abi
    return abi.load()


def launch(lib, case, kind, prec, ta, tb, flags, bias, dress="plain", null_operands=False):
    """one call; -> (device C buffer, geometry, device workspace, its length in floats)"""
    M, N, K = case
    A, B, b, C0 = R.inputs(case, kind)
    g = R.dress_geometry(dress, M, N, K, ta, tb)
    tA = dev(R.embed(R.stored(A, ta), g.lda, g.offset, R.NAN))
    tB = dev(R.embed(R.stored(B, tb), g.ldb, g.offset, R.NAN))
    tb_ = dev(R.embed(b, N, g.offset, R.NAN))
    tC = dev(R.embed(C0 if flags & R.ACCUMULATE else np.full((M, N), R.NAN, f32), g.ldc, g.offset, R.SENTINEL))
    nbytes = lib.vc_gemm_workspace_bytes(M, N, K)
    assert nbytes == R.expected_workspace_bytes(M, N, K) and nbytes % 4 == 0
    nws = nbytes // 4
    ws = dev(np.concatenate([np.full(nws, R.NAN, f32), np.full(R.GUARD, R.SENTINEL, f32)]))
    off = 4 * g.offset
    if prec == "bf16x3" and ta == 0:
        fn, fl = lib.vc_gemm_bf16x3_f32, flags
    else:
        fn, fl = lib.vc_gemm_f32, flags | (R.BF16X3 if prec == "bf16x3" else 0)
    pA, pB = (None, None) if null_operands else (P(tA) + off, P(tB) + off)
    fn(stream(), ta, tb, M, N, K, pA, g.lda, pB, g.ldb, P(tC) + off, g.ldc, P(tb_) + off if bias else None, fl, P(ws), nbytes)
    return tC, g, ws, nws


def check(tC, g, ws, nws, case, kind, prec, flags, bias, what):
    M, N, K = case
    ref = R.reference(case, kind, flags, bias)
    got = host(tC)
    hws = host(ws)
    assert np.array_equal(R.bits(hws[nws:]), R.bits(np.full(R.GUARD, R.SENTINEL, f32))), what + ": band behind the workspace overwritten"
    if kind == "exact":
        want = R.embed(ref.astype(f32), g.ldc, g.offset, R.SENTINEL)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(~(got == want))
            i = int(bad[0])
            raise AssertionError("%s: %d of %d floats of the C buffer differ, first at flat index %d (row %d, column %d): got %r, expected %r"
                                 % (what, bad.size, got.size, i, (i - g.offset) // g.ldc, (i - g.offset) % g.ldc, got[i], want[i]))
        return
    # random: the frame bit for bit, the logical part within the tolerances
    frame = got.copy()
    inner = frame[g.offset:g.offset + M * g.ldc].reshape(M, g.ldc)
    vals = inner[:, :N].copy()
    inner[:, :N] = 0
    assert np.array_equal(R.bits(frame), R.bits(R.embed(np.zeros((M, N), f32), g.ldc, g.offset, R.SENTINEL))), what + ": written outside C[:, :N]"
    if prec == "f32":
        assert_close(vals, ref, R.tol_f32(K), msg=what)
    else:
        assert_close(vals, ref, R.TOL_BF16X3, msg=what)
        err, bound = np.abs(vals - ref), R.bf16x3_bound(case, kind)
        assert (err <= bound).all(), "%s: element-wise model exceeded %.2f times" % (what, float((err / bound).max()))


def run(lib, case, kind, prec, ta, tb, flags, bias, dress="plain"):
    what = "%s %s %s ta=%d tb=%d flags=%d bias=%s %s" % (R.case_id(case), kind, prec, ta, tb, flags, "yes" if bias else "NULL", dress)
    if kind == "exact":
        assert R.is_exact(case), what
    tC, g, ws, nws = launch(lib, case, kind, prec, ta, tb, flags, bias, dress)
    check(tC, g, ws, nws, case, kind, prec, flags, bias, what)


# =================================================================== every case, four storage orders, two precisions, two kinds
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gemm_edge_case_in_four_storage_orders(lib, case, kind, prec):
    """the plan this row reaches in `prec` is R.CASE_PLANS[case][prec] (tests/test_gemm_edges_host.py)"""
    for ta, tb in R.ORDERS:
        run(lib, case, kind, prec, ta, tb, R.flags_of(case, ta, tb), R.with_bias(case, ta, tb))


# =================================================================== the other dresses on one split case per tile configuration
@pytest.mark.parametrize("dress", R.DRESSES[1:])
@pytest.mark.parametrize("prec,case", [(p, c) for p in R.PRECS for c in R.DRESS_CASES[p]], ids=lambda v: R.case_id(v) if isinstance(v, tuple) else v)
def test_gemm_operands_embedded_in_larger_buffers(lib, prec, case, dress):
    """padded: the vector paths with leading dimensions beyond the extents; odd: vector loaders, vector epilogue and the float4 reduce
    switched off by the leading dimensions; offset: by the alignment of A, B, C and bias alone.  Bias, ReLU and accumulate all on: the
    reduce kernels see the misaligned bias and C."""
    for ta, tb in R.ORDERS:
        run(lib, case, "exact", prec, ta, tb, R.RELU | R.ACCUMULATE, True, dress)


# =================================================================== determinism of the split paths
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case", R.DETERMINISM_CASES, ids=R.case_id)
def test_two_calls_on_the_same_inputs_are_bit_equal(lib, case, prec):
    """scalar reduce, float4 reduce, the tail launch's reduce: fixed summation order (include/vaecap.h: deterministic)"""
    first = launch(lib, case, "random", prec, 0, 0, R.RELU | R.ACCUMULATE, True)[0]
    second = launch(lib, case, "random", prec, 0, 0, R.RELU | R.ACCUMULATE, True)[0]
    torch.cuda.synchronize()
    assert first.data_ptr() != second.data_ptr() and torch.equal(first, second)
    assert not torch.isnan(first[:case[0] * case[1]]).any()


# =================================================================== K == 0: the zero product
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case", R.K0_CASES, ids=R.case_id)
def test_k_zero_is_the_zero_product(lib, case, prec):
    """include/vaecap.h: C = epilogue(0) -- bias or 0, + C with VC_GEMM_ACCUMULATE, ReLU'd with VC_GEMM_RELU -- in both precisions, on
    every tile configuration K == 0 can reach (64 x 64, 128 x 128, 256 x 256), with lda / ldb of 0 where K is the extent"""
    assert lib.vc_gemm_workspace_bytes(*case) == 0
    for flags in (0, R.RELU | R.ACCUMULATE):
        for bias in (True, False):
            for ta, tb in ((0, 0), (1, 1)):
                run(lib, case, "exact", prec, ta, tb, flags, bias)


def test_k_zero_reads_neither_operand(lib):
    case = R.K0_CASES[0]
    for prec in R.PRECS:
        for ta in (0, 1):
            what = "%s %s NULL operands" % (R.case_id(case), prec)
            tC, g, ws, nws = launch(lib, case, "exact", prec, ta, 0, R.ACCUMULATE, True, null_operands=True)
            check(tC, g, ws, nws, case, "exact", prec, R.ACCUMULATE, True, what)
