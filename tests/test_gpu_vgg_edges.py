"""-m gpu: the kernels the other VGG tests use as their reference -- the implicit-GEMM convolution of csrc/conv.hip (weight gradient
with split-K in every tile configuration, degenerate image sizes, the K-split tail of the data gradient), conv1_1's own kernels
(csrc/conv_first.hip) and the pooling / layout / preprocessing kernels past one sweep of their capped grid -- through the C ABI against
oracle/vgg.py in float64 and numpy (tests/vgg_edges_ref.py).  No kernel of the library serves as a reference here.

Rules of every case:
  * convolutions run on two kinds of input: "exact" (small integers: every partial sum is an integer below 2**24, asserted before the
    call, so the result must EQUAL the oracle's whatever the summation order) and "random" (standard normal, the project's rounding
    tolerances R.tol_conv / R.tol_conv1 of max|ref|);
  * outputs and workspaces enter filled with NaN: an element left unwritten fails the case (a `db` not asked for must stay NaN);
  * every output and workspace is followed by GUARD sentinel floats that must come back unchanged, and a workspace has exactly the size
    its vc_*_workspace_bytes query returns; inputs are followed by NaN;
  * a case chosen for a split count, a partial count or a grid wrap asserts that it still reaches it."""
import numpy as np
import pytest
import torch

from vae_captioning_amd.abi import VaecapError

from . import vgg_edges_ref as R
from .gpu_util import P, assert_close, dev, from_c4, host, stream, to_c4

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64
SENTINEL = f32(-24680.5)
NAN = f32(np.nan)
GRID_CAP_ITEMS = R.GRID_CAP_ITEMS   # csrc/conv.hip grid_for: 4096 blocks x 256 threads, one item per thread and sweep


@pytest.fixture(scope="module")
def lib():
    from vae_captioning_amd import abi
    return abi.load()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def guarded(a):
    """upload `a` (flattened) followed by GUARD sentinel floats"""
    a = np.ascontiguousarray(a, f32).ravel()
    return dev(np.concatenate([a, np.full(GUARD, SENTINEL, f32)]))


def poisoned(n):
    return guarded(np.full(int(n), NAN, f32))


def padded_in(a):
    """an INPUT: `a` (flattened) followed by GUARD NaN -- a read past the logical end poisons the result"""
    a = np.ascontiguousarray(a, f32).ravel()
    return dev(np.concatenate([a, np.full(GUARD, NAN, f32)]))


def raw(t, n, what):
    """host copy of the logical part after checking the guard band (NaN allowed: for buffers that must be UNCHANGED, and workspaces)"""
    h = host(t).ravel()
    assert h.size == n + GUARD, what
    assert np.array_equal(bits(h[n:]), bits(np.full(GUARD, SENTINEL, f32))), "%s: guard band overwritten" % what
    return h[:n]


def logical(t, n, what):
    out = raw(t, n, what)
    assert not np.isnan(out).any(), "%s: %d of %d elements unwritten or NaN" % (what, int(np.isnan(out).sum()), n)
    return out


def untouched(t, n, what):
    assert np.isnan(raw(t, n, what)).all(), "%s: written although not asked for" % what


def compare(got, ref, kind, tol, what):
    """exact inputs: equality with the float64 oracle; random inputs: max error <= tol * max|ref|"""
    got = np.asarray(got).reshape(np.shape(ref))
    if kind == "exact":
        np.testing.assert_array_equal(got, ref, err_msg=what)
    else:
        assert_close(got, ref, tol, msg=what)


def workspace(nbytes):
    assert nbytes % 4 == 0
    return poisoned(nbytes // 4), nbytes // 4


# =================================================================== A / B. implicit-GEMM weight gradient (vc_conv3x3_wgrad_f32)
def run_wgrad(lib, case, kind, splits):
    """db given / accumulate = 0, accumulate = 1 into non-zero dw / db, db = NULL"""
    B, H, W, Ci, Co = case
    what = "wgrad %s %s" % (R.case_id(case), kind)
    x, w, b, dy, dw0, db0 = R.conv_inputs(case, kind)
    _, dwref, dbref = R.conv_bwd_ref(case, kind, False)
    npix, MN = B * H * W, 9 * Ci * Co
    nbytes = lib.vc_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Co)
    assert nbytes % (4 * (MN + Co)) == 0 and nbytes // (4 * (MN + Co)) == splits, \
        "%s: plan_wgrad now gives %d splits, not %d: choose a shape that reaches this edge again" % (what, nbytes // (4 * (MN + Co)), splits)
    if kind == "exact":
        assert R.is_exact(npix, x, dy, dw0) and R.is_exact(npix, np.ones(1), dy, db0), what
    tol = R.tol_conv(npix)
    tx, tdy = padded_in(x), padded_in(dy)
    call = lambda dw, db, acc, ws: lib.vc_conv3x3_wgrad_f32(stream(), B, H, W, Ci, Co, P(tx), P(tdy), P(dw), db, acc, P(ws), nbytes)
    # ---- db given, accumulate = 0
    (ws, nws), dw, db = workspace(nbytes), poisoned(MN), poisoned(Co)
    call(dw, P(db), 0, ws)
    compare(logical(dw, MN, what), dwref, kind, tol, what + " dw")
    compare(logical(db, Co, what), dbref, kind, tol, what + " db")
    part = raw(ws, nws, what + " workspace")
    assert not np.isnan(part).any(), what + ": a split left part of its partial sums unwritten"
    # ---- accumulate = 1 into non-zero dw / db
    (ws, nws), dw, db = workspace(nbytes), guarded(dw0), guarded(db0)
    call(dw, P(db), 1, ws)
    compare(logical(dw, MN, what), dw0.astype(np.float64) + dwref, kind, tol, what + " dw, accumulate")
    compare(logical(db, Co, what), db0.astype(np.float64) + dbref, kind, tol, what + " db, accumulate")
    raw(ws, nws, what + " workspace")
    # ---- db = NULL: no bias gradient, no bias partials
    (ws, nws), dw, db = workspace(nbytes), poisoned(MN), poisoned(Co)
    call(dw, None, 0, ws)
    compare(logical(dw, MN, what), dwref, kind, tol, what + " dw, db = NULL")
    untouched(db, Co, what + " db")
    part = raw(ws, nws, what + " workspace")
    assert not np.isnan(part[:splits * MN]).any() and np.isnan(part[splits * MN:]).all(), what + ": bias partials without db"


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case,cfg,splits", R.WGRAD_CASES, ids=[R.case_id(c) for c, _, _ in R.WGRAD_CASES])
def test_conv_wgrad_split_k_in_every_tile_configuration(lib, case, cfg, splits, kind):
    run_wgrad(lib, case, kind, splits)


# =================================================================== B. degenerate geometry
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.GEOM_CASES, ids=R.case_id)
def test_conv_degenerate_geometry(lib, case, kind):
    """image sides 1 and 2 (SAME padding on both sides of every pixel), W = 1 with a prime H (the reciprocal pixel decode of the weight
    gradient's loader)"""
    B, H, W, Ci, Co = case
    what = "%s %s" % (R.case_id(case), kind)
    x, w, b, dy, _, _ = R.conv_inputs(case, kind)
    yb, y0 = R.conv_fwd_ref(case, kind)
    dxref, _, _ = R.conv_bwd_ref(case, kind, True)
    if kind == "exact":
        assert R.is_exact(9 * Ci, x, w, b) and R.is_exact(9 * Co, dy, w), what
    npix = B * H * W
    tx, tw, tb, tdy = padded_in(x), padded_in(w), padded_in(b), padded_in(dy)
    for relu in (0, 1):
        for bias, ref in ((P(tb), yb), (None, y0)):
            y = poisoned(npix * Co)
            lib.vc_conv3x3_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(tw), bias, P(y), relu, None, 0)
            msg = "%s fwd relu=%d bias=%s" % (what, relu, "yes" if bias else "NULL")
            compare(logical(y, npix * Co, msg), np.maximum(ref, 0) if relu else ref, kind, R.tol_conv(9 * Ci), msg)
    for src, ref in ((P(tx), dxref * (x > 0)), (None, dxref)):
        dx = poisoned(npix * Ci)
        lib.vc_conv3x3_dgrad_f32(stream(), B, H, W, Ci, Co, P(tdy), P(tw), src, P(dx), None, 0)
        msg = "%s dgrad relu_src=%s" % (what, "x" if src else "NULL")
        compare(logical(dx, npix * Ci, msg), ref, kind, R.tol_conv(9 * Co), msg)
    run_wgrad(lib, case, kind, R.GEOM_SPLITS.get(case, 1))


@pytest.mark.parametrize("kind", R.KINDS)
def test_conv_dgrad_tail_split_against_the_oracle(lib, kind):
    """the data gradient with its workspace: main launch + K-split tail + conv_tail_reduce_kernel, against the oracle and not only
    against the single launch"""
    case = R.DGRAD_WS_CASE
    B, H, W, Ci, Co = case
    what = "dgrad tail %s %s" % (R.case_id(case), kind)
    x, w, _, dy, _, _ = R.conv_inputs(case, kind)
    dxref, _, _ = R.conv_bwd_ref(case, kind, True)
    if kind == "exact":
        assert R.is_exact(9 * Co, dy, w), what
    nbytes = lib.vc_conv3x3_dgrad_workspace_bytes(B, H, W, Ci, Co)
    assert nbytes > 0, "this shape must trigger the tail split"
    n = B * H * W * Ci
    tx, tw, tdy = padded_in(x), padded_in(w), padded_in(dy)
    for src, ref in ((P(tx), dxref * (x > 0)), (None, dxref)):
        (ws, nws), dx = workspace(nbytes), poisoned(n)
        lib.vc_conv3x3_dgrad_f32(stream(), B, H, W, Ci, Co, P(tdy), P(tw), src, P(dx), P(ws), nbytes)
        msg = "%s relu_src=%s" % (what, "x" if src else "NULL")
        compare(logical(dx, n, msg), ref, kind, R.tol_conv(9 * Co), msg)
        assert not np.isnan(raw(ws, nws, msg + " workspace")).all(), msg + ": the workspace was not used"


# =================================================================== C. conv1_1 (csrc/conv_first.hip)
def conv1_forward(lib, shape, kind, nan_channel=False):
    B, H, W = shape
    what = "conv1 fwd %s %s%s" % (R.case_id(shape), kind, " x4[..., 3] = NaN" if nan_channel else "")
    x4, w, b, _, _, _ = R.conv1_inputs(shape, kind)
    pre = R.conv1_fwd_ref(shape, kind)
    if kind == "exact":
        assert R.is_exact(27, x4, w, b), what
    assert lib.vc_conv1_supported(B, H, W) == 1
    if nan_channel:
        x4 = x4.copy()
        x4[..., 3] = NAN
    n = B * H * W * 64
    tx, tw, tb = padded_in(x4), padded_in(w), padded_in(b)
    for relu in (0, 1):
        y = poisoned(n)
        lib.vc_conv1_fwd_f32(stream(), B, H, W, P(tx), P(tw), P(tb), P(y), relu)
        msg = "%s relu=%d" % (what, relu)
        got = from_c4(logical(y, n, msg), (B, H, W, 64))
        compare(got, np.maximum(pre, 0) if relu else pre, kind, R.tol_conv1(27), msg)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape,groups", R.CONV1_FWD_CASES, ids=[R.case_id(s) for s, _ in R.CONV1_FWD_CASES])
def test_conv1_forward_against_the_oracle(lib, shape, groups, kind):
    assert shape[0] * shape[1] * shape[2] // 32 == groups
    conv1_forward(lib, shape, kind)


def conv1_wgrad(lib, shape, kind, nan_channel=False):
    B, H, W = shape
    what = "conv1 wgrad %s %s%s" % (R.case_id(shape), kind, " x4[..., 3] = NaN" if nan_channel else "")
    x4, _, _, dy, dw0, db0 = R.conv1_inputs(shape, kind)
    dwref, dbref = R.conv1_wgrad_ref(shape, kind)
    npix = B * H * W
    if kind == "exact":
        assert R.is_exact(npix, x4, dy, dw0) and R.is_exact(npix, np.ones(1), dy, db0), what
    if nan_channel:
        x4 = x4.copy()
        x4[..., 3] = NAN
    nbytes = lib.vc_conv1_wgrad_workspace_bytes()
    tol = R.tol_conv1(npix)
    tx, tdy = padded_in(x4), padded_in(to_c4(dy))
    for acc in (0, 1):
        for with_db in (True, False):
            ws, nws = workspace(nbytes)
            dw = guarded(dw0) if acc else poisoned(27 * 64)
            db = guarded(db0) if acc and with_db else poisoned(64)
            lib.vc_conv1_wgrad_f32(stream(), B, H, W, P(tx), P(tdy), P(dw), P(db) if with_db else None, acc, P(ws), nbytes)
            msg = "%s accumulate=%d db=%s" % (what, acc, "yes" if with_db else "NULL")
            compare(logical(dw, 27 * 64, msg), dwref + (dw0.astype(np.float64) if acc else 0), kind, tol, msg + " dw")
            if with_db:
                compare(logical(db, 64, msg), dbref + (db0.astype(np.float64) if acc else 0), kind, tol, msg + " db")
            else:
                untouched(db, 64, msg + " db")
            raw(ws, nws, msg + " workspace")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape,parts", R.CONV1_WGRAD_CASES, ids=[R.case_id(s) for s, _ in R.CONV1_WGRAD_CASES])
def test_conv1_wgrad_against_the_oracle(lib, shape, parts, kind):
    assert min(-(-(shape[0] * shape[1] * shape[2] // 32) // 4), 1024) == parts
    conv1_wgrad(lib, shape, kind)


@pytest.mark.parametrize("kind", R.KINDS)
def test_conv1_ignores_the_fourth_input_channel(lib, kind):
    """include/vaecap.h: "x4: [B,H,W,4] ... (fourth channel ignored)" -- NaN there must change nothing"""
    conv1_forward(lib, R.CONV1_FWD_NAN_CASE, kind, nan_channel=True)
    conv1_wgrad(lib, R.CONV1_WGRAD_NAN_CASE, kind, nan_channel=True)


def test_conv1_refusals_come_before_any_launch(lib):
    B, H = 1, 4
    nbytes = lib.vc_conv1_wgrad_workspace_bytes()
    ws, nws = workspace(nbytes)
    w, b = dev(np.ones((3, 3, 3, 64), f32)), dev(np.ones(64, f32))
    # ---- W % 32 != 0
    W = 48
    assert lib.vc_conv1_supported(B, H, W) == 0
    x4, dyc = dev(np.ones((B, H, W, 4), f32)), dev(np.ones((B, 16, H, W, 4), f32))
    y, dw, db = poisoned(B * H * W * 64), poisoned(27 * 64), poisoned(64)
    with pytest.raises(VaecapError):
        lib.vc_conv1_fwd_f32(stream(), B, H, W, P(x4), P(w), P(b), P(y), 1)
    with pytest.raises(VaecapError):
        lib.vc_conv1_wgrad_f32(stream(), B, H, W, P(x4), P(dyc), P(dw), P(db), 0, P(ws), nbytes)
    untouched(y, B * H * W * 64, "y, W = 48")
    # ---- a workspace one float short
    W = 64
    assert lib.vc_conv1_supported(B, H, W) == 1
    x4 = dev(np.ones((B, H, W + 1, 4), f32))            # (room for the offset pointer below)
    dyc = dev(np.ones((B, 16, H, W, 4), f32))
    with pytest.raises(VaecapError):
        lib.vc_conv1_wgrad_f32(stream(), B, H, W, P(x4), P(dyc), P(dw), P(db), 0, P(ws), nbytes - 4)
    with pytest.raises(VaecapError):
        lib.vc_conv1_wgrad_f32(stream(), B, H, W, P(x4), P(dyc), P(dw), P(db), 0, None, nbytes)
    # ---- x4 four bytes off a 16-byte boundary: the forward loads 16-byte pixels
    y = poisoned(B * H * W * 64)
    with pytest.raises(VaecapError):
        lib.vc_conv1_fwd_f32(stream(), B, H, W, P(x4) + 4, P(w), P(b), P(y), 1)
    untouched(y, B * H * W * 64, "y, x4 misaligned")
    untouched(dw, 27 * 64, "dw")
    untouched(db, 64, "db")
    untouched(ws, nws, "workspace")


# =================================================================== D. pooling, layout, preprocessing: small edges and the grid wrap
def wraps(items):
    assert items > GRID_CAP_ITEMS, "%d items no longer exceed one sweep of the capped grid" % items


@pytest.mark.parametrize("shape", R.POOL_SMALL + [R.POOL_WRAP], ids=R.case_id)
def test_maxpool_forward_and_backward(lib, shape):
    B, H, W, C = shape
    if shape == R.POOL_WRAP:
        wraps(B * (H // 2) * (W // 2) * (C // 4))
    x, dy = R.pool_inputs(shape)
    yref, arg, dxref, dxrelu = R.pool_ref(shape)
    assert (yref < 0).any() or shape[1:3] == (2, 2)
    tx, tdy = padded_in(x), padded_in(dy)
    y = poisoned(yref.size)
    lib.vc_maxpool2x2_fwd_f32(stream(), B, H, W, C, P(tx), P(y))
    np.testing.assert_array_equal(logical(y, yref.size, "maxpool fwd").reshape(yref.shape), yref)
    for relu_grad, ref in ((0, dxref), (1, dxrelu)):
        dx = poisoned(x.size)
        lib.vc_maxpool2x2_bwd_f32(stream(), B, H, W, C, P(tx), P(tdy), P(dx), relu_grad)
        np.testing.assert_array_equal(logical(dx, x.size, "maxpool bwd").reshape(x.shape), ref, err_msg="relu_grad=%d" % relu_grad)


@pytest.mark.parametrize("shape", R.POOL_SMALL + [R.POOL_WRAP], ids=R.case_id)
def test_maxpool_backward_from_host_built_routing_codes(lib, shape):
    B, H, W, C = shape
    if shape == R.POOL_WRAP:
        wraps(B * (C // 4) * (H // 2) * (W // 2))
    x, dy = R.pool_inputs(shape)
    yref, arg, _, dxrelu = R.pool_ref(shape)
    words = R.pool_codes_words(R.pool_codes(arg, yref))
    assert words.size >= lib.vc_conv3x3_wino_pool_words(B, H, W, C)
    tbits = dev(words.view(np.int32))
    tdy = padded_in(to_c4(dy))
    dx = poisoned(x.size)
    lib.vc_maxpool2x2_bwd_bits_f32(stream(), B, H, W, C, P(tbits), P(tdy), P(dx))
    np.testing.assert_array_equal(from_c4(logical(dx, x.size, "maxpool bwd bits"), shape), dxrelu)


@pytest.mark.parametrize("shape", R.LAYOUT_SMALL + [R.LAYOUT_WRAP], ids=R.case_id)
def test_nhwc_to_c4_and_back(lib, shape):
    B, H, W, C = shape
    if shape == R.LAYOUT_WRAP:
        wraps(B * H * W * (C // 4))
    n = B * H * W * C
    a = np.arange(n, dtype=f32).reshape(shape)       # every element distinct (n < 2**24)
    assert n < 2 ** 24
    ta, c4, back = padded_in(a), poisoned(n), poisoned(n)
    lib.vc_nhwc_to_c4_f32(stream(), B, H, W, C, P(ta), P(c4))
    np.testing.assert_array_equal(logical(c4, n, "nhwc -> c4"), R.to_c4(a).ravel())
    lib.vc_c4_to_nhwc_f32(stream(), B, H, W, C, P(c4), P(back))
    np.testing.assert_array_equal(logical(back, n, "c4 -> nhwc"), a.ravel())


@pytest.mark.parametrize("shape", R.PREPROCESS_F32, ids=R.case_id)
def test_preprocess_f32(lib, shape):
    B, H, W = shape
    if shape == R.PREPROCESS_F32[0]:
        wraps(B * H * W)
    img = np.random.default_rng(B * H * W).integers(0, 256, size=(B, H, W, 3)).astype(f32)
    out = poisoned(B * H * W * 4)
    lib.vc_vgg_preprocess_f32(stream(), P(padded_in(img)), B, H, W, P(out))
    np.testing.assert_array_equal(logical(out, B * H * W * 4, "preprocess f32"), R.preprocess_ref(img).ravel())


@pytest.mark.parametrize("shape", R.PREPROCESS_U8, ids=R.case_id)
def test_preprocess_u8(lib, shape):
    B, H, W = shape
    if shape == R.PREPROCESS_U8[0]:
        wraps(B * H * W // 4)
    img = np.random.default_rng(B * H * W + 1).integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    out = poisoned(B * H * W * 4)
    lib.vc_vgg_preprocess_u8(stream(), P(dev(img)), B, H, W, P(out))
    np.testing.assert_array_equal(logical(out, B * H * W * 4, "preprocess u8"), R.preprocess_ref(img).ravel())


@pytest.mark.parametrize("case", R.PAD_DIM, ids=R.case_id)
def test_pad_dim(lib, case):
    outer, c_src, c_dst, inner = case
    if case in R.PAD_DIM[:2]:
        wraps(outer * c_dst * inner)
    n = outer * c_dst * inner
    src = np.arange(1, outer * c_src * inner + 1, dtype=f32).reshape(outer, c_src, inner)   # distinct, non-zero
    dst = poisoned(n)
    lib.vc_pad_dim_f32(stream(), P(padded_in(src)), outer, c_src, c_dst, inner, P(dst))
    np.testing.assert_array_equal(logical(dst, n, "pad_dim"), R.pad_dim_ref(src, c_dst).ravel())
