"""-m gpu: the Winograd kernels every VGG16 layer behind conv1_1 runs -- F(2x2,3x3) forward / data gradient (csrc/conv_wino.hip), F(4x4,3x3)
forward / data gradient, fused and with the pre-transformed input (csrc/conv_wino4.hip), F(3x3,2x2) weight gradient
(csrc/conv_wino_wgrad*.hip) -- at the edges of their host-side plans: every tile-block shape and LDS pitch plan_wino2 can choose, blocks
ragged in x, in y and in both, a last workgroup of empty blocks, odd and tiny images, the workgroup order past one chunk of channel
tiles, K splits of several blocks with a short last one.  Through the C ABI against oracle/vgg.py in float64 (tests/wino_edges_ref.py);
a library kernel serves as a reference only where two entries must agree BIT FOR BIT (mask bits against the float mask, the
pre-transformed form against the fused one, db == NULL against db given, y == NULL against y given).

Rules of every case (those of tests/test_gpu_vgg_edges.py):
  * outputs, mask and routing-code buffers and workspaces enter as NaN (integer buffers: all-ones words) and are followed by GUARD
    sentinel elements that must come back bit-unchanged; an element left unwritten fails the case;
  * a workspace has exactly the size its query returns; inputs are followed by NaN;
  * before launching, a case asserts that the library agrees with the plan restated in tests/wino_edges_ref.py, through the buffer-size
    and *_supported queries the ABI exports: a case chosen for an edge fails when the plan moves, it does not test something else;
  * "exact" inputs (F(2x2,3x3), weight gradient): the result must EQUAL the oracle's; "random": the project's tolerances of max|ref|."""
import functools

import numpy as np
import pytest

from vae_captioning_amd.abi import VaecapError

from . import wino_edges_ref as R
from .gpu_util import P, assert_close, dev, from_c4, host, stream, to_c4

pytestmark = pytest.mark.gpu

f32 = np.float32
compare = functools.partial(R.compare, close=assert_close)


@pytest.fixture(scope="module")
def lib():
    from vae_captioning_amd import abi
    return abi.load()


# ---- device buffers (uint32 words travel as int32)
def poisoned(n):
    return dev(R.poison(n))


def words(n):
    return dev(R.poison(n, np.uint32).view(np.int32))


def guarded(a):
    return dev(R.with_guard(np.ascontiguousarray(a, f32)))


def padded_in(a):
    return dev(R.with_nan_tail(a))


def down(t):
    h = host(t)
    return h.view(np.uint32) if h.dtype == np.int32 else h


def raw(t, n, what):
    return R.raw(down(t), n, what)


def logical(t, n, what):
    return R.logical(down(t), n, what)


def untouched(t, n, what):
    R.untouched(down(t), n, what)


def same_bits(a, b, what):
    assert np.array_equal(R.bits(a), R.bits(b)), "%s: not bit-identical (%d of %d elements differ)" % (what, int((R.bits(a) != R.bits(b)).sum()), a.size)


def nhwc(flat, shape):
    return from_c4(flat, shape)


def pack(lib, fn, npos, tw, Cin, Cout, transpose):
    """packed transformed weights, poisoned and guarded like every other output"""
    n = npos * Cin * Cout
    wp = poisoned(n)
    getattr(lib, fn)(stream(), Cin, Cout, P(tw), transpose, P(wp))
    logical(wp, n, "%s transpose=%d" % (fn, transpose))
    return wp


# =================================================================== F(2x2,3x3) forward / data gradient (csrc/conv_wino.hip)
def w2_plan_agrees(lib, case, g):
    B, H, W, Ci, Co = case
    assert lib.vc_conv3x3_wino_supported(B, H, W, Ci, Co, 0) == 1
    assert lib.vc_conv3x3_wino_supported(B, H, W, Ci, Co, 1) == (1 if R.plan_wino2(B, H, W, Co, Ci) else 0)
    per = (Co // 32) * 256
    # B = 4: cdiv(4 blocks_img, 4) workgroups = blocks_img; B = 5: the round-up to four blocks per workgroup
    assert lib.vc_conv3x3_wino_mask_words(4, H, W, Co) == g["blocks_img"] * per, "plan_wino2 no longer cuts %dx%d into %d blocks" % (H, W, g["blocks_img"])
    assert lib.vc_conv3x3_wino_mask_words(5, H, W, Co) == R.cdiv(5 * g["blocks_img"], 4) * per
    assert lib.vc_conv3x3_wino_mask_words(B, H, W, Co) == R.wino_mask_words(B, H, W, Co)
    assert lib.vc_conv3x3_wino_pool_words(B, H, W, Co) == R.wino_pool_words(B, H, W, Co)


def run_w2(lib, case, kind):
    B, H, W, Ci, Co = case
    what = "wino2 %s %s" % (R.case_id(case), kind)
    g = R.plan_wino2(*case)
    w2_plan_agrees(lib, case, g)
    d, r = R.conv_inputs(case, kind), R.conv_ref(case, kind)
    if kind == "exact":
        assert R.exact_bound_fwd(Ci, d["x"], d["w"], d["b"]) < R.EXACT_LIMIT and R.exact_bound_fwd(Co, d["dy"], d["w"]) < R.EXACT_LIMIT, what
        assert R.exact_bound_fwd(Ci, d["dy2"], d["w2"]) < R.EXACT_LIMIT and R.weights_transform_to_integers(d["w"]), what
    tol, told = R.tol_wino2(9 * Ci), R.tol_wino2(9 * Co)
    ys, ps, xs = (B, H, W, Co), (B, H // 2, W // 2, Co), (B, H, W, Ci)
    ny, npl, nx = int(np.prod(ys)), int(np.prod(ps)), int(np.prod(xs))
    act = np.maximum(r["pre"], 0)
    scale = np.abs(act).max()
    tx, tw, tb = padded_in(to_c4(d["x"])), padded_in(d["w"]), padded_in(d["b"])
    wp = pack(lib, "vc_conv3x3_wino_pack_f32", 16, tw, Ci, Co, 0)
    # ---- forward with bias and ReLU, without either
    for bias, relu, ref in ((P(tb), 1, act), (None, 0, r["pre0"])):
        y = poisoned(ny)
        lib.vc_conv3x3_wino_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), bias, P(y), None, relu)
        msg = "%s fwd bias=%s relu=%d" % (what, "yes" if bias else "NULL", relu)
        compare(nhwc(logical(y, ny, msg), ys), ref, kind, tol, msg)
    # ---- forward with the fused pool
    ypool_ref, _ = R.pool_ref(r["pre"], d["dyp"])
    y, yp = poisoned(ny), poisoned(npl)
    lib.vc_conv3x3_wino_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), P(yp), 1)
    msg = what + " fwd + pool"
    compare(nhwc(logical(y, ny, msg), ys), act, kind, tol, msg + ": y")
    compare(nhwc(logical(yp, npl, msg), ps), ypool_ref, kind, tol, msg + ": ypool", scale=scale)
    # ---- pooled forward with routing codes; the codes routed by vc_maxpool2x2_bwd_bits_f32 against the oracle's MaxPoolGrad
    nw = R.wino_pool_words(B, H, W, Co)
    y, yp, codes = poisoned(ny), poisoned(npl), words(nw)
    lib.vc_conv3x3_wino_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), P(yp), P(codes))
    msg = what + " fwd_pool"
    compare(nhwc(logical(y, ny, msg), ys), act, kind, tol, msg + ": y")
    compare(nhwc(logical(yp, npl, msg), ps), ypool_ref, kind, tol, msg + ": ypool", scale=scale)
    raw(codes, nw, msg + ": codes")
    dxp = poisoned(ny)
    lib.vc_maxpool2x2_bwd_bits_f32(stream(), B, H, W, Co, P(codes), P(padded_in(to_c4(d["dyp"]))), P(dxp))
    R.compare_routing(nhwc(logical(dxp, ny, msg + ": routed"), ys), r["pre"], d["dyp"], 0.0 if kind == "exact" else tol * scale, msg + ": routed")
    # ---- forward leaving the ReLU mask as bits -> the NEXT layer's data gradient (Cout -> Cin) reading them: bit-identical to the one that
    # loads the float activation, and (the mask being this y, itself held to the oracle) equal to the oracle's data gradient under that mask
    nm = R.wino_mask_words(B, H, W, Co)
    y, mask = poisoned(ny), words(nm)
    lib.vc_conv3x3_wino_fwd_mask_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), 1, P(mask))
    msg = what + " fwd_mask"
    hy = nhwc(logical(y, ny, msg), ys)
    compare(hy, act, kind, tol, msg)
    raw(mask, nm, msg + ": mask")
    wpt2 = pack(lib, "vc_conv3x3_wino_pack_f32", 16, padded_in(d["w2"]), Co, Ci, 1)
    tdy2 = padded_in(to_c4(d["dy2"]))
    dxa, dxb = poisoned(ny), poisoned(ny)
    lib.vc_conv3x3_wino_dgrad_f32(stream(), B, H, W, Co, Ci, P(tdy2), P(wpt2), P(y), P(dxa))
    lib.vc_conv3x3_wino_dgrad_bits_f32(stream(), B, H, W, Co, Ci, P(tdy2), P(wpt2), P(mask), P(dxb))
    msg = what + " dgrad_bits of the next layer"
    ha, hb = logical(dxa, ny, msg + " (float mask)"), logical(dxb, ny, msg)
    same_bits(ha, hb, msg)
    compare(nhwc(hb, ys), r["dx2"] * (hy > 0), kind, R.tol_wino2(9 * Ci), msg)
    # ---- data gradient with and without relu_src
    if R.plan_wino2(B, H, W, Co, Ci) is None:
        return
    wpt = pack(lib, "vc_conv3x3_wino_pack_f32", 16, tw, Ci, Co, 1)
    tdy = padded_in(to_c4(d["dy"]))
    for src, ref in ((P(tx), r["dx"] * (d["x"] > 0)), (None, r["dx"])):
        dx = poisoned(nx)
        lib.vc_conv3x3_wino_dgrad_f32(stream(), B, H, W, Ci, Co, P(tdy), P(wpt), src, P(dx))
        msg = "%s dgrad relu_src=%s" % (what, "x" if src else "NULL")
        compare(nhwc(logical(dx, nx, msg), xs), ref, kind, told, msg)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case,shape", [(c, s) for c, s, _ in R.W2_SHAPE_CASES], ids=[i for _, _, i in R.W2_SHAPE_CASES])
def test_wino2_every_block_shape_and_pitch(lib, case, shape, kind):
    """one image = one block of the shape: patch size, pitch, magic divisors and dead lanes (lj >= TBH * TBW) of every shape the plan can
    choose; five images: the second workgroup holds one block and three empty ones"""
    g = R.plan_wino2(*case)
    assert (g["TBH"], g["TBW"], g["P"]) == shape and g["nblocks"] == 5
    run_w2(lib, case, kind)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case,directions", [(c, d) for c, d, _, _ in R.W2_RAGGED_CASES], ids=[i for _, _, _, i in R.W2_RAGGED_CASES])
def test_wino2_ragged_blocks(lib, case, directions, kind):
    assert R.ragged(R.plan_wino2(*case)) == directions
    run_w2(lib, case, kind)


def test_wino2_longest_reduction(lib):
    assert R.plan_wino2(*R.W2_LONG_CASE)["chunks"] == 32
    run_w2(lib, R.W2_LONG_CASE, "random")


@pytest.mark.parametrize("case", R.W2_REFUSED, ids=R.case_id)
def test_wino2_refusals_write_nothing(lib, case):
    """images no block fits (a 24 x 2 strip: every shape's halo patch exceeds 100 pixels) and odd sizes: refused by the query and the call"""
    B, H, W, Ci, Co = case
    assert R.plan_wino2(*case) is None
    assert lib.vc_conv3x3_wino_supported(B, H, W, Ci, Co, 0) == 0 and lib.vc_conv3x3_wino_supported(B, H, W, Ci, Co, 1) == 0
    assert lib.vc_conv3x3_wino_mask_words(B, H, W, Co) == 0
    n = B * H * W * Co
    x, wp = padded_in(np.ones(B * H * W * Ci, f32)), padded_in(np.ones(16 * Ci * Co, f32))
    y, yp, mask = poisoned(n), poisoned(n), words(256)
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino_fwd_f32(stream(), B, H, W, Ci, Co, P(x), P(wp), None, P(y), None, 0)
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(x), P(wp), None, P(y), P(yp), P(mask))
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino_fwd_mask_f32(stream(), B, H, W, Ci, Co, P(x), P(wp), None, P(y), 1, P(mask))
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino_dgrad_f32(stream(), B, H, W, Ci, Co, P(x), P(wp), None, P(y))
    with pytest.raises(VaecapError):
        lib.vc_conv3x3_wino_dgrad_bits_f32(stream(), B, H, W, Ci, Co, P(x), P(wp), P(mask), P(y))
    untouched(y, n, "y")
    untouched(yp, n, "ypool")
    untouched(mask, 256, "mask / codes")


# =================================================================== F(4x4,3x3) forward / data gradient (csrc/conv_wino4.hip), random kind
PACK4 = "vc_conv3x3_wino4_pack_f32"


def vspace(lib, B, H, W, C):
    """the pre-transformed input's workspace: NaN, exactly the queried size, guarded"""
    nbytes = lib.vc_conv3x3_wino4v_workspace_bytes(B, H, W, C)
    assert nbytes == R.wino4v_workspace_bytes(B, H, W, C) and nbytes > 0 and nbytes % 4 == 0
    return poisoned(nbytes // 4), nbytes


def run_w4_forward(lib, case):
    B, H, W, Ci, Co = case
    what = "wino4 %s" % R.case_id(case)
    g, v = R.plan_wino4(*case), R.plan_wino4v(*case)
    assert lib.vc_conv3x3_wino4_supported(B, H, W, Ci, Co, 0) == 1
    assert lib.vc_conv3x3_wino4_mask_words(B, H, W, Co) == R.cdiv(g["square_blocks"], 2) * (Co // 32) * 512, what + ": square blocks"
    assert lib.vc_conv3x3_wino4v_supported(B, H, W, Ci, Co, 0) == (1 if v else 0), what + ": linear blocks (lt)"
    assert lib.vc_conv3x3_wino4v_workspace_bytes(B, H, W, Ci) == (v["linear_blocks"] * Ci * 2304 if v else 0), what + ": linear blocks"
    d, r = R.conv_inputs(case, "random"), R.conv_ref(case, "random")
    tol = R.TOL_WINO4
    ys, ps = (B, H, W, Co), (B, H // 2, W // 2, Co)
    ny, npl = int(np.prod(ys)), int(np.prod(ps))
    act = np.maximum(r["pre"], 0)
    scale = np.abs(act).max()
    tx, tw, tb = padded_in(to_c4(d["x"])), padded_in(d["w"]), padded_in(d["b"])
    wp = pack(lib, PACK4, 36, tw, Ci, Co, 0)
    # ---- forward with bias and ReLU, without either; the pre-transformed form bit-identical
    for bias, relu, ref in ((P(tb), 1, act), (None, 0, r["pre0"])):
        y = poisoned(ny)
        lib.vc_conv3x3_wino4_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), bias, P(y), None, relu)
        msg = "%s fwd bias=%s relu=%d" % (what, "yes" if bias else "NULL", relu)
        hy = logical(y, ny, msg)
        compare(nhwc(hy, ys), ref, "random", tol, msg)
        if v:
            yv, (vws, nbytes) = poisoned(ny), vspace(lib, B, H, W, Ci)
            lib.vc_conv3x3_wino4v_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), bias, P(yv), None, relu, P(vws), nbytes)
            same_bits(logical(yv, ny, msg + " (wino4v)"), hy, msg + " (wino4v)")
            logical(vws, nbytes // 4, msg + " (wino4v): workspace")
    # ---- ReLU mask as bits -> the next layer's data gradient
    nm = R.wino4_mask_words(B, H, W, Co)
    y, mask = poisoned(ny), words(nm)
    lib.vc_conv3x3_wino4_fwd_mask_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), 1, P(mask))
    msg = what + " fwd_mask"
    fy = logical(y, ny, msg)
    hy = nhwc(fy, ys)
    compare(hy, act, "random", tol, msg)
    hmask = raw(mask, nm, msg + ": mask")
    wpt2 = pack(lib, PACK4, 36, padded_in(d["w2"]), Co, Ci, 1)
    tdy2 = padded_in(to_c4(d["dy2"]))
    assert lib.vc_conv3x3_wino4_supported(B, H, W, Co, Ci, 1) == 1
    dxa, dxb = poisoned(ny), poisoned(ny)
    lib.vc_conv3x3_wino4_dgrad_f32(stream(), B, H, W, Co, Ci, P(tdy2), P(wpt2), P(y), P(dxa))
    lib.vc_conv3x3_wino4_dgrad_bits_f32(stream(), B, H, W, Co, Ci, P(tdy2), P(wpt2), P(mask), P(dxb))
    msg = what + " dgrad_bits of the next layer"
    ha, hb = logical(dxa, ny, msg + " (float mask)"), logical(dxb, ny, msg)
    same_bits(ha, hb, msg)
    compare(nhwc(hb, ys), r["dx2"] * (hy > 0), "random", tol, msg)
    if v:
        assert lib.vc_conv3x3_wino4v_supported(B, H, W, Co, Ci, 1) == 1
        yv, maskv, (vws, nbytes) = poisoned(ny), words(nm), vspace(lib, B, H, W, Ci)
        lib.vc_conv3x3_wino4v_fwd_mask_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(yv), 1, P(maskv), P(vws), nbytes)
        same_bits(logical(yv, ny, what + " fwd_mask (wino4v)"), fy, what + " fwd_mask (wino4v)")
        same_bits(raw(maskv, nm, what + " fwd_mask (wino4v): mask"), hmask, what + " fwd_mask (wino4v): mask")
        for bits_form in (0, 1):
            dxv, (vws, nbytes) = poisoned(ny), vspace(lib, B, H, W, Ci)
            if bits_form:
                lib.vc_conv3x3_wino4v_dgrad_bits_f32(stream(), B, H, W, Co, Ci, P(tdy2), P(wpt2), P(mask), P(dxv), P(vws), nbytes)
            else:
                lib.vc_conv3x3_wino4v_dgrad_f32(stream(), B, H, W, Co, Ci, P(tdy2), P(wpt2), P(y), P(dxv), P(vws), nbytes)
            msg = "%s dgrad of the next layer (wino4v, bits=%d)" % (what, bits_form)
            same_bits(logical(dxv, ny, msg), hb, msg)
            logical(vws, nbytes // 4, msg + ": workspace")
    # ---- pooled entries: even sizes only; odd ones are refused and write nothing
    nw = R.wino_pool_words(B, H, W, Co)
    if (H | W) & 1:
        y, yp, codes = poisoned(ny), poisoned(npl), words(nw)
        with pytest.raises(VaecapError):
            lib.vc_conv3x3_wino4_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), P(yp), 1)
        with pytest.raises(VaecapError):
            lib.vc_conv3x3_wino4_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), P(yp), P(codes))
        with pytest.raises(VaecapError):
            lib.vc_conv3x3_wino4_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), None, P(yp), P(codes))
        if v:
            vws, nbytes = vspace(lib, B, H, W, Ci)
            with pytest.raises(VaecapError):
                lib.vc_conv3x3_wino4v_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), P(yp), 1, P(vws), nbytes)
            with pytest.raises(VaecapError):
                lib.vc_conv3x3_wino4v_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), P(yp), P(codes), P(vws), nbytes)
            untouched(vws, nbytes // 4, what + " pooled, odd size: workspace")
        untouched(y, ny, what + " pooled, odd size: y")
        untouched(yp, npl, what + " pooled, odd size: ypool")
        untouched(codes, nw, what + " pooled, odd size: codes")
        return
    assert lib.vc_conv3x3_wino_pool_words(B, H, W, Co) == nw
    ypool_ref, _ = R.pool_ref(r["pre"], d["dyp"])
    y, yp = poisoned(ny), poisoned(npl)
    lib.vc_conv3x3_wino4_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y), P(yp), 1)
    msg = what + " fwd + pool"
    py = logical(y, ny, msg + ": y")
    compare(nhwc(py, ys), act, "random", tol, msg + ": y")
    hp = logical(yp, npl, msg + ": ypool")
    compare(nhwc(hp, ps), ypool_ref, "random", tol, msg + ": ypool", scale=scale)
    tdyp = padded_in(to_c4(d["dyp"]))
    hcodes = None
    for store in (1, 0):      # y given; y == NULL: the kernel without its full-size store (STORE = false)
        y, yp, codes = poisoned(ny), poisoned(npl), words(nw)
        lib.vc_conv3x3_wino4_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(y) if store else None, P(yp), P(codes))
        msg = "%s fwd_pool y=%s" % (what, "yes" if store else "NULL")
        if store:
            same_bits(logical(y, ny, msg + ": y"), py, msg + ": y")
        else:
            untouched(y, ny, msg + ": y")
        same_bits(logical(yp, npl, msg + ": ypool"), hp, msg + ": ypool")
        hc = raw(codes, nw, msg + ": codes")
        if hcodes is None:
            hcodes = hc
            dxp = poisoned(ny)
            lib.vc_maxpool2x2_bwd_bits_f32(stream(), B, H, W, Co, P(codes), P(tdyp), P(dxp))
            R.compare_routing(nhwc(logical(dxp, ny, msg + ": routed"), ys), r["pre"], d["dyp"], tol * scale, msg + ": routed")
        same_bits(hc, hcodes, msg + ": codes")
        if v:
            yv, ypv, codesv, (vws, nbytes) = poisoned(ny), poisoned(npl), words(nw), vspace(lib, B, H, W, Ci)
            lib.vc_conv3x3_wino4v_fwd_pool_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(yv) if store else None, P(ypv), P(codesv), P(vws), nbytes)
            msg += " (wino4v)"
            if store:
                same_bits(logical(yv, ny, msg + ": y"), py, msg + ": y")
            else:
                untouched(yv, ny, msg + ": y")
            same_bits(logical(ypv, npl, msg + ": ypool"), hp, msg + ": ypool")
            same_bits(raw(codesv, nw, msg + ": codes"), hcodes, msg + ": codes")
            logical(vws, nbytes // 4, msg + ": workspace")
    if v:
        yv, ypv, (vws, nbytes) = poisoned(ny), poisoned(npl), vspace(lib, B, H, W, Ci)
        lib.vc_conv3x3_wino4v_fwd_f32(stream(), B, H, W, Ci, Co, P(tx), P(wp), P(tb), P(yv), P(ypv), 1, P(vws), nbytes)
        same_bits(logical(yv, ny, what + " fwd + pool (wino4v): y"), py, what + " fwd + pool (wino4v): y")
        same_bits(logical(ypv, npl, what + " fwd + pool (wino4v): ypool"), hp, what + " fwd + pool (wino4v): ypool")


def run_w4_dgrad(lib, case):
    """the case's own data gradient (gathered Cout, produced Cin) against the oracle, with and without relu_src; wino4v bit-identical"""
    B, H, W, Ci, Co = case
    what = "wino4 %s" % R.case_id(case)
    g, v = R.plan_wino4(B, H, W, Co, Ci), R.plan_wino4v(B, H, W, Co, Ci)
    assert lib.vc_conv3x3_wino4_supported(B, H, W, Ci, Co, 1) == 1
    assert lib.vc_conv3x3_wino4_mask_words(B, H, W, Ci) == R.cdiv(g["square_blocks"], 2) * (Ci // 32) * 512
    assert lib.vc_conv3x3_wino4v_supported(B, H, W, Ci, Co, 1) == (1 if v else 0)
    d, r = R.conv_inputs(case, "random"), R.conv_ref(case, "random")
    xs = (B, H, W, Ci)
    nx = int(np.prod(xs))
    tx, tdy = padded_in(to_c4(d["x"])), padded_in(to_c4(d["dy"]))
    wpt = pack(lib, PACK4, 36, padded_in(d["w"]), Ci, Co, 1)
    for src, ref in ((P(tx), r["dx"] * (d["x"] > 0)), (None, r["dx"])):
        dx = poisoned(nx)
        lib.vc_conv3x3_wino4_dgrad_f32(stream(), B, H, W, Ci, Co, P(tdy), P(wpt), src, P(dx))
        msg = "%s dgrad relu_src=%s" % (what, "x" if src else "NULL")
        hx = logical(dx, nx, msg)
        compare(nhwc(hx, xs), ref, "random", R.TOL_WINO4, msg)
        if v:
            dxv, (vws, nbytes) = poisoned(nx), vspace(lib, B, H, W, Co)
            lib.vc_conv3x3_wino4v_dgrad_f32(stream(), B, H, W, Ci, Co, P(tdy), P(wpt), src, P(dxv), P(vws), nbytes)
            same_bits(logical(dxv, nx, msg + " (wino4v)"), hx, msg + " (wino4v)")
            logical(vws, nbytes // 4, msg + " (wino4v): workspace")


@pytest.mark.parametrize("case,lt", [(c, lt) for c, lt, _ in R.W4_ODD_CASES], ids=[i for _, _, i in R.W4_ODD_CASES])
def test_wino4_odd_and_tiny_sizes(lib, case, lt):
    """any H, W >= 4: "stores and pooling windows past the image are masked" (plan_wino4) -- in the square-block and the linear-tile form,
    forward, mask bits and data gradient"""
    B, H, W, Ci, Co = case
    g = R.plan_wino4(*case)
    assert lt is None or g["lt"] == lt
    run_w4_forward(lib, case)
    if R.plan_wino4(B, H, W, Co, Ci) is not None:
        run_w4_dgrad(lib, case)
    else:
        assert Ci % 32 and lib.vc_conv3x3_wino4_supported(B, H, W, Ci, Co, 1) == 0


@pytest.mark.parametrize("case,tiles,tg,chunks", [c[:4] for c in R.W4_ORDER_CASES], ids=[c[4] for c in R.W4_ORDER_CASES])
def test_wino4_workgroup_order_forward(lib, case, tiles, tg, chunks):
    """wino4_launch's id -> (chunk of tg channel tiles, block pair, tile of the chunk) map past one chunk, and unchunked with an odd tile
    count; three square blocks: the second block pair is half empty.  Includes the pooled forward without its full-size store."""
    g = R.plan_wino4(*case)
    assert (g["lt"], g["nblocks"], g["tiles_n"], g["tg"], g["chunks_n"]) == (0, 3, tiles, tg, chunks)
    run_w4_forward(lib, case)


def test_wino4_workgroup_order_data_gradient(lib):
    B, H, W, Ci, Co = R.W4_ORDER_DGRAD_CASE
    g = R.plan_wino4(B, H, W, Co, Ci)
    assert (g["lt"], g["nblocks"], g["tiles_n"], g["tg"], g["chunks_n"]) == (0, 3, 8, 4, 2)
    run_w4_dgrad(lib, R.W4_ORDER_DGRAD_CASE)


# =================================================================== F(3x3,2x2) weight gradient (csrc/conv_wino_wgrad*.hip)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case,expect", [(c, e) for c, e, _ in R.WG_CASES], ids=[i for _, _, i in R.WG_CASES])
def test_wino_wgrad_split_and_block_edges(lib, case, expect, kind):
    """K splits of several blocks with a short last split, one split that walks every block, a block smaller than its shape, ragged
    multi-block images in each block shape: dw and db; accumulate = 1 onto non-zero dw / db; db == NULL; a workspace one float short"""
    B, H, W, Ci, Co = case
    what = "wino wgrad %s %s" % (R.case_id(case), kind)
    p = R.plan_wino_wgrad(*case)
    for k, v in expect.items():
        assert (R.ragged(p) if k == "ragged" else p[k]) == v, (what, k)
    assert lib.vc_conv3x3_wino_wgrad_supported(B, H, W, Ci, Co) == 1
    nbytes = lib.vc_conv3x3_wino_wgrad_workspace_bytes(B, H, W, Ci, Co)
    assert nbytes == p["nsplit"] * (16 * Ci * Co + Co) * 4, "%s: plan_wino_wgrad now gives %.2f splits, not %d" % (what, nbytes / ((16 * Ci * Co + Co) * 4.0), p["nsplit"])
    d, r = R.wgrad_inputs(case, kind), R.wgrad_ref(case, kind)
    if kind == "exact":
        ntiles = B * p["TW"] * p["TH"]
        assert R.exact_bound_wgrad(ntiles, d["x"], d["dy"], d["dw0"]) < R.EXACT_LIMIT, what
        assert R.exact_bound_wgrad(ntiles, np.ones(1), d["dy"], d["db0"]) < R.EXACT_LIMIT, what
    tol = R.tol_wgrad(B * H * W)
    MN, nws = 9 * Ci * Co, nbytes // 4
    tx, tdy = padded_in(to_c4(d["x"])), padded_in(to_c4(d["dy"]))

    def call(dw, db, acc, ws, size=nbytes):
        lib.vc_conv3x3_wino_wgrad_f32(stream(), B, H, W, Ci, Co, P(tx), P(tdy), P(dw), db, acc, P(ws), size)

    # ---- db given, accumulate = 0
    ws, dw, db = poisoned(nws), poisoned(MN), poisoned(Co)
    call(dw, P(db), 0, ws)
    first = logical(dw, MN, what + " dw")
    compare(first, r["dw"], kind, tol, what + " dw")
    compare(logical(db, Co, what + " db"), r["db"], kind, tol, what + " db")
    logical(ws, nws, what + ": a split left part of its partial sums unwritten; workspace")
    # ---- accumulate = 1 onto non-zero dw / db
    ws, dw, db = poisoned(nws), guarded(d["dw0"]), guarded(d["db0"])
    call(dw, P(db), 1, ws)
    compare(logical(dw, MN, what + " dw, accumulate"), d["dw0"].astype(np.float64) + r["dw"], kind, tol, what + " dw, accumulate")
    compare(logical(db, Co, what + " db, accumulate"), d["db0"].astype(np.float64) + r["db"], kind, tol, what + " db, accumulate")
    raw(ws, nws, what + " workspace, accumulate")
    # ---- db == NULL: the same dw bit for bit, db untouched
    ws, dw, db = poisoned(nws), poisoned(MN), poisoned(Co)
    call(dw, None, 0, ws)
    same_bits(logical(dw, MN, what + " dw, db = NULL"), first, what + " dw, db = NULL")
    untouched(db, Co, what + " db, db = NULL")
    raw(ws, nws, what + " workspace, db = NULL")
    # ---- a workspace one float short: VC_EWORKSPACE (10002), nothing written
    ws, dw = poisoned(nws), poisoned(MN)
    with pytest.raises(VaecapError, match="code 10002"):
        call(dw, P(db), 0, ws, nbytes - 4)
    untouched(dw, MN, what + " dw, short workspace")
    untouched(db, Co, what + " db, short workspace")
    untouched(ws, nws, what + " workspace, short workspace")
