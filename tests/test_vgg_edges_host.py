"""CPU only: what tests/test_gpu_vgg_edges.py takes for granted about tests/vgg_edges_ref.py.

  * every "exact" convolution case really is exact: n_terms * max|a| * max|b| (+ max|addend|) < 2**24 from the actual arrays, and the
    float64 oracle's outputs are integers;
  * the exact inputs are not degenerate: more than half of every compared tensor is non-zero (of a weight gradient: more than half of
    the taps that meet a pixel pair inside the image -- at H = 1 or W = 1 the other taps are zero by construction);
  * the case tables say what their comments say (pixel groups, partial counts, item counts past the grid cap);
  * the host-built max-pool routing codes decode back to the oracle's MaxPoolGrad."""
import numpy as np
import pytest

from oracle import vgg as OV

from . import vgg_edges_ref as R

GRID_CAP_ITEMS = R.GRID_CAP_ITEMS


def _integers(a):
    return np.array_equal(a, np.rint(a)) and np.abs(a).max() < R.EXACT_LIMIT


def _mostly_nonzero(a, what, of=None):
    a = np.asarray(a)
    n = a.size if of is None else int(np.broadcast_to(of, a.shape).sum())
    nz = int(np.count_nonzero(a))
    assert 2 * nz > n, "%s: only %d of %d elements non-zero" % (what, nz, n)


def _check_wgrad(x, dy, dw0, db0, dw, db, H, W, what):
    n = dy.shape[0] * dy.shape[1] * dy.shape[2]
    assert R.is_exact(n, x, dy, dw0), what
    assert R.is_exact(n, np.ones(1), dy, db0), what
    assert _integers(dw) and _integers(db), what
    taps = R.reachable_taps(H, W)[:, :, None, None]
    assert not dw[~np.broadcast_to(taps, dw.shape)].any()
    _mostly_nonzero(dw, what + " dw", of=taps)
    _mostly_nonzero(db, what + " db")
    _mostly_nonzero(dw0, what + " dw0")


@pytest.mark.parametrize("case", [c for c, _, _ in R.WGRAD_CASES], ids=R.case_id)
def test_exact_weight_gradient_cases_are_exact_and_not_degenerate(case):
    B, H, W, Ci, Co = case
    x, w, b, dy, dw0, db0 = R.conv_inputs(case, "exact")
    _, dw, db = R.conv_bwd_ref(case, "exact", False)
    _check_wgrad(x, dy, dw0, db0, dw, db, H, W, R.case_id(case))


def test_the_issue_figure_of_the_largest_weight_gradient_case():
    case = (2, 256, 257, 4, 8)
    _, dw, _ = R.conv_bwd_ref(case, "exact", False)
    assert 1000 < np.abs(dw).max() < R.EXACT_LIMIT / 100     # |dw| ~ 6e3: orders of magnitude inside the limit


@pytest.mark.parametrize("case", R.GEOM_CASES + [R.DGRAD_WS_CASE], ids=R.case_id)
def test_exact_forward_and_gradient_cases_are_exact_and_not_degenerate(case):
    B, H, W, Ci, Co = case
    what = R.case_id(case)
    x, w, b, dy, dw0, db0 = R.conv_inputs(case, "exact")
    assert x.min() >= 0 and x.max() <= 7 and np.abs(w).max() <= 3 and np.abs(b).max() <= 5 and np.abs(dy).max() <= 3
    assert R.is_exact(9 * Ci, x, w, b), what
    assert R.is_exact(9 * Co, dy, w), what
    yb, y = R.conv_fwd_ref(case, "exact")
    dx, dw, db = R.conv_bwd_ref(case, "exact", True)
    assert _integers(yb) and _integers(y) and _integers(dx), what
    for name, a in (("y", y), ("y + b", yb), ("relu(y)", np.maximum(y, 0)), ("relu(y + b)", np.maximum(yb, 0)), ("dx", dx),
                    ("dx * (x > 0)", dx * (x > 0))):
        _mostly_nonzero(a, "%s %s" % (what, name))
    if case != R.DGRAD_WS_CASE:
        _check_wgrad(x, dy, dw0, db0, dw, db, H, W, what)


@pytest.mark.parametrize("shape", sorted({s for s, _ in R.CONV1_FWD_CASES + R.CONV1_WGRAD_CASES}), ids=R.case_id)
def test_exact_conv1_cases_are_exact_and_not_degenerate(shape):
    B, H, W = shape
    what = R.case_id(shape)
    x4, w, b, dy, dw0, db0 = R.conv1_inputs(shape, "exact")
    assert np.abs(x4).max() <= 4 and not x4[..., 3].any() and np.abs(w).max() <= 3 and np.abs(b).max() <= 5
    if shape in [s for s, _ in R.CONV1_FWD_CASES]:
        assert R.is_exact(27, x4, w, b), what
        pre = R.conv1_fwd_ref(shape, "exact")
        assert _integers(pre), what
        _mostly_nonzero(pre, what + " y")
        _mostly_nonzero(np.maximum(pre, 0), what + " relu(y)")
    if shape in [s for s, _ in R.CONV1_WGRAD_CASES]:
        dw, db = R.conv1_wgrad_ref(shape, "exact")
        _check_wgrad(x4, dy, dw0, db0, dw, db, H, W, what)
        if shape == (3, 1821, 96):
            assert 1000 < np.abs(dw).max() < R.EXACT_LIMIT / 100   # |dw| ~ 2e4


def test_case_tables_reach_the_edges_they_name():
    for (B, H, W), groups in R.CONV1_FWD_CASES:
        assert W % 32 == 0 and B * H * W // 32 == groups
    waves = 2048 * 4                                        # conv1_fwd_kernel: at most 2048 workgroups of four waves
    assert [g for _, g in R.CONV1_FWD_CASES] == [1, 3, 20, waves, waves + 1, 2 * waves + 5]
    for (B, H, W), parts in R.CONV1_WGRAD_CASES:
        groups = B * H * W // 32
        assert W % 32 == 0 and min(-(-groups // 4), 1024) == parts
    # the reduce loop (`p + 8 < parts; p += 16`, then one leftover): no pair / leftover only; first pair; pairs only; pair + leftover; ...
    assert [p for _, p in R.CONV1_WGRAD_CASES] == [1, 8, 9, 16, 17, 24, 1024, 1024]
    assert 1 * 241 * 544 // 32 == 4 * 1024 + 1             # one wave of the capped launch takes two groups
    for (B, H, W, Ci, Co), _, splits in R.WGRAD_CASES:
        assert (splits > 1) == (B * H * W >= 1024)          # plan_wgrad: one split per 512 pixels
    B, H, W, C = R.POOL_WRAP
    assert B * (H // 2) * (W // 2) * (C // 4) > GRID_CAP_ITEMS
    B, H, W, C = R.LAYOUT_WRAP
    assert B * H * W * (C // 4) > GRID_CAP_ITEMS
    assert np.prod(R.PREPROCESS_F32[0]) > GRID_CAP_ITEMS and np.prod(R.PREPROCESS_U8[0]) // 4 > GRID_CAP_ITEMS
    for outer, cs, cd, inner in R.PAD_DIM[:2]:
        assert outer * cd * inner > GRID_CAP_ITEMS


@pytest.mark.parametrize("shape", R.POOL_SMALL + [(2, 6, 8, 16)], ids=R.case_id)
def test_pool_codes_decode_to_the_oracles_maxpool_gradient(shape):
    x, dy = R.pool_inputs(shape)
    y, arg, dx, dxr = R.pool_ref(shape)
    codes = R.pool_codes(arg, y)
    B, H, W, C = shape
    assert codes.shape == (B, C // 4, H // 2, W // 2) and codes.dtype == np.uint16
    np.testing.assert_array_equal(R.decode_pool_codes(codes, dy, shape), dxr)
    np.testing.assert_array_equal(dxr, OV.maxpool_bwd(dy, arg, shape) * (x > 0))   # the form tests/test_gpu_ops.py uses
    # one element by hand: channel 4 q + j of image b at pooled (r, c) is nibble j of half-word [b, q, r, c]
    b, r, c, ch = B - 1, 0, W // 2 - 1, C - 3
    nib = (int(codes[b, ch // 4, r, c]) >> (4 * (ch % 4))) & 15
    win = x[b, 2 * r:2 * r + 2, 2 * c:2 * c + 2, ch].ravel()
    assert nib & 3 == int(np.argmax(win)) and bool(nib & 4) == bool(win.max() > 0)
    # the planted ties: zeros -> first position, no ReLU gradient; the positive pair -> first position
    assert int(codes[0, 0, 0, 0]) == 0
    if W >= 4:
        assert int(codes[B - 1, 0, 0, 1]) == 0x4444
    assert (y < 0).any() or x.size < 64                      # windows with a negative maximum occur
    words = R.pool_codes_words(codes)
    assert words.dtype == np.uint32 and words.size == (codes.size + 1) // 2
    assert int(words[0]) & 0xffff == int(codes.ravel()[0])


def test_layout_and_preprocess_references():
    a = np.arange(2 * 3 * 5 * 8, dtype=np.float32).reshape(2, 3, 5, 8)
    c4 = R.to_c4(a)
    assert c4.shape == (2, 2, 3, 5, 4) and c4[1, 1, 2, 4, 3] == a[1, 2, 4, 7]
    img = np.array([[[[0, 128, 255]]]], np.uint8)
    np.testing.assert_array_equal(R.preprocess_ref(img)[0, 0, 0], np.array([0, 128, 255, 0], np.float32) - np.append(OV.MEAN_RGB, np.float32(0)))
    src = np.arange(2 * 3 * 2, dtype=np.float32).reshape(2, 3, 2)
    assert R.pad_dim_ref(src, 4).shape == (2, 4, 2) and not R.pad_dim_ref(src, 4)[:, 3].any()
    np.testing.assert_array_equal(R.pad_dim_ref(R.pad_dim_ref(src, 4), 3), src)
