"""CPU only: what tests/test_gpu_wino_edges.py takes for granted about tests/wino_edges_ref.py.

  * the case tables say what their ids say: one F(2x2,3x3) case per distinct (TBH, TBW, P) of the restated plan over even H, W <= 64
    (38 of them: a plan change must show up here, not as an emptied table), ragged cases ragged in the direction they name, K-split cases
    with a short last split, block orders with the chunk counts they name, refusals refused;
  * every "exact" case really is exact -- the bound of every partial sum IN THE TRANSFORMED DOMAIN, from the actual arrays, is below
    2**24, the transformed weights are integers -- the float64 oracle's outputs are integers, and more than half of every compared
    tensor is non-zero (of a MaxPoolGrad, which fills at most a quarter: more than half of the windows route a gradient);
  * the new rules bite: the GPU test's own comparison helpers fail on an oracle output with one element of a ragged block left NaN, with
    one guard element changed, and with one block dropped from the last K split of an exact weight-gradient case."""
import numpy as np
import pytest

from . import wino_edges_ref as R

f32 = np.float32


def _integers(a):
    return np.array_equal(a, np.rint(a)) and np.abs(a).max() < R.EXACT_LIMIT


def _mostly_nonzero(a, what):
    a = np.asarray(a)
    nz = int(np.count_nonzero(a))
    assert 2 * nz > a.size, "%s: only %d of %d elements non-zero" % (what, nz, a.size)


W2_EXACT = [c for c, _, _ in R.W2_SHAPE_CASES] + [c for c, _, _, _ in R.W2_RAGGED_CASES]


# ------------------------------------------------------------------------------------------------ the plans and their tables
def test_the_row_pitch_search_gives_the_pitches_the_kernel_comment_names():
    """csrc/conv_wino.hip: "P = 6 (4 x 4 tiles) and P = 12 (2 x 7 tiles)"; the 224 / 112 / 56-wide layers get 4 x 4 blocks.  (The 28-
    wide layers get 2 x 7 as that comment says, the 14-wide ones 7 x 2: of equally efficient shapes the search keeps the narrowest.)"""
    assert R.wino2_row_pitch_search(4, 4) == 6 and R.wino2_row_pitch_search(2, 7) == 12
    for H in (224, 112, 56):
        g = R.plan_wino2(1, H, H, 64, 64)
        assert (g["TBH"], g["TBW"], g["P"]) == (4, 4, 6)
    assert [(g["TBH"], g["TBW"], g["P"]) for g in (R.plan_wino2(1, H, H, 64, 64) for H in (28, 14))] == [(2, 7, 12), (7, 2, 3)]
    assert R.wino2_row_pitch_search(16, 2) == 0         # 34 rows of three pairs: no pitch fits the 79 units of a plane


def test_one_case_per_block_shape_of_the_plan():
    shapes = R.wino2_block_shapes()
    assert len(shapes) == 38 and len(R.W2_SHAPE_CASES) == 38
    names = sorted((tbh, tbw) for tbh, tbw, _ in shapes)
    assert len(set(names)) == 38                        # one pitch per block shape
    expect = [(1, w) for w in range(1, 12)] + [(2, w) for w in range(1, 8)] + [(3, w) for w in range(1, 6)] + [(4, w) for w in range(1, 5)] + \
             [(5, w) for w in range(1, 4)] + [(6, 1), (6, 2), (7, 1), (7, 2)] + [(h, 1) for h in range(8, 12)]
    assert names == sorted(expect)
    assert len({i for _, _, i in R.W2_SHAPE_CASES}) == 38
    for (B, H, W, Ci, Co), (tbh, tbw, p), _ in R.W2_SHAPE_CASES:
        g = R.plan_wino2(B, H, W, Ci, Co)
        assert (H, W) == (2 * tbh, 2 * tbw) and (g["TBH"], g["TBW"], g["P"]) == (tbh, tbw, p)
        assert g["blocks_img"] == 1 and g["nblocks"] == 5 and g["workgroups"] == 2     # a full workgroup and one with three empty blocks
        assert g["PH"] * g["PW"] <= R.W2_PIX and g["PH"] * g["P"] <= R.W2_PLANE - 1 and 2 * g["P"] >= g["PW"]
        assert R.plan_wino2(B, H, W, Co, Ci) is not None                                # the data gradient runs too
        assert R.wino_mask_words(4, H, W, Co) == 256 and R.wino_mask_words(5, H, W, Co) == 512
    assert sum(1 for _, (tbh, tbw, _), _ in R.W2_SHAPE_CASES if tbh * tbw < 16) >= 30   # blocks with dead lanes (lj >= ntl)


def test_ragged_long_and_refused_cases_of_the_f2_plan():
    for case, directions, mod4, _ in R.W2_RAGGED_CASES:
        g = R.plan_wino2(*case)
        assert R.ragged(g) == directions and g["blocks_img"] > 1
        if mod4 is not None:
            assert g["nblocks"] % 4 == mod4
    g = R.plan_wino2(*R.W2_RAGGED_CASES[0][0])
    assert (g["TBH"], g["TBW"], g["bx_n"], g["by_n"], g["nblocks"]) == (5, 3, 6, 4, 24)
    g = R.plan_wino2(*R.W2_RAGGED_CASES[2][0])
    assert g["N"] // 32 == 3 and g["chunks"] == 3
    assert R.plan_wino2(*R.W2_LONG_CASE)["chunks"] == 32
    for case in R.W2_REFUSED:
        assert R.plan_wino2(*case) is None and R.wino_mask_words(*case[:3], 32) == 0
    assert R.wino_pool_words(3, 6, 10, 64) == 3 * 3 * 5 * 16 // 2


def test_f4_cases_take_the_block_form_and_the_order_they_name():
    for case, lt, name in R.W4_ODD_CASES:
        B, H, W, Ci, Co = case
        g = R.plan_wino4(*case)
        assert g is not None and (lt is None or g["lt"] == lt), name
        assert name.startswith("strip") or (H | W) & 1 or (H, W) == (4, 4)
        # the pre-transformed form takes the linear cases (and one 4 x 4-tile square per image); its workspace is per linear block
        v = R.plan_wino4v(*case)
        assert (v is not None) == bool(g["lt"]), name
        if v is not None:
            assert R.wino4v_workspace_bytes(B, H, W, Ci) == R.cdiv(B * R.cdiv(H, 4) * R.cdiv(W, 4), 16) * Ci * 2304
        assert R.wino4_mask_words(B, H, W, Co) == R.cdiv(B * R.cdiv(H, 16) * R.cdiv(W, 16), 2) * (Co // 32) * 512
    assert [g for g in (R.plan_wino4(*c)["square_blocks"] for c, _, _ in R.W4_ODD_CASES[:5])] == [1, 1, 2, 2, 3]
    for case, tiles, tg, chunks, name in R.W4_ORDER_CASES:
        g = R.plan_wino4(*case)
        assert (g["lt"], g["nblocks"], g["pairs"]) == (0, 3, 2), name              # three square blocks: the second pair is ragged
        assert (g["tiles_n"], g["tg"], g["chunks_n"], g["per_chunk"]) == (tiles, tg, chunks, 2 * tg), name
    B, H, W, Ci, Co = R.W4_ORDER_DGRAD_CASE
    g = R.plan_wino4(B, H, W, Co, Ci)                                                # gathered = Cout, produced = Cin
    assert (g["lt"], g["pairs"], g["tiles_n"], g["tg"], g["chunks_n"]) == (0, 2, 8, 4, 2)
    assert R.plan_wino4(1, 3, 8, 32, 32) is None and R.plan_wino4(1, 8, 8, 32, 48) is None and R.plan_wino4(1, 8, 8, 4, 32) is None
    assert R.plan_wino4v(2, 8, 8, 32, 32) is not None and R.plan_wino4v(1, 8, 8, 32, 32) is None      # tests/test_gpu_conv_wino4.py
    assert R.wino4v_workspace_bytes(2, 224, 224, 64) == 0


def test_weight_gradient_cases_reach_the_split_and_block_edges_they_name():
    for case, expect, name in R.WG_CASES:
        p = R.plan_wino_wgrad(*case)
        for k, v in expect.items():
            assert (R.ragged(p) if k == "ragged" else p[k]) == v, (name, k)
        assert 1 <= p["last"] <= p["cps"] and (p["nsplit"] - 1) * p["cps"] + p["last"] == p["nblocks"]
        if "cps" in name:
            assert p["cps"] >= 2 and p["last"] < p["cps"], name                      # a short last split
        if "ragged" in name:
            assert p["blocks_img"] > 1, name
        B, H, W, C, N = case
        assert R.wino_wgrad_workspace_bytes(*case) == p["nsplit"] * (16 * C * N + N) * 4
    assert sorted(R.plan_wino_wgrad(*c)["shape"] for c, _, _ in R.WG_CASES[4:]) == [0, 1, 2]
    assert R.plan_wino_wgrad(1, 2, 8, 64, 64) is None and R.plan_wino_wgrad(1, 4, 8, 32, 64) is None and R.plan_wino_wgrad(1, 5, 8, 64, 64) is None
    # production, conv5_x at 64 images: 128 blocks in four splits of 32
    p = R.plan_wino_wgrad(64, 14, 14, 512, 512)
    assert (p["TBH"], p["TBW"], p["ns"], p["cps"], p["nsplit"]) == (4, 7, 4, 32, 4)


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("case", W2_EXACT, ids=R.case_id)
def test_exact_f2_cases_are_exact_and_not_degenerate(case):
    B, H, W, Ci, Co = case
    what = R.case_id(case)
    d, r = R.conv_inputs(case, "exact"), R.conv_ref(case, "exact")
    assert d["x"].min() >= 0 and d["x"].max() <= 7 and np.abs(d["w"]).max() <= 12 and np.abs(d["dy"]).max() <= 3
    for w in (d["w"], d["w2"]):
        assert R.weights_transform_to_integers(w), what
    assert R.exact_bound_fwd(Ci, d["x"], d["w"], d["b"]) < R.EXACT_LIMIT, what            # forward
    assert R.exact_bound_fwd(Co, d["dy"], d["w"]) < R.EXACT_LIMIT, what                   # data gradient
    assert R.exact_bound_fwd(Ci, d["dy2"], d["w2"]) < R.EXACT_LIMIT, what                 # data gradient of the next layer
    act = np.maximum(r["pre"], 0)
    ypool, dpool = R.pool_ref(r["pre"], d["dyp"])
    for name, a in (("y", r["pre0"]), ("y + b", r["pre"]), ("relu(y + b)", act), ("dx", r["dx"]), ("dx * (x > 0)", r["dx"] * (d["x"] > 0)),
                    ("dx2 * (y > 0)", r["dx2"] * (act > 0)), ("pooled", ypool)):
        assert _integers(a), "%s %s" % (what, name)
        _mostly_nonzero(a, "%s %s" % (what, name))
    assert _integers(dpool) and 2 * np.count_nonzero(dpool) > ypool.size, what           # more than half of the windows route a gradient
    assert not R.ambiguous_windows(r["pre"], 0.0).any()


@pytest.mark.parametrize("case", [c for c, _, _ in R.WG_CASES], ids=R.case_id)
def test_exact_weight_gradient_cases_are_exact_and_not_degenerate(case):
    what = R.case_id(case)
    d, r = R.wgrad_inputs(case, "exact"), R.wgrad_ref(case, "exact")
    p = R.plan_wino_wgrad(*case)
    ntiles = p["B"] * p["TW"] * p["TH"]
    assert R.exact_bound_wgrad(ntiles, d["x"], d["dy"], d["dw0"]) < R.EXACT_LIMIT, what
    assert R.exact_bound_wgrad(ntiles, np.ones(1), d["dy"], d["db0"]) < R.EXACT_LIMIT, what
    assert _integers(r["dw"]) and _integers(r["db"]), what
    for name, a in (("dw", r["dw"]), ("db", r["db"]), ("dw0 + dw", d["dw0"] + r["dw"]), ("db0 + db", d["db0"] + r["db"])):
        _mostly_nonzero(a, "%s %s" % (what, name))


def test_random_f4_inputs_are_not_degenerate():
    for case in [c for c, _, _ in R.W4_ODD_CASES] + [c for c, _, _, _, _ in R.W4_ORDER_CASES]:
        d, r = R.conv_inputs(case, "random"), R.conv_ref(case, "random")
        assert 0.2 < (r["pre"] > 0).mean() < 0.8 and 0.2 < (d["x"] > 0).mean() < 0.8, case
        assert R.ambiguous_windows(r["pre"][:, :case[1] & ~1, :case[2] & ~1], R.TOL_WINO4 * np.abs(r["pre"]).max()).mean() < 0.01, case


# ------------------------------------------------------------------------------------------------ the rules bite
def _from_c4(a, shape):
    B, H, W, C = shape
    return np.ascontiguousarray(np.asarray(a).reshape(B, C // 4, H, W, 4).transpose(0, 2, 3, 1, 4).reshape(B, H, W, C))


def _fails(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def test_a_ragged_block_element_left_nan_and_a_changed_guard_element_fail():
    case = R.W2_RAGGED_CASES[0][0]                                      # 34 x 34: the last block column and row are ragged
    B, H, W, Ci, Co = case
    g = R.plan_wino2(*case)
    ref = np.maximum(R.conv_ref(case, "exact")["pre"], 0)
    good = R.V.to_c4(ref).astype(f32)
    n = good.size
    buf = R.with_guard(good)
    R.compare(_from_c4(R.logical(buf, n, "y"), ref.shape), ref, "exact", 0.0, "y")          # the unperturbed output passes
    # ---- one element of the last (ragged in x and y) block never written
    y, x = 2 * g["TBH"] * (g["by_n"] - 1), 2 * g["TBW"] * (g["bx_n"] - 1)
    assert H - y < 2 * g["TBH"] and W - x < 2 * g["TBW"]
    hole = good.copy()
    hole[0, Co // 4 - 1, H - 1, W - 1, 3] = np.nan
    _fails(R.logical, R.with_guard(hole), n, "y")
    # ---- an element of a ragged block that is zero behind the ReLU, left at a wrong value: the zero-initialised tests could not see NaN there
    zeros = np.argwhere(good[0, :, :, x:, :] == 0)                      # (the last block column)
    assert len(zeros)
    q, yy, xx, e = zeros[-1]
    stale = good.copy()
    stale[0, q, yy, x + xx, e] = np.nan
    _fails(R.logical, R.with_guard(stale), n, "y")
    # ---- one guard element changed (a store past the last image), float and integer buffers
    for k in (0, R.GUARD - 1):
        over = buf.copy()
        over[n + k] = 0.0
        _fails(R.raw, over, n, "y")
    words = R.poison(256, np.uint32)
    R.untouched(words, 256, "mask")
    over = words.copy()
    over[256] ^= np.uint32(1)
    _fails(R.raw, over, 256, "mask")
    over = words.copy()
    over[255] = 0
    _fails(R.untouched, over, 256, "mask")
    _fails(R.raw, buf[:-1], n, "y")                                     # a buffer of another size than the query says


def test_a_block_dropped_from_the_last_k_split_fails_the_exact_comparison():
    case, _, _ = R.WG_CASES[0]                                          # 17 blocks, cps = 2: the last split holds block 16 alone
    p = R.plan_wino_wgrad(*case)
    assert p["last"] == 1 and p["cps"] == 2
    d, r = R.wgrad_inputs(case, "exact"), R.wgrad_ref(case, "exact")
    R.compare(r["dw"].astype(f32), r["dw"], "exact", 0.0, "dw")
    b, ys, xs = R.wgrad_block_region(p, p["nblocks"] - 1)
    assert b == case[0] - 1
    dy = d["dy"].copy()
    dy[b, ys, xs] = 0                                                   # what a split that stops one block early sums
    dw, db = R.oracle_wgrad(d["x"], dy)
    assert 0 < np.abs(dw - r["dw"]).max() <= 16 * 7 * 3                 # sixteen pixels of one image out of seventeen
    _fails(R.compare, dw.astype(f32), r["dw"], "exact", 0.0, "dw")
    _fails(R.compare, db.astype(f32), r["db"], "exact", 0.0, "db")
