"""Plans, cases, inputs, expected values and comparison helpers of tests/test_gpu_wino_edges.py and tests/test_wino_edges_host.py: numpy
and oracle/vgg.py only (no GPU, no library call, no torch), so that the CPU test can check every property the GPU test relies on.

  * the host-side plans of the Winograd kernels restated in Python -- plan_wino2 with its LDS row-pitch search (csrc/conv_wino.hip),
    plan_wino4 / plan_wino4v with the workgroup order of wino4_launch (csrc/conv_wino4.hip), plan_wino_wgrad (csrc/conv_wino_wgrad.hip)
    -- and the size formulas of the buffer queries.  The GPU test asserts that the library agrees through what the ABI exports; the case
    tables below are GENERATED from these plans, so a case names its edge only while the plan still puts it there;
  * two kinds of input for F(2x2,3x3) and the weight gradient F(3x3,2x2):
      "exact"   small integers stored as float32 whose TRANSFORMED values are integers too (weights are multiples of 4: G has two 1/2);
                while the bound of every partial sum in the transformed domain (`exact_bound_fwd`, `exact_bound_wgrad`, from the actual
                arrays) stays below 2**24, fp32 arithmetic is exact in any order and the kernel's output must EQUAL the float64 oracle's;
      "random"  standard normal, for the project's rounding tolerances (`tol_wino2`, `tol_wgrad`).
    F(4x4,3x3) has no exact kind (G holds 1/6 and 1/24): random inputs and the flat tolerance `TOL_WINO4`;
  * the comparison helpers of the GPU test (guard bands, unwritten elements, equality / tolerance): they take host arrays, so the CPU test
    can show that each of them fails on a perturbed oracle output."""
import functools
import zlib

import numpy as np

from oracle import vgg as OV

from . import vgg_edges_ref as V

f32 = np.float32
f64 = np.float64
KINDS = V.KINDS
EXACT_LIMIT = V.EXACT_LIMIT
GUARD = 64
SENTINEL = f32(-24680.5)
SENTINEL_WORD = np.uint32(0x5A5AA5A5)
ONES_WORD = np.uint32(0xFFFFFFFF)
NAN = f32(np.nan)
TOL_WINO4 = 6e-5                      # tests/test_gpu_conv_wino4.py: flat, of max|ref|
LAUNCH_BYTES = 0x7fffffff             # a launch addresses its tensors with 32-bit byte offsets


def cdiv(a, b):
    return -(-a // b)


def tol_wino2(K):
    """tests/test_gpu_conv_wino.py: of max|ref|; K = 9 Cin (forward), 9 Cout (data gradient)"""
    return 3e-6 * np.sqrt(K) + 1e-6


def tol_wgrad(npix):
    """tests/test_gpu_conv_wino.py: of max|ref|; npix = B H W"""
    return 3e-6 * np.sqrt(npix) + 1e-6


# ================================================================================================ F(2x2,3x3): csrc/conv_wino.hip
W2_PIX = 100       # patch pixels of a block: (2 TBH + 2)(2 TBW + 2) <= 100
W2_PLANE = 80      # 16-byte units per LDS plane: PH * P <= 79 (unit 79 is the dump slot of the staging writes)
# the sixteen lanes each of the four groups a wave64 ds_read_b128 is served in
W2_LANE_GROUPS = ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27), (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31),
                  (32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59), (36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63))


@functools.lru_cache(maxsize=None)
def wino2_row_pitch_search(TBH, TBW):
    """wino2_row_pitch_search: the pitch P (pixel pairs per patch row) with the fewest bank conflicts, the smallest such; 0: no fit.
    cost = sum over (patch row r, pixel pair c, lane group) of the largest number of DISTINCT units on one bank quad (unit mod 16)"""
    PW, PH, ntl = 2 * TBW + 2, 2 * TBH + 2, TBH * TBW
    best, best_cost = 0, 1 << 30
    P = PW // 2
    while PH * P <= W2_PLANE - 1:
        cost = 0
        for r in range(4):
            for c in range(2):
                for group in W2_LANE_GROUPS:
                    units = set()
                    for lane in group:
                        lj, lg = lane & 15, lane >> 4
                        jt = lj if lj < ntl else 0
                        units.add(lg * W2_PLANE + (2 * (jt // TBW) + r) * P + jt % TBW + c)
                    quads = [u & 15 for u in units]
                    cost += max(quads.count(q) for q in set(quads))
        if cost < best_cost:
            best_cost, best = cost, P
        P += 1
    return best


def plan_wino2(B, H, W, C, N):
    """plan_wino2 -> dict or None (refused).  C = gathered channels, N = produced channels"""
    if B <= 0 or H < 2 or W < 2 or (H & 1) or (W & 1) or C <= 0 or N <= 0 or C % 16 or N % 32:
        return None
    if B * H * W * max(C, N) * 4 > LAUNCH_BYTES or 16 * C * N * 4 > LAUNCH_BYTES:
        return None
    TW, TH = W // 2, H // 2
    best, best_h, best_eff = 0, 0, 0.0
    for tbw in range(1, min(16, TW) + 1):
        tbh = min(16 // tbw, TH)
        if (2 * tbh + 2) * (2 * tbw + 2) > W2_PIX:
            continue
        eff = float(TW * TH) / (float(cdiv(TW, tbw)) * cdiv(TH, tbh) * 16.0)
        if eff > best_eff + 1e-9:
            best_eff, best, best_h = eff, tbw, tbh
    if not best:
        return None
    g = dict(B=B, H=H, W=W, C=C, N=N, TW=TW, TH=TH, TBW=best, TBH=best_h, PW=2 * best + 2, PH=2 * best_h + 2)
    g["bx_n"], g["by_n"] = cdiv(TW, best), cdiv(TH, best_h)
    g["blocks_img"] = g["bx_n"] * g["by_n"]
    g["nblocks"] = B * g["blocks_img"]
    if g["nblocks"] > 0x3fffffff or g["nblocks"] * g["blocks_img"] >= 1 << 32:
        return None
    g["P"] = wino2_row_pitch_search(best_h, best)
    if g["P"] <= 0:
        return None
    g["workgroups"] = cdiv(g["nblocks"], 4)             # four blocks per workgroup (x N / 32 channel tiles)
    g["chunks"] = C // 16
    return g


def wino_mask_words(B, H, W, C):
    """vc_conv3x3_wino_mask_words: 256 words per workgroup, blocks rounded up to four per workgroup"""
    g = plan_wino2(B, H, W, 16, C)
    return 0 if g is None else cdiv(g["nblocks"], 4) * (C // 32) * 256


def wino_pool_words(B, H, W, C):
    """vc_conv3x3_wino_pool_words: one half-word per (channel quad, pooled pixel)"""
    return B * (H // 2) * (W // 2) * (C // 8)


@functools.lru_cache(maxsize=None)
def wino2_block_shapes(limit=64):
    """{(TBH, TBW, P): smallest image (H, W) that gets it} over even H, W <= limit"""
    found = {}
    for H in range(2, limit + 1, 2):
        for W in range(2, limit + 1, 2):
            g = plan_wino2(1, H, W, 32, 32)
            if g is None:
                continue
            key = (g["TBH"], g["TBW"], g["P"])
            if key not in found or H * W < found[key][0] * found[key][1]:
                found[key] = (H, W)
    return found


def _w2_shape_cases():
    """one case per block shape: the image of exactly one block, five images = one full workgroup and one with three empty blocks"""
    out = []
    for (tbh, tbw, p), first in sorted(wino2_block_shapes().items()):
        g = plan_wino2(5, 2 * tbh, 2 * tbw, 32, 32)
        H, W = (2 * tbh, 2 * tbw) if g is not None and (g["TBH"], g["TBW"], g["P"]) == (tbh, tbw, p) else first
        out.append(((5, H, W, 32, 32), (tbh, tbw, p), "block%dx%d-pitch%d" % (tbh, tbw, p)))
    return out


W2_SHAPE_CASES = _w2_shape_cases()                  # (case, (TBH, TBW, P), id)
# (case, ragged directions, blocks % 4, id)
W2_RAGGED_CASES = [
    ((1, 34, 34, 32, 64), "xy", 0, "ragged-xy-24blocks-34x34"),
    ((3, 10, 10, 16, 32), "x", 2, "ragged-x-blocks%4=2-10x10"),
    ((1, 18, 18, 48, 96), "y", None, "ragged-y-3coltiles-3chunks-18x18"),
]
W2_LONG_CASE = (1, 6, 10, 512, 32)                  # 32 chunks of sixteen gathered channels: the longest reduction (random kind)
W2_REFUSED = [(1, 24, 2, 32, 32), (1, 24, 4, 32, 32), (1, 7, 8, 32, 32), (1, 8, 7, 32, 32)]   # no block fits 100 patch pixels; odd H; odd W


# ================================================================================================ F(4x4,3x3): csrc/conv_wino4.hip
def plan_wino4(B, H, W, C, N):
    """plan_wino4 + the workgroup order of wino4_launch -> dict or None"""
    if B <= 0 or H < 4 or W < 4 or C <= 0 or N <= 0 or C % 8 or N % 32:
        return None
    if B * H * W * max(C, N) * 4 > LAUNCH_BYTES or 36 * C * N * 4 > LAUNCH_BYTES:
        return None
    g = dict(B=B, H=H, W=W, C=C, N=N, bx_n=cdiv(W, 16), by_n=cdiv(H, 16))
    g["blocks_img"] = g["bx_n"] * g["by_n"]
    g["square_blocks"] = B * g["blocks_img"]
    if g["square_blocks"] > 0x3fffffff or g["square_blocks"] * g["blocks_img"] >= 1 << 32:
        return None
    g["th"], g["tw"] = cdiv(H, 4), cdiv(W, 4)
    g["tiles_img"] = g["th"] * g["tw"]
    g["ntiles_all"] = B * g["tiles_img"]
    g["linear_blocks"] = cdiv(g["ntiles_all"], 16)
    g["lt"] = 1 if g["ntiles_all"] < 0x7ffffff0 and g["linear_blocks"] < g["square_blocks"] else 0
    g["nblocks"] = g["linear_blocks"] if g["lt"] else g["square_blocks"]
    return _wino4_order(g)


def _wino4_order(g):
    g["tiles_n"] = g["N"] // 32
    g["pairs"] = cdiv(g["nblocks"], 2)                  # two blocks per workgroup
    g["tg"] = 4 if g["tiles_n"] % 4 == 0 else g["tiles_n"]
    g["per_chunk"] = g["pairs"] * g["tg"]
    g["chunks_n"] = g["tiles_n"] // g["tg"]
    g["workgroups"] = g["pairs"] * g["tiles_n"]
    return g


def plan_wino4v(B, H, W, C, N):
    g = plan_wino4(B, H, W, C, N)
    if g is None or not (g["lt"] or (g["tw"] == 4 and g["th"] == 4)):
        return None
    g["lt"], g["nblocks"] = 1, g["linear_blocks"]
    if g["nblocks"] * C * 2304 > LAUNCH_BYTES:
        return None
    return _wino4_order(g)


def wino4_mask_words(B, H, W, C):
    """vc_conv3x3_wino4_mask_words: 512 words per workgroup of the SQUARE-block count (never less than the linear one)"""
    g = plan_wino4(B, H, W, 8, C)
    return 0 if g is None else cdiv(g["square_blocks"], 2) * (C // 32) * 512


def wino4v_workspace_bytes(B, H, W, C):
    """vc_conv3x3_wino4v_workspace_bytes: 36 positions x 16 tiles x 4 bytes per block and gathered channel"""
    g = plan_wino4v(B, H, W, C, 32)
    return 0 if g is None else g["nblocks"] * C * 2304


# (case, lt, id): odd and tiny sizes at Cin = Cout = 32
W4_ODD_CASES = [
    ((1, 4, 4, 32, 32), 0, "square-one-tile-4x4"),
    ((1, 5, 7, 32, 32), 0, "square-odd-5x7"),
    ((1, 16, 17, 32, 32), 0, "square-one-pixel-into-a-second-block-16x17"),
    ((1, 9, 21, 32, 32), 0, "square-odd-9x21"),
    ((1, 33, 15, 32, 32), 0, "square-odd-33x15"),
    ((3, 5, 7, 32, 32), 1, "linear-odd-5x7"),
    ((3, 7, 9, 32, 32), 1, "linear-odd-7x9"),
    ((2, 17, 17, 32, 32), 1, "linear-odd-17x17"),
    ((1, 31, 33, 32, 32), 1, "linear-odd-31x33"),
    ((1, 4, 64, 32, 32), None, "strip-4x64"),
    ((1, 64, 4, 32, 32), None, "strip-64x4"),
    ((3, 5, 7, 8, 32), 1, "shortest-reduction-cin8-odd-5x7"),
]
# (case, channel tiles, tg, chunks, id): three square blocks = a ragged block pair; the forward's channel tiles are Cout / 32
W4_ORDER_CASES = [
    ((3, 16, 16, 8, 256), 8, 4, 2, "order-8tiles-two-chunks"),
    ((3, 16, 16, 8, 160), 5, 5, 1, "order-5tiles-unchunked"),
    ((3, 16, 16, 8, 96), 3, 3, 1, "order-3tiles-unchunked"),
]
W4_ORDER_DGRAD_CASE = (3, 16, 16, 256, 8)           # the data gradient produces Cin = 256 channels: eight tiles, two chunks


# ================================================================================================ F(3x3,2x2): csrc/conv_wino_wgrad.hip
WG_SHAPES = ((4, 8), (4, 7), (2, 14))


def plan_wino_wgrad(B, H, W, C, N):
    """plan_wino_wgrad -> dict or None: block shape, K splits (`cps` blocks per split, `last` blocks in the last one)"""
    if B <= 0 or H < 4 or W < 2 or (H & 1) or (W & 1) or C <= 0 or N <= 0 or C % 64 or N % 64:
        return None
    if B * H * W * max(C, N) * 4 > LAUNCH_BYTES:
        return None
    TW, TH = W // 2, H // 2
    best, shape = 0.0, 0
    for k, (tbh, tbw) in enumerate(WG_SHAPES):
        eff = float(TW * TH) / (float(cdiv(TW, tbw)) * cdiv(TH, tbh) * tbh * tbw)
        if eff > best + 1e-9:
            best, shape = eff, k
    tbh, tbw = WG_SHAPES[shape]
    p = dict(B=B, H=H, W=W, C=C, N=N, TW=TW, TH=TH, shape=shape, TBH=tbh, TBW=tbw, bx_n=cdiv(TW, tbw), by_n=cdiv(TH, tbh))
    p["blocks_img"] = p["bx_n"] * p["by_n"]
    p["nblocks"] = B * p["blocks_img"]
    if p["nblocks"] > 0x3fffffff:
        return None
    p["ncb"], p["nnb"] = C // 64, N // 64
    p["ns"] = min(cdiv(256, p["ncb"] * p["nnb"]), p["nblocks"])
    p["cps"] = cdiv(p["nblocks"], p["ns"])
    p["nsplit"] = cdiv(p["nblocks"], p["cps"])
    p["last"] = p["nblocks"] - (p["nsplit"] - 1) * p["cps"]
    return p


def wino_wgrad_workspace_bytes(B, H, W, C, N):
    """vc_conv3x3_wino_wgrad_workspace_bytes (one launch): [split][16][C][N] position sums, then [split][N] bias partials"""
    p = plan_wino_wgrad(B, H, W, C, N)
    return 0 if p is None else (p["nsplit"] * 16 * C * N + p["nsplit"] * N) * 4


def wgrad_block_region(p, blk):
    """(image, row slice, column slice) of the dy pixels of block `blk` (clipped to the image)"""
    b, rem = divmod(blk, p["blocks_img"])
    by, bx = divmod(rem, p["bx_n"])
    return b, slice(by * 2 * p["TBH"], min((by + 1) * 2 * p["TBH"], p["H"])), slice(bx * 2 * p["TBW"], min((bx + 1) * 2 * p["TBW"], p["W"]))


# (case, expected plan values, id).  "ragged": directions in which the image is no multiple of the block
WG_CASES = [
    ((17, 4, 4, 256, 256), dict(ns=16, cps=2, nsplit=9, last=1), "split-cps2-last1"),
    ((40, 4, 4, 256, 256), dict(ns=16, cps=3, nsplit=14, last=1), "split-cps3-last1"),
    ((2, 4, 4, 1024, 1024), dict(ns=1, cps=2, nsplit=1, last=2), "split-ns1-one-split-walks-both-blocks"),
    ((1, 4, 2, 64, 64), dict(shape=1, nblocks=1, nsplit=1), "block4x7-one-block-smaller-than-its-shape"),
    ((2, 20, 60, 64, 64), dict(shape=0, ragged="xy"), "block4x8-ragged-xy"),
    ((3, 20, 12, 64, 128), dict(shape=1, ragged="xy"), "block4x7-ragged-xy"),
    ((5, 12, 20, 64, 64), dict(shape=2, ragged="x"), "block2x14-ragged-x"),
]


def ragged(g):
    """directions in which the tile grid of plan `g` (F(2x2,3x3) or weight gradient) is no multiple of its block"""
    return ("x" if g["TW"] % g["TBW"] else "") + ("y" if g["TH"] % g["TBH"] else "")


def case_id(c):
    return "x".join(map(str, c))


# ================================================================================================ inputs and oracle values
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ro(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _nonzero(rng, shape, kind):
    a = V.ints(rng, -3, 3, shape) if kind == "exact" else rng.standard_normal(shape, dtype=f32)
    a[a == 0] = 1.0
    return a


@functools.lru_cache(maxsize=None)
def conv_inputs(case, kind):
    """forward / data gradient of layer (Cin -> Cout) and the data gradient of a NEXT layer (Cout -> Cin) that reads this layer's ReLU
    mask.  -> dict of read-only float32 arrays: x [B,H,W,Ci] post-ReLU, w [3,3,Ci,Co], b [Co], dy [B,H,W,Co], w2 [3,3,Co,Ci],
    dy2 [B,H,W,Ci], dyp [B,H/2,W/2,Co] (no zero: the pooled gradient).  "exact": weights are multiples of 4 that favour positive values"""
    B, H, W, Ci, Co = case
    rng = _rng("wino", case, kind)
    if kind == "exact":
        d = dict(x=V.ints(rng, 0, 7, (B, H, W, Ci)), w=4 * V.skewed_ints(rng, -3, 3, (3, 3, Ci, Co)), b=V.ints(rng, -5, 5, Co),
                 dy=V.ints(rng, -3, 3, (B, H, W, Co)), w2=4 * V.skewed_ints(rng, -3, 3, (3, 3, Co, Ci)), dy2=V.ints(rng, -3, 3, (B, H, W, Ci)))
    else:
        d = dict(x=np.maximum(rng.standard_normal((B, H, W, Ci), dtype=f32), 0),
                 w=rng.standard_normal((3, 3, Ci, Co), dtype=f32) * f32(1 / np.sqrt(9 * Ci)), b=rng.standard_normal(Co, dtype=f32),
                 dy=rng.standard_normal((B, H, W, Co), dtype=f32),
                 w2=rng.standard_normal((3, 3, Co, Ci), dtype=f32) * f32(1 / np.sqrt(9 * Co)), dy2=rng.standard_normal((B, H, W, Ci), dtype=f32))
    d["dyp"] = _nonzero(rng, (B, H // 2, W // 2, Co), kind)
    return _ro(d)


def oracle_dgrad(w, dy):
    """float64 data gradient of a layer with HWIO weights w [3,3,Ci,Co] for dy [B,H,W,Co] -> [B,H,W,Ci]"""
    B, H, W, _ = dy.shape
    return OV.conv3x3_bwd(np.zeros((B, H, W, w.shape[2])), w.astype(f64), dy.astype(f64), need_dx=True)[0]


@functools.lru_cache(maxsize=None)
def conv_ref(case, kind):
    """float64: pre (conv + b), pre0 (conv), dx (data gradient of dy, no mask), dx2 (data gradient of the next layer, no mask)"""
    d = conv_inputs(case, kind)
    pre0 = OV.conv3x3_fwd(d["x"].astype(f64), d["w"].astype(f64), np.zeros(d["w"].shape[3]))
    return _ro(dict(pre=pre0 + d["b"].astype(f64), pre0=pre0, dx=oracle_dgrad(d["w"], d["dy"]), dx2=oracle_dgrad(d["w2"], d["dy2"])))


def pool_ref(pre, dyp):
    """oracle of the fused pool behind the ReLU of pre-activation `pre`: (ypool, MaxPoolGrad(dyp) with ReluGrad)"""
    act = np.maximum(pre, 0)
    y, arg = OV.maxpool_fwd(act)
    return y, OV.maxpool_bwd(dyp.astype(f64) * (y > 0), arg, act.shape)


def ambiguous_windows(pre, tolabs):
    """[B, H/2, W/2, C] bool: pooling windows whose routing a rounding error of `tolabs` can change -- the two largest pre-activations
    closer than 2 tolabs with the maximum positive, or a maximum within tolabs of zero (the valid bit).  tolabs = 0: none (exact ties go to
    the first maximum in row-major order, in the kernel as in the oracle)"""
    B, H, W, C = pre.shape
    win = np.sort(pre.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4), axis=-1)
    top, second = win[..., 3], win[..., 2]
    return ((top - second < 2 * tolabs) & (top > -tolabs)) | (np.abs(top) < tolabs)


@functools.lru_cache(maxsize=2)
def wgrad_inputs(case, kind):
    """-> dict: x [B,H,W,Ci] post-ReLU, dy [B,H,W,Co], dw0 [3,3,Ci,Co], db0 [Co] (what accumulate = 1 adds to)"""
    B, H, W, Ci, Co = case
    rng = _rng("wino wgrad", case, kind)
    if kind == "exact":
        d = dict(x=V.ints(rng, 0, 7, (B, H, W, Ci)), dy=V.ints(rng, -3, 3, (B, H, W, Co)), dw0=V.ints(rng, -3, 3, (3, 3, Ci, Co)),
                 db0=V.ints(rng, -3, 3, Co))
    else:
        d = dict(x=np.maximum(rng.standard_normal((B, H, W, Ci), dtype=f32), 0), dy=rng.standard_normal((B, H, W, Co), dtype=f32),
                 dw0=rng.standard_normal((3, 3, Ci, Co), dtype=f32), db0=rng.standard_normal(Co, dtype=f32))
    return _ro(d)


def oracle_wgrad(x, dy):
    """float64 (dw, db)"""
    _, dw, db = OV.conv3x3_bwd(x.astype(f64), np.zeros((3, 3, x.shape[3], dy.shape[3])), dy.astype(f64), need_dx=False)
    return dw, db


@functools.lru_cache(maxsize=2)
def wgrad_ref(case, kind):
    d = wgrad_inputs(case, kind)
    dw, db = oracle_wgrad(d["x"], d["dy"])
    return _ro(dict(dw=dw, db=db))


# ================================================================================================ exactness in the transformed domain
def exact_bound_fwd(C, d, g, addend=None):
    """F(2x2,3x3), forward (d = x, g = w, addend = bias) or data gradient (d = dy): |B^T d B| <= 4 max|d| (a row of B^T has two entries
    +-1), |G g G^T| <= 2.25 max|g| (a row of G sums to at most 3/2 in magnitude), a position product sums C of those, A^T M A adds nine
    position products per output (rows of A^T have three entries +-1), the bias rides in one of them"""
    return 9 * C * (4 * V.amax(d)) * (2.25 * V.amax(g)) + V.amax(addend)


def weights_transform_to_integers(g):
    """G g G^T holds quarters of sums of the taps: integer whenever every tap is a multiple of 4"""
    return bool(np.array_equal(g, 4 * np.rint(g / 4)))


def exact_bound_wgrad(ntiles, x, dy, addend=None):
    """F(3x3,2x2): |B^T d B| <= 4 max|x|, |G' e G'^T| <= 4 max|dy| (rows of G' have at most two entries 1), a position sum S runs over all
    tiles of all images (in K splits, summed in any order).  The output transform A'^T S A' halves twice: its intermediate values are
    QUARTERS of integers of magnitude <= 4 max|S| (rows of A'^T sum to at most 2), exact in fp32 while 16 max|S| < 2**24 -- the factor 16
    makes this bound stricter than max|S| < 2**24 alone.  addend: what accumulate = 1 adds to (integers)"""
    return 16 * (ntiles * (4 * V.amax(x)) * (4 * V.amax(dy))) + V.amax(addend)


# ================================================================================================ comparison helpers (host arrays)
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def sentinel_of(dtype):
    return np.full(GUARD, SENTINEL if np.dtype(dtype) == np.dtype(f32) else SENTINEL_WORD, dtype)


def with_guard(a):
    """`a` (flattened, float32 or uint32) followed by GUARD sentinel elements"""
    a = np.ascontiguousarray(a).ravel()
    return np.concatenate([a, sentinel_of(a.dtype)])


def poison(n, dtype=f32):
    """what an output, mask / code buffer or workspace of n elements enters as: NaN (all-ones words for integer buffers) + the guard band"""
    return with_guard(np.full(int(n), NAN if np.dtype(dtype) == np.dtype(f32) else ONES_WORD, dtype))


def with_nan_tail(a):
    """an INPUT: `a` (flattened) followed by GUARD NaN -- a read past the logical end poisons the result"""
    return np.concatenate([np.ascontiguousarray(a, f32).ravel(), np.full(GUARD, NAN, f32)])


def raw(h, n, what):
    """logical part of a downloaded buffer after checking its guard band bit for bit"""
    h = np.asarray(h).ravel()
    assert h.size == n + GUARD, "%s: %d elements, expected %d + guard" % (what, h.size, n)
    assert np.array_equal(bits(h[n:]), bits(sentinel_of(h.dtype))), "%s: guard band overwritten" % what
    return h[:n]


def logical(h, n, what):
    """raw() + every element written (float buffers enter as NaN)"""
    out = raw(h, n, what)
    bad = np.isnan(out)
    assert not bad.any(), "%s: %d of %d elements unwritten or NaN (first at %d)" % (what, int(bad.sum()), n, int(np.argmax(bad)))
    return out


def untouched(h, n, what):
    out = raw(h, n, what)
    if out.dtype == np.dtype(f32):
        assert np.isnan(out).all(), "%s: written although the call was refused or the buffer not asked for" % what
    else:
        assert (out == ONES_WORD).all(), "%s: written although the call was refused or the buffer not asked for" % what


def compare(got, ref, kind, tol, what, close=None, scale=None):
    """exact inputs: equality with the float64 oracle; random inputs: close(got, ref, tol) = tests/gpu_util.py assert_close"""
    got = np.asarray(got).reshape(np.shape(ref))
    if kind == "exact":
        np.testing.assert_array_equal(got, ref, err_msg=what)
    else:
        close(got, ref, tol, atol_scale=scale, msg=what)


def compare_routing(got, pre, dyp, tolabs, what):
    """got [B,H,W,C]: the pooled gradient dyp routed by the kernel's codes; must EQUAL the oracle's MaxPoolGrad (with ReluGrad) of the
    oracle activation relu(pre) in every window that a rounding error of tolabs cannot re-route (all of them when tolabs = 0)"""
    _, ref = pool_ref(pre, dyp)
    amb = ambiguous_windows(pre, tolabs)
    assert amb.mean() < 0.01, "%s: %d of %d windows ambiguous" % (what, int(amb.sum()), amb.size)
    keep = ~np.repeat(np.repeat(amb, 2, axis=1), 2, axis=2)
    got = np.asarray(got).reshape(ref.shape)
    np.testing.assert_array_equal(got[keep], ref[keep], err_msg=what)
