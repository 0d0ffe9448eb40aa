"""Cases, inputs and expected values of tests/test_gpu_vgg_edges.py and tests/test_vgg_edges_host.py: numpy and oracle/vgg.py only (no
GPU, no library call), so that the CPU test can check every property the GPU test relies on.

Two kinds of input for every convolution case:

  "exact"   small integers stored as float32 -- activations in [-4, 4] (post-ReLU ones in [0, 7]), weights and output gradients in
            [-3, 3], bias in [-5, 5].  While  n_terms * max|a| * max|b| (+ max|addend|) < 2**24  (`exact_bound`, computed from the actual
            arrays) every product and every partial sum, in whatever order and however split, is an integer below 2**24 in magnitude:
            fp32 FMA is then exact, and the kernel's output must EQUAL the float64 oracle's -- one missing, doubled or misplaced pixel
            fails at any tensor size.  The weights and the conv1_1 input favour positive values (`skewed_ints`), so that sums have a
            positive mean and more than half of a ReLU'd output is non-zero (test_vgg_edges_host.py asserts it).
  "random"  standard normal (ReLU'd where the kernel expects a post-ReLU tensor, weights scaled by 1/sqrt(K)), for the project's
            rounding tolerances (`tol_conv`, `tol_conv1`).
"""
import functools
import zlib

import numpy as np

from oracle import vgg as OV

f32 = np.float32
f64 = np.float64
KINDS = ("exact", "random")
EXACT_LIMIT = 2 ** 24

# ---- A. implicit-GEMM weight gradient: (B, H, W, Cin, Cout), tile configuration of csrc/conv.hip launch_wgrad, split count of plan_wgrad
WGRAD_CASES = [
    ((1, 25, 44, 4, 8), "Small", 2),            # 1100 pixels: kchunk 576, the last split has 524
    ((1, 25, 44, 4, 128), "Small, two column tiles", 2),
    ((1, 25, 44, 16, 32), "Narrow", 2),
    ((2, 10, 12, 128, 64), "Narrow, 4.5 row tiles", 1),
    ((1, 25, 44, 128, 64), "Narrow", 2),
    ((1, 29, 53, 64, 64), "W192n", 3),          # 1537 pixels: kchunk 544, the last split has 449 = 14 K-tiles + 1 pixel
    ((1, 29, 53, 64, 128), "W192w", 3),
    ((1, 25, 44, 128, 256), "Wide", 2),
    ((1, 47, 47, 512, 512), "Wide", 4),
    ((2, 256, 257, 4, 8), "Small", 242),
]
# ---- B. degenerate geometry (forward, data gradient, weight gradient); the second has 16 splits and a prime H with W = 1
GEOM_CASES = [(5, 1, 1, 4, 8), (2, 4099, 1, 4, 8), (3, 1, 67, 8, 4), (1, 2, 2, 64, 64)]
GEOM_SPLITS = {(2, 4099, 1, 4, 8): 16}
DGRAD_WS_CASE = (3, 14, 14, 512, 512)           # data gradient with the K-split tail launch (vc_conv3x3_dgrad_workspace_bytes > 0)
# ---- C. conv1_1 (csrc/conv_first.hip): (B, H, W) -> groups of 32 pixels = B * H * W / 32; the forward launches min(ceil(groups / 4),
# 2048) workgroups of four waves, a wave takes groups  first, first + 8192, ...
CONV1_FWD_CASES = [
    ((1, 1, 32), 1),         # one wave of the workgroup works; every vertical tap is outside the image
    ((1, 3, 32), 3),
    ((2, 5, 64), 20),        # the image boundary falls between the waves of a workgroup
    ((1, 512, 512), 8192),   # every wave exactly one trip
    ((3, 2731, 32), 8193),   # one wave takes a second trip
    ((3, 1821, 96), 16389),  # a third trip: the prefetch returns to slot 0
]
# the weight gradient launches parts = min(ceil(groups / 4), 1024) workgroups; the reduce kernel's eight thread groups take partials
# pg, pg + 8 in pairs (`p + 8 < parts; p += 16`) and a single leftover: (B, H, W) -> parts
CONV1_WGRAD_CASES = [
    ((1, 1, 32), 1),
    ((1, 16, 64), 8),
    ((1, 11, 96), 9),
    ((2, 16, 64), 16),
    ((5, 13, 32), 17),
    ((3, 31, 32), 24),
    ((1, 241, 544), 1024),   # 4097 groups on 4096 waves: one wave takes two groups
    ((3, 1821, 96), 1024),
]
CONV1_FWD_NAN_CASE = (2, 5, 64)      # fourth channel of x4 = NaN: include/vaecap.h says it is ignored
CONV1_WGRAD_NAN_CASE = (5, 13, 32)
# ---- D. pooling, layout and preprocessing kernels: csrc/conv.hip grid_for launches at most 4096 blocks of 256 threads, a thread takes
# items  i, i + 4096 * 256, ...: a launch of more items than this wraps
GRID_CAP_ITEMS = 4096 * 256
POOL_WRAP = (1, 260, 260, 256)       # 130 * 130 * 64 = 1 081 600 float4 items / pooled pixels of a plane
POOL_SMALL = [(1, 2, 2, 4), (3, 2, 6, 8)]
LAYOUT_WRAP = (1, 260, 260, 64)
LAYOUT_SMALL = [(1, 1, 1, 4), (3, 2, 6, 8)]
PREPROCESS_F32 = [(21, 224, 224), (1, 1, 1), (2, 3, 5)]
PREPROCESS_U8 = [(84, 224, 224), (1, 2, 2), (3, 2, 6)]          # B * H * W % 4 == 0; a thread takes four pixels
PAD_DIM = [(9, 3, 4, 30011), (9, 4, 3, 40009), (9, 3, 4, 64), (1, 1, 5, 1)]   # (outer, c_src, c_dst, inner)


def case_id(c):
    return "x".join(map(str, c))


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def skewed_ints(rng, lo, hi, shape):
    """integers of [lo, hi] as float32, each positive value twice as likely as each other value"""
    vals = np.arange(lo, hi + 1)
    p = np.where(vals > 0, 2.0, 1.0)
    return rng.choice(vals, size=shape, p=p / p.sum()).astype(f32)


def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(f32)


# ------------------------------------------------------------------------------------------------ exactness
def amax(a):
    return 0.0 if a is None else float(np.abs(a).max())


def exact_bound(n_terms, a, b, addend=None):
    """upper bound of every partial sum of  sum_{n_terms} a * b (+ addend)"""
    return n_terms * amax(a) * amax(b) + amax(addend)


def is_exact(n_terms, a, b, addend=None):
    return exact_bound(n_terms, a, b, addend) < EXACT_LIMIT


def reachable_taps(H, W):
    """[3, 3] bool: taps (ky, kx) that meet at least one pixel pair inside an H x W image (|ky - 1| < H and |kx - 1| < W); the
    weight gradient of the other taps is zero by construction"""
    ky, kx = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    return (np.abs(ky - 1) < H) & (np.abs(kx - 1) < W)


# ------------------------------------------------------------------------------------------------ tolerances of the random kind
def tol_conv(K):
    """tests/test_gpu_ops.py, csrc/conv.hip kernels: of max|ref|; K = 9 Cin (forward), 9 Cout (data gradient), B H W (weight gradient)"""
    return 2e-6 * np.sqrt(K) + 1e-6


def tol_conv1(K):
    """the same with tests/test_gpu_cfg4_geometry.py's figure for conv1_1's kernels; K = 27 (forward), B H W (weight gradient)"""
    return 3e-6 * np.sqrt(K) + 1e-6


# ------------------------------------------------------------------------------------------------ implicit-GEMM convolution
@functools.lru_cache(maxsize=None)
def conv_inputs(case, kind):
    """-> x (post-ReLU), w, b, dy, dw0, db0 (what accumulate = 1 adds to), float32, read-only"""
    B, H, W, Ci, Co = case
    rng = _rng("conv", case, kind)
    if kind == "exact":
        x = ints(rng, 0, 7, (B, H, W, Ci))
        w = skewed_ints(rng, -3, 3, (3, 3, Ci, Co))
        b = ints(rng, -5, 5, Co)
        dy = ints(rng, -3, 3, (B, H, W, Co))
        dw0 = ints(rng, -3, 3, (3, 3, Ci, Co))
        db0 = ints(rng, -3, 3, Co)
    else:
        x = np.maximum(rng.standard_normal((B, H, W, Ci), dtype=f32), 0)
        w = rng.standard_normal((3, 3, Ci, Co), dtype=f32) * f32(1 / np.sqrt(9 * Ci))
        b = rng.standard_normal(Co, dtype=f32)
        dy = rng.standard_normal((B, H, W, Co), dtype=f32)
        dw0 = rng.standard_normal((3, 3, Ci, Co), dtype=f32)
        db0 = rng.standard_normal(Co, dtype=f32)
    return _ro(x, w, b, dy, dw0, db0)


@functools.lru_cache(maxsize=None)
def conv_fwd_ref(case, kind):
    """float64 pre-activations with and without bias: (conv + b, conv)"""
    x, w, b, _, _, _ = conv_inputs(case, kind)
    y = OV.conv3x3_fwd(x.astype(f64), w.astype(f64), np.zeros(w.shape[3]))
    return _ro(y + b.astype(f64), y)


@functools.lru_cache(maxsize=None)
def conv_bwd_ref(case, kind, need_dx):
    """float64 (dx or None, dw, db)"""
    x, w, _, dy, _, _ = conv_inputs(case, kind)
    dx, dw, db = OV.conv3x3_bwd(x.astype(f64), w.astype(f64), dy.astype(f64), need_dx=need_dx)
    _ro(dw, db)
    if dx is not None:
        _ro(dx)
    return dx, dw, db


# ------------------------------------------------------------------------------------------------ conv1_1
@functools.lru_cache(maxsize=2)
def conv1_inputs(shape, kind):
    """-> x4 [B, H, W, 4] (fourth channel zero), w [3, 3, 3, 64], b, dy [B, H, W, 64] (NHWC), dw0, db0"""
    B, H, W = shape
    rng = _rng("conv1", shape, kind)
    x4 = np.zeros((B, H, W, 4), f32)
    if kind == "exact":
        x4[..., :3] = skewed_ints(rng, -4, 4, (B, H, W, 3))
        w = skewed_ints(rng, -3, 3, (3, 3, 3, 64))
        b = ints(rng, -5, 5, 64)
        dy = ints(rng, -3, 3, (B, H, W, 64))
        dw0 = ints(rng, -3, 3, (3, 3, 3, 64))
        db0 = ints(rng, -3, 3, 64)
    else:
        x4[..., :3] = rng.standard_normal((B, H, W, 3), dtype=f32)
        w = rng.standard_normal((3, 3, 3, 64), dtype=f32) * f32(1 / np.sqrt(27))
        b = rng.standard_normal(64, dtype=f32)
        dy = rng.standard_normal((B, H, W, 64), dtype=f32)
        dw0 = rng.standard_normal((3, 3, 3, 64), dtype=f32)
        db0 = rng.standard_normal(64, dtype=f32)
    return _ro(x4, w, b, dy, dw0, db0)


def conv1_fwd_ref(shape, kind):
    """float64 pre-activation conv(x4[..., :3], w) + b, NHWC"""
    x4, w, b, _, _, _ = conv1_inputs(shape, kind)
    return OV.conv3x3_fwd(x4[..., :3].astype(f64), w.astype(f64), b.astype(f64))


def conv1_wgrad_ref(shape, kind):
    """float64 (dw, db)"""
    x4, w, _, dy, _, _ = conv1_inputs(shape, kind)
    _, dw, db = OV.conv3x3_bwd(x4[..., :3].astype(f64), w.astype(f64), dy.astype(f64), need_dx=False)
    return dw, db


# ------------------------------------------------------------------------------------------------ pooling
@functools.lru_cache(maxsize=None)
def pool_inputs(shape):
    """x: standard normal, NOT ReLU'd (windows whose maximum is negative occur), with a window of zeros (tie at zero) and a positive
    pair (tie: the first in scan order wins); dy: standard normal, no zero"""
    B, H, W, C = shape
    rng = _rng("pool", shape)
    x = rng.standard_normal(shape, dtype=f32)
    x[0, 0:2, 0:2, :] = 0.0
    if W >= 4:
        x[B - 1, 0, 2, :] = x[B - 1, 1, 3, :] = 5.0      # positions 0 and 3 of the window at pooled (0, 1)
    dy = rng.standard_normal((B, H // 2, W // 2, C), dtype=f32)
    dy[dy == 0] = 1.0
    return _ro(x, dy)


@functools.lru_cache(maxsize=None)
def pool_ref(shape):
    """oracle: (y, arg, dx without ReluGrad, dx with ReluGrad = dx * (window maximum > 0))"""
    x, dy = pool_inputs(shape)
    y, arg = OV.maxpool_fwd(x)
    dx = OV.maxpool_bwd(dy, arg, x.shape)
    dxr = OV.maxpool_bwd(dy * (y > 0), arg, x.shape)
    return _ro(y, arg, dx, dxr)


def pool_codes(arg, y):
    """The routing codes vc_maxpool2x2_bwd_bits_f32 reads (csrc/conv.hip, above maxpool_bwd_bits_c4_kernel; include/vaecap.h): one
    16-bit half-word per plane b * C/4 + q, pooled row and pooled column -- layout [B][C/4][H/2][W/2] --, nibble j of it belongs to
    channel 4 q + j and holds  arg | 4 if the window's maximum is > 0  (arg = position of the first maximum, row-major).
    arg, y: the oracle's [B, H/2, W/2, C].  -> uint16 [B, C/4, H/2, W/2]"""
    B, Ho, Wo, C = arg.shape
    nib = (arg.astype(np.uint16) | np.where(y > 0, 4, 0).astype(np.uint16)).reshape(B, Ho, Wo, C // 4, 4)
    half = nib[..., 0] | (nib[..., 1] << 4) | (nib[..., 2] << 8) | (nib[..., 3] << 12)
    return np.ascontiguousarray(half.transpose(0, 3, 1, 2).astype(np.uint16))


def pool_codes_words(codes):
    """the half-words as whole little-endian 32-bit words (zero-padded), the unit of vc_conv3x3_wino_pool_words"""
    flat = codes.ravel()
    if flat.size % 2:
        flat = np.concatenate([flat, np.zeros(1, np.uint16)])
    return np.ascontiguousarray(flat).view(np.uint32)


def decode_pool_codes(codes, dy, in_shape):
    """what the codes mean, on the host: [B, C/4, H/2, W/2] half-words + dy [B, H/2, W/2, C] -> dx [B, H, W, C]"""
    B, Q, Ho, Wo = codes.shape
    nib = np.stack([(codes >> (4 * j)) & 15 for j in range(4)], axis=-1)          # [B, Q, Ho, Wo, 4]
    nib = nib.transpose(0, 2, 3, 1, 4).reshape(B, Ho, Wo, Q * 4)
    assert (nib < 8).all()
    return OV.maxpool_bwd(dy * ((nib & 4) != 0), (nib & 3).astype(np.int64), in_shape)


# ------------------------------------------------------------------------------------------------ layouts, preprocessing
def to_c4(a):
    B, H, W, C = a.shape
    return np.ascontiguousarray(a.reshape(B, H, W, C // 4, 4).transpose(0, 3, 1, 2, 4))


def preprocess_ref(img):
    """img [B, H, W, 3] (float32 or uint8 pixel values) -> [B, H, W, 4] float32: RGB - mean, fourth channel zero.  One IEEE
    subtraction of float32 values, as the kernel's: exact comparison."""
    out = np.zeros(img.shape[:3] + (4,), f32)
    out[..., :3] = img.astype(f32) - OV.MEAN_RGB
    return out


def pad_dim_ref(src, c_dst):
    """src [outer, c_src, inner] -> [outer, c_dst, inner]: zero-padded or truncated middle dimension"""
    outer, c_src, inner = src.shape
    out = np.zeros((outer, c_dst, inner), src.dtype)
    n = min(c_src, c_dst)
    out[:, :n] = src[:, :n]
    return out
