"""Cases, inputs, planner transcription and expected values of tests/test_gpu_gemm_edges.py and tests/test_gemm_edges_host.py: numpy only
(no GPU, no library call), so that the CPU test can check every property the GPU test relies on.

  * `plan_gemm`, `plan_bx256`, `expected_workspace_bytes`: csrc/gemm.hip's planners, line by line.  tests/test_gemm_edges_host.py pins
    them to the built library through vc_gemm_workspace_bytes; `plan_for` is what gemm_impl launches for a precision.
  * CASES: one row per edge of the dispatch, each with the plan it is meant to reach IN BOTH PRECISIONS (asserted on the host).
  * two kinds of input:
      "exact"   small integers stored as float32 -- A in [-4, 4], B in [-3, 3], bias and C0 in [-5, 5].  While
                K * max|A| * max|B| + max|bias| + max|C0| < 2**24 (`is_exact`, from the actual arrays) every product and every partial
                sum, in whatever order and however split, is an integer below 2**24: f32 FMA is exact, and so is the split-bf16 product
                (an integer of magnitude <= 256 is a bf16 value: hi = a, lo = 0).  The result must EQUAL the float64 reference: a k that
                is dropped or counted twice at a split or shift boundary fails at any K.
      "random"  standard normal, for the project's rounding tolerances.
  * dresses: how an operand sits in its allocation (`DRESSES`, `dress_geometry`, `embed`)."""
import collections
import functools
import zlib

import numpy as np

f32 = np.float32
f64 = np.float64
KINDS = ("exact", "random")
PRECS = ("f32", "bf16x3")
ORDERS = ((0, 0), (0, 1), (1, 0), (1, 1))      # (ta, tb)
EXACT_LIMIT = 2 ** 24
RELU, ACCUMULATE, BF16X3 = 1, 2, 4             # include/vaecap.h VC_GEMM_*
GUARD = 64                                     # floats after every buffer
SENTINEL = f32(-24680.5)
NAN = f32(np.nan)
REDUCE_CAP = 2048 * 256                        # splitk_reduce_kernel: at most 2048 blocks of 256 threads, one element per thread and sweep
REDUCE4_CAP = 4096 * 256                       # splitk_reduce4_kernel: at most 4096 blocks, one float4 per thread and sweep
BX_GROUP = 8                                   # gemm_body, PREC == 1: tile rows per group of the grouped order


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ csrc/gemm.hip, transcribed
GemmPlan = collections.namedtuple("GemmPlan", "big skinny splits kchunk tiles_m tiles_n main_m tail_splits tail_kchunk")
BxPlan = collections.namedtuple("BxPlan", "use tiles_m tiles_n splits kchunk")
Plan = collections.namedtuple("Plan", "tile splits kchunk tail_splits bx")   # what a test row names; tile: "64", "128", "skinny", "256"


def plan_gemm(M, N, K):
    if M <= 64 and N >= 256 and K >= 512:
        tiles_n = cdiv(N, 128)
        sa = min(768 // tiles_n, K // 256, 64)
        sa = max(sa, 1)
        kchunk = cdiv(cdiv(K, sa), 32) * 32
        return GemmPlan(False, True, cdiv(K, kchunk), kchunk, 1, tiles_n, 1, 1, 0)
    t128 = cdiv(M, 128) * cdiv(N, 128)
    sa = 1
    if t128 <= 128:
        sa = max(min(768 // t128, K // 512, 64), 1)
    elif t128 < 768:
        sa = max(min((1200 + t128 // 2) // t128, K // 640), 1)
    big = t128 >= 384 or (t128 <= 128 and t128 * sa >= 256) or (t128 > 128 and sa > 1)
    b = 128 if big else 64
    tiles_m, tiles_n = cdiv(M, b), cdiv(N, b)
    tiles = tiles_m * tiles_n
    splits = sa
    if not big:
        splits = 1
        if tiles < 192:
            splits = max(min((512 + tiles - 1) // tiles, K // 256, 64), 1)
    kchunk = max(cdiv(cdiv(K, splits), 32) * 32, 32)
    splits = max(cdiv(K, kchunk), 1)
    main_m, tail_splits, tail_kchunk = tiles_m, 1, 0
    if big and splits == 1:
        slots = 768
        full = (tiles // slots) * slots
        if 0 < full < tiles:
            mm = full // tiles_n
            tail = tiles - mm * tiles_n
            ktiles = cdiv(K, 32)
            S = min(slots // tail, ktiles // 16, 32)
            if S >= 2:
                tail_kchunk = cdiv(ktiles, S) * 32
                tail_splits = cdiv(K, tail_kchunk)
                main_m = mm
    return GemmPlan(big, False, splits, kchunk, tiles_m, tiles_n, main_m, tail_splits, tail_kchunk)


def plan_bx256(M, N, K):
    if M < 192 or N < 192:
        return BxPlan(False, 0, 0, 0, 0)
    tiles_m, tiles_n = cdiv(M, 256), cdiv(N, 256)
    t = tiles_m * tiles_n
    best, beff = 1, 0.0
    maxs = min(max(K // 1024, 1), 16)
    for s in range(1, maxs + 1):
        w = t * s
        eff = w / float(cdiv(w, 256) * 256) - 0.02 * (s - 1)
        if eff > beff + 1e-9:
            beff, best = eff, s
    if t * best < 200:
        return BxPlan(False, tiles_m, tiles_n, 0, 0)
    kchunk = max(cdiv(cdiv(K, best), 32) * 32, 32)
    return BxPlan(True, tiles_m, tiles_n, max(cdiv(K, kchunk), 1), kchunk)


def expected_workspace_bytes(M, N, K):
    """vc_gemm_workspace_bytes: the larger of what the two precisions need"""
    p, b = plan_gemm(M, N, K), plan_bx256(M, N, K)
    f = 0
    if p.splits > 1:
        f = p.splits * M * N * 4
    elif p.tail_splits > 1:
        f = p.tail_splits * (M - p.main_m * 128) * N * 4
    bx = b.splits * M * N * 4 if b.use and b.splits > 1 else 0
    return max(f, bx)


def plan_for(M, N, K, prec):
    """what gemm_impl launches for `prec` when it is given the whole workspace"""
    if prec == "bf16x3":
        b = plan_bx256(M, N, K)
        if b.use:
            return Plan("256", b.splits, b.kchunk, 1, True)
    p = plan_gemm(M, N, K)
    return Plan("skinny" if p.skinny else "128" if p.big else "64", p.splits, p.kchunk, p.tail_splits, False)


def last_split_k(M, N, K, prec):
    """length of the last split's K range"""
    p = plan_for(M, N, K, prec)
    return K - (p.splits - 1) * p.kchunk


def tail_last_split_k(M, N, K):
    p = plan_gemm(M, N, K)
    return K - (p.tail_splits - 1) * p.tail_kchunk if p.tail_splits > 1 else None


def vec_in(M, N, K, ta, tb):
    """gemm_impl's `vec` for contiguous operands on allocation boundaries: the aligned (VEC) loaders"""
    return (M if ta else K) % 4 == 0 and (K if tb else N) % 4 == 0


# ------------------------------------------------------------------------------------------------ the case table
# (M, N, K) -> (plan in f32, plan in bf16x3), each (tile, splits, kchunk, tail splits, bx); tests/test_gemm_edges_host.py asserts every
# row against the transcription above and the coverage list against the rows.
def _row(shape, f, b, note):
    return shape, Plan(*f), Plan(*b), note


CASE_ROWS = [
    # ---- skinny boundary: M <= 64 && N >= 256 && K >= 512, and one step outside on each axis
    _row((64, 256, 512), ("skinny", 2, 256, 1, False), ("skinny", 2, 256, 1, False), "on the boundary"),
    _row((1, 256, 512), ("skinny", 2, 256, 1, False), ("skinny", 2, 256, 1, False), "one row"),
    _row((65, 256, 512), ("64", 2, 256, 1, False), ("64", 2, 256, 1, False), "M one past"),
    _row((64, 255, 512), ("64", 2, 256, 1, False), ("64", 2, 256, 1, False), "N one short"),
    _row((64, 256, 511), ("64", 1, 512, 1, False), ("64", 1, 512, 1, False), "K one short: K // 256 == 1, no split"),
    _row((61, 390, 1100), ("skinny", 4, 288, 1, False), ("skinny", 4, 288, 1, False), "ragged N and K"),
    _row((64, 256, 1101), ("skinny", 4, 288, 1, False), ("skinny", 4, 288, 1, False), "K % 4 != 0: the row-contiguous order keeps the aligned loaders, shift 19"),
    _row((64, 1027, 8200), ("skinny", 29, 288, 1, False), ("skinny", 29, 288, 1, False), "9 column tiles, the last of 3 columns"),
    # ---- 64 x 64: one K tile, K just around 32
    _row((1, 1, 1), ("64", 1, 32, 1, False), ("64", 1, 32, 1, False), "one element"),
    _row((3, 5, 31), ("64", 1, 32, 1, False), ("64", 1, 32, 1, False), "K < 32"),
    _row((4, 8, 32), ("64", 1, 32, 1, False), ("64", 1, 32, 1, False), "K == 32, aligned: the shift is 0"),
    _row((63, 65, 33), ("64", 1, 64, 1, False), ("64", 1, 64, 1, False), "second K tile of one k"),
    _row((129, 131, 37), ("64", 1, 64, 1, False), ("64", 1, 64, 1, False), "3 x 3 tiles, everything ragged"),
    _row((520, 530, 2600), ("64", 7, 384, 1, False), ("64", 7, 384, 1, False), "N % 4 != 0: scalar reduce"),
    _row((513, 515, 2100), ("64", 7, 320, 1, False), ("64", 7, 320, 1, False), "scalar reduce, ragged"),
    _row((1000, 530, 2600), ("64", 4, 672, 1, False), ("64", 4, 672, 1, False), "M N = 530000: scalar reduce past its 2048-block cap"),
    _row((260, 264, 2100), ("64", 8, 288, 1, False), ("64", 8, 288, 1, False), "aligned 64 x 64 split: float4 reduce (dress case)"),
    # ---- 128 x 128 with global split-K
    _row((3200, 512, 5000), ("128", 7, 736, 1, False), ("128", 7, 736, 1, False), "one whole round through split-K"),
    _row((2052, 2300, 2080), ("128", 3, 704, 1, False), ("128", 3, 704, 1, False), "M N / 4 = 1179900: float4 reduce past its 4096-block cap"),
    _row((2049, 2303, 2081), ("128", 3, 704, 1, False), ("128", 3, 704, 1, False), "fully ragged: scalar reduce past its cap"),
    # ---- the whole-rounds tail launch
    _row((3584, 3584, 1024), ("128", 1, 1024, 2, False), ("128", 1, 1024, 2, False), "27 tile rows + tail of 1 x 2 splits; 196 bx tiles < 200"),
    _row((3500, 3580, 1060), ("128", 1, 1088, 2, False), ("128", 1, 1088, 2, False), "the same, ragged: the tail's second split has 516"),
    _row((12300, 1028, 1060), ("128", 1, 1088, 2, False), ("256", 1, 1088, 1, True), "f32: tail after 85 rows; bx: 49 x 5 tiles, last group of one row"),
    # ---- 256 x 256 (split-bf16 only)
    _row((3700, 3500, 40), ("128", 1, 64, 1, False), ("256", 1, 64, 1, True), "15 x 14 tiles, two K tiles, the second shifted by 24"),
    _row((3588, 3332, 100), ("128", 1, 128, 1, False), ("256", 1, 128, 1, True), "four K tiles, the last shifted by 28"),
    _row((3332, 3600, 32), ("128", 1, 32, 1, False), ("256", 1, 32, 1, True), "one K tile on the aligned loaders: the loop never reaches its second LDS image"),
    _row((3330, 3601, 31), ("128", 1, 32, 1, False), ("256", 1, 32, 1, True), "K < 32: guarded loaders"),
    _row((3601, 3331, 33), ("128", 1, 64, 1, False), ("256", 1, 64, 1, True), "K = 33, odd M and N: guarded in every order"),
    _row((3600, 3332, 33), ("128", 1, 64, 1, False), ("256", 1, 64, 1, True), "K = 33: shift 31 in the row-contiguous order (ta = 1, tb = 0), guarded in the others"),
    _row((900, 900, 13312), ("128", 12, 1120, 1, False), ("256", 13, 1024, 1, True), "4 x 4 tiles, 13 splits of exactly 1024"),
    _row((772, 1020, 13400), ("128", 13, 1056, 1, False), ("256", 13, 1056, 1, True), "last split 728 = 22 tiles + 24: shifted, aligned"),
    _row((769, 1021, 13401), ("128", 13, 1056, 1, False), ("256", 13, 1056, 1, True), "the same, guarded"),
    # ---- a shifted K tile that is the whole last split (K - (splits - 1) * kchunk = 4, aligned: the split-bf16 loaders read [K - 32, K)
    # and zero the first 28 k).  The 256 x 256 plan cannot have one: its splits are >= 1024 long and at most 16, and a last split under
    # 32 needs kchunk <= 32 * splits.
    _row((64, 256, 2308), ("skinny", 9, 288, 1, False), ("skinny", 9, 288, 1, False), "last split of 4 k"),
    _row((260, 264, 2308), ("64", 9, 288, 1, False), ("64", 9, 288, 1, False), "last split of 4 k"),
    _row((260, 264, 15236), ("128", 29, 544, 1, False), ("128", 29, 544, 1, False), "last split of 4 k"),
    # ---- K == 0 (run by the K = 0 test only)
    _row((70, 96, 0), ("64", 1, 32, 1, False), ("64", 1, 32, 1, False), "K == 0"),
    _row((64, 300, 0), ("64", 1, 32, 1, False), ("64", 1, 32, 1, False), "K == 0, M <= 64 && N >= 256"),
    _row((300, 300, 0), ("64", 1, 32, 1, False), ("64", 1, 32, 1, False), "K == 0, M, N >= 192"),
    _row((3601, 3331, 0), ("128", 1, 32, 1, False), ("256", 1, 32, 1, True), "K == 0 on the 128 x 128 and 256 x 256 tiles (210 bx tiles)"),
]
CASES = [r[0] for r in CASE_ROWS if r[0][2] > 0]
K0_CASES = [r[0] for r in CASE_ROWS if r[0][2] == 0]
CASE_PLANS = {r[0]: {"f32": r[1], "bf16x3": r[2]} for r in CASE_ROWS}
CASE_INDEX = {c: i for i, c in enumerate(CASES)}

# the other three dresses: one split case per tile configuration and precision, N % 4 == 0 (so that the dress alone moves the call from the
# float4 reduce to the scalar one)
DRESS_CASES = {
    "f32": [(260, 264, 2100), (3200, 512, 5000), (64, 256, 512), (3584, 3584, 1024)],
    "bf16x3": [(260, 264, 2100), (3200, 512, 5000), (64, 256, 512), (772, 1020, 13400)],
}
DETERMINISM_CASES = [(520, 530, 2600), (3200, 512, 5000), (3584, 3584, 1024)]   # scalar reduce, float4 reduce, tail launch


def case_id(c):
    return "x".join(map(str, c))


def flags_of(case, ta, tb):
    """round-robin by case index, advanced by the storage order: every case meets every flag combination in some order"""
    return (CASE_INDEX[case] + 2 * ta + tb) % 4


def with_bias(case, ta, tb):
    """both with and without a bias for every case (tb = 0 / 1 swap with the case index)"""
    return (CASE_INDEX[case] + tb) % 2 == 0


# ------------------------------------------------------------------------------------------------ inputs and references
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(f32)


@functools.lru_cache(maxsize=4)
def inputs(case, kind):
    """-> A [M, K], B [K, N], bias [N], C0 [M, N]: float32, read-only"""
    M, N, K = case
    rng = _rng("gemm", case, kind)
    if kind == "exact":
        A, B = ints(rng, -4, 4, (M, K)), ints(rng, -3, 3, (K, N))
        bias, C0 = ints(rng, -5, 5, N), ints(rng, -5, 5, (M, N))
    else:
        A, B = rng.standard_normal((M, K), dtype=f32), rng.standard_normal((K, N), dtype=f32)
        bias, C0 = rng.standard_normal(N, dtype=f32), rng.standard_normal((M, N), dtype=f32)
    return _ro(A, B, bias, C0)


def amax(a):
    return float(np.abs(a).max()) if a.size else 0.0


def exact_bound(case, kind="exact"):
    A, B, bias, C0 = inputs(case, kind)
    return case[2] * amax(A) * amax(B) + amax(bias) + amax(C0)


def is_exact(case, kind="exact"):
    return exact_bound(case, kind) < EXACT_LIMIT


@functools.lru_cache(maxsize=4)
def product(case, kind):
    """float64 op(A) op(B), [M, N]"""
    A, B, _, _ = inputs(case, kind)
    return _ro(A.astype(f64) @ B.astype(f64))


@functools.lru_cache(maxsize=2)
def abs_product(case, kind):
    """float64 |A| |B|: the scale of the split-bf16 error model"""
    A, B, _, _ = inputs(case, kind)
    return _ro(np.abs(A).astype(f64) @ np.abs(B).astype(f64))


def reference(case, kind, flags, bias=True):
    """float64 epilogue(product): + bias, + C0 (VC_GEMM_ACCUMULATE), ReLU (VC_GEMM_RELU)"""
    _, _, b, C0 = inputs(case, kind)
    out = product(case, kind).copy()
    if bias:
        out += b.astype(f64)
    if flags & ACCUMULATE:
        out += C0.astype(f64)
    if flags & RELU:
        np.maximum(out, 0, out=out)
    return out


def tol_f32(K):
    """tests/test_gpu_ops.py test_gemm_training_shapes: of the tensor maximum"""
    return 2e-6 * np.sqrt(K) + 2e-6


TOL_BF16X3 = 6e-5     # tests/test_gpu_bf16x3.py TOL: of the tensor maximum


def bf16x3_bound(case, kind):
    """tests/test_gpu_bf16x3.py's element-wise model of the product's error; it also bounds the error after the epilogue (adding
    the same bias / C0 to both sides changes nothing, ReLU is 1-Lipschitz)"""
    return 2.0 ** -16 * abs_product(case, kind) + 1e-6


# ------------------------------------------------------------------------------------------------ dresses
DRESSES = ("plain", "padded", "odd", "offset")
Geometry = collections.namedtuple("Geometry", "lda ldb ldc offset")


def dress_geometry(dress, M, N, K, ta, tb):
    """leading dimensions and the offset (floats) of A, B, C and bias into their allocations.
      plain    contiguous
      padded   lda = extent + 4, ldb = extent + 8, ldc = N + 4: keeps the vector paths
      odd      every leading dimension extent + 1: vector loaders and vector epilogue off by the leading dimension
      offset   contiguous, every buffer starts one float into its allocation: off by alignment alone"""
    ea, eb = (M if ta else K), (K if tb else N)
    if dress == "plain":
        return Geometry(ea, eb, N, 0)
    if dress == "padded":
        return Geometry(ea + 4, eb + 8, N + 4, 0)
    if dress == "odd":
        return Geometry(ea + 1, eb + 1, N + 1, 0)
    if dress == "offset":
        return Geometry(ea, eb, N, 1)
    raise ValueError(dress)


def embed(a, ld, offset, fill):
    """the 2-d array `a` as stored, rows `ld` apart, `offset` floats into a flat buffer that ends with GUARD floats; everything
    that is not `a` is `fill`"""
    a = np.asarray(a, f32)
    if a.ndim == 1:
        a = a[None, :]
    rows, cols = a.shape
    assert ld >= cols
    buf = np.full(offset + rows * ld + GUARD, fill, f32)
    buf[offset:offset + rows * ld].reshape(rows, ld)[:, :cols] = a
    return buf


def stored(a, transposed):
    return np.ascontiguousarray(a.T) if transposed else a


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)
