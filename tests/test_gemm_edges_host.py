"""CPU only: what tests/test_gpu_gemm_edges.py takes for granted about tests/gemm_edges_ref.py.

  * The transcription of csrc/gemm.hip's planners gives the workspace size the built library gives (vc_gemm_workspace_bytes needs no
    device), for every case of the table and for a seeded sweep over the planners' thresholds.  The query returns
    max(f32 need, split-bf16 need), each `splits * M * N * 4` or `tail_splits * tail_rows * N * 4`: it pins the split count, the
    tail-launch decision and the 256 x 256 plan's use wherever they change that figure.  What it CANNOT see: the tile choice at equal
    splits (64 x 64 against 128 x 128 at one split or at the same split count), kchunk beyond what fixes `splits`, and the smaller of
    the two precisions' needs.  For those the tests rest on the transcription alone -- no test observes the tile size on the device.
  * Every row of the case table reaches the plan it names, in both precisions, and the table as a whole reaches every branch of
    REQUIRED_BRANCHES (asserted, not commented).
  * Every "exact" case is exact (bound from the actual arrays, float64 reference integral) and not degenerate."""
import numpy as np
import pytest

from vae_captioning_amd import abi

from . import gemm_edges_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return abi.load()


# ------------------------------------------------------------------------------------------------ the transcription against the library
def _threshold_shapes():
    """(M, N) whose 128 x 128 tile count sits on plan_gemm's thresholds and whose 256 x 256 tile count on plan_bx256's, with ragged
    variants; K on the steps of K / 256, K / 512, K / 640, K / 1024 and the whole-rounds tail's K-tile counts"""
    mn = []
    for t, pairs in ((128, [(8, 16), (128, 1), (2, 64)]), (129, [(3, 43), (43, 3)]), (383, [(383, 1), (1, 383)]), (384, [(16, 24), (6, 64)]),
                     (767, [(13, 59), (59, 13)]), (768, [(24, 32), (96, 8)]), (769, [(769, 1), (1, 769)]), (776, [(97, 8), (8, 97)]),
                     (1540, [(55, 28), (28, 55)])):
        for tm, tn in pairs:
            assert tm * tn == t
            for dm, dn in ((0, 0), (127, 0), (0, 127), (1, 3)):
                mn.append((tm * 128 - dm, tn * 128 - dn))
    for t, pairs in ((199, [(199, 1), (1, 199)]), (200, [(10, 20), (8, 25), (200, 1)]), (16, [(4, 4)]), (15, [(3, 5)]), (13, [(13, 1)])):
        for tm, tn in pairs:
            assert tm * tn == t
            for dm, dn in ((0, 0), (255, 0), (0, 255), (64, 64), (65, 64)):
                mn.append((tm * 256 - dm, tn * 256 - dn))
    mn += [(64, 256), (65, 256), (64, 255), (1, 256), (64, 128 * 7), (64, 128 * 12 + 1), (191, 5000), (192, 192 * 200), (300, 300), (1, 1)]
    ks = {0, 1, 31, 32, 33, 255, 256, 257, 511, 512, 513}
    for step in (256, 512, 640, 1024):
        for q in (1, 2, 3, 4, 7, 12, 13, 15, 16, 17, 32, 33, 64, 65):
            ks.update((q * step - 1, q * step, q * step + 1))
    return [(M, N, K) for M, N in mn for K in sorted(ks)]


def _seeded_shapes(n=3000):
    rng = np.random.default_rng(20240521)
    out = []
    for _ in range(n):
        kind = rng.integers(0, 4)
        if kind == 0:      # around the skinny boundary
            out.append((int(rng.integers(1, 70)), int(rng.integers(250, 1300)), int(rng.integers(480, 9000))))
        elif kind == 1:    # small outputs, deep K
            out.append((int(rng.integers(1, 1500)), int(rng.integers(1, 1500)), int(rng.integers(0, 40000))))
        elif kind == 2:    # around one round of 128 x 128 tiles and 200 tiles of 256 x 256
            out.append((int(rng.integers(1500, 5000)), int(rng.integers(1500, 5000)), int(rng.integers(0, 20000))))
        else:              # long and narrow
            out.append((int(rng.integers(1, 60000)), int(rng.integers(1, 1200)), int(rng.integers(0, 5000))))
    return out


def test_workspace_query_matches_the_transcription_on_every_case(built):
    for M, N, K in R.CASES + R.K0_CASES:
        assert built.vc_gemm_workspace_bytes(M, N, K) == R.expected_workspace_bytes(M, N, K), (M, N, K)
    for M, N, K in R.K0_CASES:
        assert built.vc_gemm_workspace_bytes(M, N, K) == 0                      # include/vaecap.h: K == 0 needs no workspace


def test_workspace_query_matches_the_transcription_on_a_sweep_of_the_thresholds(built):
    shapes = _threshold_shapes() + _seeded_shapes()
    assert len(shapes) > 5000
    seen = set()
    for M, N, K in shapes:
        got, want = built.vc_gemm_workspace_bytes(M, N, K), R.expected_workspace_bytes(M, N, K)
        assert got == want, ((M, N, K), got, want, R.plan_gemm(M, N, K), R.plan_bx256(M, N, K))
        p, b = R.plan_gemm(M, N, K), R.plan_bx256(M, N, K)
        seen.add(("skinny" if p.skinny else "128" if p.big else "64", p.splits > 1, p.tail_splits > 1, b.use, b.use and b.splits > 1))
    # the sweep is not one-sided: every tile choice with and without splits, the tail, the 256 x 256 plan with and without splits
    for want in (("skinny", True), ("skinny", False), ("64", True), ("64", False), ("128", True), ("128", False)):
        assert any(s[:2] == want for s in seen), want
    assert any(s[2] for s in seen) and any(s[3] and not s[4] for s in seen) and any(s[4] for s in seen)
    assert any(s[3] and s[2] for s in seen)      # bx in use where the f32 plan has a tail: the query takes the larger need


def test_planners_never_return_zero_splits():
    for M, N in ((1, 1), (64, 300), (70, 96), (300, 300), (3601, 3331), (12400, 1024)):
        p, b = R.plan_gemm(M, N, 0), R.plan_bx256(M, N, 0)
        assert p.splits == 1 and p.kchunk == 32 and p.tail_splits == 1
        assert not b.use or (b.splits == 1 and b.kchunk == 32)
        assert R.expected_workspace_bytes(M, N, 0) == 0


def test_k_zero_still_validates_its_arguments(built):
    """argument checks come before any device work: K == 0 lets A and B be NULL (they are never read), not C"""
    for fn, flags in ((built.vc_gemm_f32, 0), (built.vc_gemm_f32, R.BF16X3), (built.vc_gemm_bf16x3_f32, 0)):
        with pytest.raises(abi.VaecapError) as e:
            fn(None, 0, 0, 4, 4, 0, None, 0, None, 4, None, 4, None, flags, None, 0)
        assert "null operand" in str(e.value)
        with pytest.raises(abi.VaecapError) as e:
            fn(None, 0, 0, 4, 4, -1, None, 0, None, 4, None, 4, None, flags, None, 0)
        assert "negative dimension" in str(e.value)
        assert fn(None, 0, 0, 0, 4, 0, None, 0, None, 4, None, 4, None, flags, None, 0) == 0      # M == 0: nothing to do


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("row", R.CASE_ROWS, ids=lambda r: R.case_id(r[0]))
def test_every_row_reaches_the_plan_it_names(row):
    (M, N, K), f, b, note = row
    assert R.plan_for(M, N, K, "f32") == f, (note, R.plan_for(M, N, K, "f32"))
    assert R.plan_for(M, N, K, "bf16x3") == b, (note, R.plan_for(M, N, K, "bf16x3"))


def branches(case):
    """names of the dispatch branches a case reaches (in the plain dress, given its whole workspace)"""
    M, N, K = case
    out = set()
    for prec in R.PRECS:
        p = R.plan_for(M, N, K, prec)
        g = R.plan_gemm(M, N, K)
        out.add("tile %s %s" % (p.tile, prec))
        if p.splits > 1:
            out.add("split-K %s %s" % (p.tile, prec))
            last = R.last_split_k(M, N, K, prec)
            if last == p.kchunk:
                out.add("splits of exactly kchunk %s" % prec)
            if 0 < last < 32 <= K and prec == "bf16x3" and all(R.vec_in(M, N, K, ta, tb) for ta, tb in R.ORDERS):
                out.add("shifted tile is a split's only tile")
            if last > 32 and last % 32 and prec == "bf16x3" and p.tile == "256":
                out.add("256: shifted tile in the last split, %s" % ("aligned" if R.vec_in(M, N, K, 0, 1) else "guarded"))
            elems = M * N
            if N % 4 == 0 and elems // 4 > R.REDUCE4_CAP:
                out.add("float4 reduce past its cap")
            if N % 4 == 0:
                out.add("float4 reduce")
            else:
                out.add("scalar reduce")
                if elems > R.REDUCE_CAP:
                    out.add("scalar reduce past its cap")
        if p.tail_splits > 1:
            out.add("tail launch %s" % prec)
            rows = M - g.main_m * 128
            assert 0 < rows <= (g.tiles_m - g.main_m) * 128
            if R.tail_last_split_k(M, N, K) % 32:
                out.add("tail launch, ragged last split")
        if prec == "bf16x3" and p.tile == "256":
            b = R.plan_bx256(M, N, K)
            if b.tiles_m > R.BX_GROUP and b.tiles_m % R.BX_GROUP:
                out.add("256: grouped order with a short last group")
            if K < 32:
                out.add("256: K < 32")
            if p.splits == 1 and R.cdiv(K, 32) == 1:
                out.add("256: one-tile K loop, %s" % ("aligned" if K == 32 and R.vec_in(M, N, K, 0, 1) and R.vec_in(M, N, K, 1, 0) else "guarded"))
            if p.splits == 1 and K > 32 and K % 32:
                out.add("256: shifted last K tile")
        if p.tile != "64" and N % 4:     # the row pitch of the output is N for C and for the workspace alike (plain dress)
            out.add("scalar epilogue on %s %s" % (p.tile, prec))
    if K % 4 and K % 32 and K > 32 and R.vec_in(M, N, K, 1, 0):     # ta = 1, tb = 0: VEC holds with any K
        out.add("row-contiguous order: shift with K %% 4 != 0 on %s" % R.plan_for(M, N, K, "bf16x3").tile)
    return out


REQUIRED_BRANCHES = (
    ["tile %s %s" % (t, p) for p in R.PRECS for t in ("64", "128", "skinny")] + ["tile 256 bf16x3"] +
    ["split-K %s %s" % (t, p) for p in R.PRECS for t in ("64", "128", "skinny")] + ["split-K 256 bf16x3"] +
    ["tail launch f32", "tail launch bf16x3", "tail launch, ragged last split",
     "scalar reduce", "float4 reduce", "scalar reduce past its cap", "float4 reduce past its cap",
     "256: grouped order with a short last group", "256: K < 32", "256: one-tile K loop, aligned", "256: one-tile K loop, guarded", "256: shifted last K tile",
     "256: shifted tile in the last split, aligned", "256: shifted tile in the last split, guarded",
     "splits of exactly kchunk bf16x3", "shifted tile is a split's only tile",
     "row-contiguous order: shift with K % 4 != 0 on 64", "row-contiguous order: shift with K % 4 != 0 on skinny",
     "row-contiguous order: shift with K % 4 != 0 on 256",
     "scalar epilogue on 128 f32", "scalar epilogue on 256 bf16x3", "scalar epilogue on skinny f32", "scalar epilogue on skinny bf16x3"])


def test_the_table_reaches_every_branch_it_is_there_for():
    reached = {}
    for c in R.CASES:
        for b in branches(c):
            reached.setdefault(b, []).append(c)
    missing = [b for b in REQUIRED_BRANCHES if b not in reached]
    assert not missing, missing
    # the skinny boundary: the three conditions of `M <= 64 && N >= 256 && K >= 512`, each one step outside
    assert R.plan_gemm(64, 256, 512).skinny and R.plan_gemm(1, 256, 512).skinny
    for c in ((65, 256, 512), (64, 255, 512), (64, 256, 511)):
        assert c in R.CASES and not R.plan_gemm(*c).skinny
    # the shapes that differ between the precisions do so because plan_bx256 takes or declines them at 200 tiles
    assert R.plan_bx256(3584, 3584, 1024).tiles_m * R.plan_bx256(3584, 3584, 1024).tiles_n == 196
    b = R.plan_bx256(12300, 1028, 1060)
    assert b.use and (b.tiles_m, b.tiles_n) == (49, 5) and b.tiles_m % R.BX_GROUP == 1
    assert R.plan_gemm(12300, 1028, 1060).main_m == 85 and R.plan_gemm(3584, 3584, 1024).main_m == 27
    # K = 33 shifts by 31, K = 40 by 24, K = 100 by 28; 13400 = 12 * 1056 + 22 * 32 + 24
    assert 13400 - 12 * 1056 == 22 * 32 + 24 and R.last_split_k(772, 1020, 13400, "bf16x3") == 728
    for c in ((64, 256, 2308), (260, 264, 2308), (260, 264, 15236)):
        assert R.last_split_k(*c, "bf16x3") == 4 and R.last_split_k(*c, "f32") == 4


def test_every_flag_meets_every_case_and_the_dress_cases_have_splits():
    for c in R.CASES:
        assert sorted(R.flags_of(c, ta, tb) for ta, tb in R.ORDERS) == [0, 1, 2, 3]
        assert {R.with_bias(c, ta, tb) for ta, tb in R.ORDERS} == {True, False}
    for prec in R.PRECS:
        tiles = set()
        for c in R.DRESS_CASES[prec]:
            M, N, K = c
            p = R.plan_for(M, N, K, prec)
            assert c in R.CASES and (p.splits > 1 or p.tail_splits > 1) and N % 4 == 0, c
            assert all(R.vec_in(M, N, K, ta, tb) for ta, tb in R.ORDERS), c      # the dress is what switches the vector paths off
            tiles.add(p.tile)
        assert tiles == ({"64", "128", "skinny"} | ({"256"} if prec == "bf16x3" else set()))
    assert R.plan_for(*R.DRESS_CASES["f32"][3], "f32").tail_splits == 2
    for c in R.DETERMINISM_CASES:
        assert c in R.CASES
    assert "scalar reduce" in branches(R.DETERMINISM_CASES[0]) and "float4 reduce" in branches(R.DETERMINISM_CASES[1])
    assert "tail launch f32" in branches(R.DETERMINISM_CASES[2]) and "tail launch bf16x3" in branches(R.DETERMINISM_CASES[2])


def test_dress_geometry_says_what_it_is_for():
    M, N, K = 772, 1020, 13400
    for ta, tb in R.ORDERS:
        ea, eb = (M if ta else K), (K if tb else N)
        assert R.dress_geometry("plain", M, N, K, ta, tb) == (ea, eb, N, 0)
        g = R.dress_geometry("padded", M, N, K, ta, tb)
        assert (g.lda, g.ldb, g.ldc, g.offset) == (ea + 4, eb + 8, N + 4, 0) and g.lda % 4 == 0 and g.ldb % 4 == 0 and g.ldc % 4 == 0
        g = R.dress_geometry("odd", M, N, K, ta, tb)
        assert g.lda % 4 and g.ldb % 4 and g.ldc % 4 and g.offset == 0
        assert R.dress_geometry("offset", M, N, K, ta, tb) == (ea, eb, N, 1)
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    buf = R.embed(a, 5, 1, R.NAN)
    assert buf.size == 1 + 10 + R.GUARD and np.isnan(buf[0]) and np.array_equal(buf[1:4], a[0]) and np.array_equal(buf[6:9], a[1])
    assert np.isnan(buf[4:6]).all() and np.isnan(buf[9:]).all()


# ------------------------------------------------------------------------------------------------ the inputs
def _integers(a):
    return np.array_equal(a, np.rint(a)) and (a.size == 0 or np.abs(a).max() < R.EXACT_LIMIT)


@pytest.mark.parametrize("case", R.CASES + R.K0_CASES, ids=R.case_id)
def test_exact_cases_are_exact_and_not_degenerate(case):
    M, N, K = case
    A, B, bias, C0 = R.inputs(case, "exact")
    assert A.shape == (M, K) and B.shape == (K, N) and bias.shape == (N,) and C0.shape == (M, N)
    assert R.amax(A) <= 4 and R.amax(B) <= 3 and R.amax(bias) <= 5 and R.amax(C0) <= 5
    assert R.is_exact(case) and R.exact_bound(case) == K * R.amax(A) * R.amax(B) + R.amax(bias) + R.amax(C0)
    assert _integers(R.product(case, "exact"))
    # the (flags, bias) pairs the GPU test runs: a case's four storage orders; every pair for K == 0
    combos = [(f, wb) for f in range(4) for wb in (True, False)] if K == 0 else \
        [(R.flags_of(case, ta, tb), R.with_bias(case, ta, tb)) for ta, tb in R.ORDERS]
    for flags, with_bias in combos:
        ref = R.reference(case, "exact", flags, with_bias)
        assert _integers(ref), (case, flags)
        if M * N < 64 or (K == 0 and not with_bias and not flags & R.ACCUMULATE):
            continue            # 1 and 15 outputs: fractions mean nothing; epilogue(0) without bias and C0 is all zero
        if flags & R.RELU:
            pre = R.reference(case, "exact", flags & ~R.RELU, with_bias)
            assert 4 * np.count_nonzero(pre < 0) >= pre.size and 4 * np.count_nonzero(ref > 0) >= ref.size, (case, flags)
        else:
            assert 2 * np.count_nonzero(ref) > ref.size, (case, flags)


def test_random_inputs_are_standard_normal_and_cached_read_only():
    case = (129, 131, 37)
    A, B, bias, C0 = R.inputs(case, "random")
    assert A.dtype == np.float32 and abs(float(A.std()) - 1) < 0.05 and abs(float(B.mean())) < 0.05
    assert R.inputs(case, "random")[0] is A and not A.flags.writeable
    with pytest.raises(ValueError):
        R.product(case, "random")[0, 0] = 1.0
    ref = R.reference(case, "random", R.RELU | R.ACCUMULATE)
    want = np.maximum(A.astype(np.float64) @ B.astype(np.float64) + bias + C0, 0)
    np.testing.assert_allclose(ref, want, rtol=0, atol=1e-12)
