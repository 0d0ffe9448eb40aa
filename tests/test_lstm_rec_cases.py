"""The case tables of tests/lstm_rec_ref.py (what tests/test_gpu_lstm_rec.py runs on the device) checked on the host: on the 256 CUs
of an MI355X every backward case lands on the instantiation of lstm_rec_bwd_kernel<RT, BX, CT> its id names, the tables cover every
instantiation with whole and ragged row blocks and one and several passes, they evaluate on other CU counts, and the comparison the
device tests use is tight enough that a kernel skipping one row could not pass."""
import numpy as np
import pytest

from . import lstm_rec_ref as R
from .gpu_util import assert_close

BWD_IDS = [c[0] for c in R.BWD_CASES]


@pytest.mark.parametrize("case", R.BWD_CASES, ids=BWD_IDS)
def test_backward_case_lands_on_its_variant_on_256_cus(case):
    name, n_of, want = case
    N = n_of(256)
    path = R.bwd_path(N, 256)
    assert R.bwd_case_skip_reason(name, N, 256) is None, "no case may be skipped on 256 CUs"
    assert want(path), (name, N, path)
    assert (N, path) == R.BWD_ON_256[name]


def test_backward_mirror_restates_the_rule():
    """spot values worked out by hand from rec_bwd / rec_row_groups"""
    assert R.bwd_path(320, 256) == (1, 3, 8, 40, 1, 40)      # 8 groups of 40 rows
    assert R.bwd_path(599, 256) == (1, 5, 8, 75, 1, 74)      # 7 x 75 + 74
    assert R.bwd_path(600, 256) == (2, 3, 16, 38, 1, 30)     # 15 x 38 + 30
    assert R.bwd_path(1700, 256) == (2, 5, 16, 107, 2, 95)   # 15 x 107 + 95 = 80 + 15
    assert R.bwd_path(2560, 256) == (2, 5, 16, 160, 2, 160)
    assert R.bwd_path(5, 256) == (1, 3, 1, 5, 1, 5)
    assert R.bwd_path(650, 64) == (2, 5, 4, 163, 3, 161)
    assert R.bwd_path(40, 8) == (1, 3, 1, 40, 1, 40)          # fewer CUs than column slices: one row group


def test_backward_table_covers_every_variant():
    paths = {name: R.bwd_path(n_of(256), 256) for name, n_of, _ in R.BWD_CASES}
    assert len(set(BWD_IDS)) == len(BWD_IDS) == 13 and set(BWD_IDS) == set(R.BWD_ON_256)
    assert {(p.CT, p.RT) for p in paths.values()} == {(1, 3), (1, 5), (2, 3), (2, 5)}
    for pair in ((1, 3), (1, 5), (2, 3), (2, 5)):
        assert any((p.CT, p.RT) == pair and p.last_group_rows % 16 != 0 for p in paths.values()), "no ragged case for CT%d / RT%d" % pair
    ct2rt5 = [p for p in paths.values() if (p.CT, p.RT) == (2, 5)]
    assert any(p.passes == 1 for p in ct2rt5) and any(p.passes >= 2 for p in ct2rt5)
    for name, p in paths.items():
        assert R.bwd_case_ct(name) == p.CT and ("rt%d" % p.RT) in name


def test_forward_table_covers_every_variant():
    ns = [n_of(256) for _, n_of, _ in R.FWD_BX_CASES]
    assert ns == R.FWD_BX_NS_ON_256
    paths = []
    for name, n_of, want in R.FWD_BX_CASES:
        path = R.fwd_path(n_of(256), 256)
        assert want(*path), (name, path)
        assert name.startswith(path[0])
        paths.append(path)
    kinds = {(k, min(p, 2)) for k, _, p in paths}
    assert {("rec-rt3", 1), ("rec-rt5", 1), ("rec-rt5", 2), ("rec8", 1), ("rec8", 2)} <= kinds


def test_forward_mirror_restates_the_rule():
    assert R.fwd_path(320, 256) == ("rec-rt5", 80, 1)
    assert R.fwd_path(400, 256) == ("rec-rt5", 100, 2)
    assert R.fwd_path(401, 256) == ("rec8", 51, 1)
    assert R.fwd_path(1281, 256) == ("rec8", 161, 3)
    assert R.fwd_path(37, 256) == ("rec-rt3", 13, 1)


@pytest.mark.parametrize("cus", [64, 104, 256, 304])
def test_tables_evaluate_on_other_cu_counts(cus):
    for name, n_of, want in R.BWD_CASES:
        N = n_of(cus)
        assert N >= 1, name
        path = R.bwd_path(N, cus)
        assert path.RG >= 1 and path.rows >= 1 and path.passes >= 1 and 1 <= path.last_group_rows <= path.rows
        assert (path.RG - 1) * path.rows < N <= path.RG * path.rows, "every row group has a row"
        reason = R.bwd_case_skip_reason(name, N, cus)
        assert reason is None or (str(N) in reason and name in reason)
        assert isinstance(want(path), bool)
    for name, n_of, want in R.FWD_BX_CASES:
        N = n_of(cus)
        assert N >= 1, name
        assert isinstance(want(*R.fwd_path(N, cus)), bool)


# ----------------------------------------------------------------------------- the checker itself
@pytest.fixture(scope="module")
def small():
    return R.make_bwd_problem(40, 3, 8, 32, seed=40)


def test_reference_matches_the_oracle_and_masks_rows(small):
    ref, lens = small["ref"], small["lens"]
    assert lens[0] == 3 and lens[39] == 3 and lens[1] == 0 and lens[2] == 1
    assert (ref["dG"][:, 1] == 0).all() and (ref["dG"][1:, 2] == 0).all() and (ref["dG"][0, 2] != 0).any()
    assert np.array_equal(ref["dc0"][1], small["dC0"][1].astype(np.float64)), "a row that never runs carries dC"
    assert_close(ref["dG"] @ small["cache"]["W"][:8].T, ref["dX"], 1e-12, msg="dX of the restated loop")
    assert_close(ref["dG"].sum((0, 1)), ref["db"], 1e-12, msg="db of the restated loop")


def test_reference_without_external_gradients_differs(small):
    """dhs_ext = NULL is another problem, not the same one: the external gradient reaches every output"""
    bare = R.make_bwd_problem(40, 3, 8, 32, seed=40, with_ext=False)
    assert bare["dhs_ext"] is None and np.array_equal(bare["act"], small["act"])
    for k in ("dG", "dh1", "dc0"):
        with pytest.raises(AssertionError):
            assert_close(bare["ref"][k], small["ref"][k], 5e-5)


def test_checker_rejects_a_skipped_dG_row(small):
    ref, lens = small["ref"]["dG"], small["lens"]
    assert_close(ref.copy(), ref, 5e-5)
    for t in range(3):
        for row in np.nonzero(lens > t)[0]:   # every active row of every step: none is small enough to hide
            bad = ref.copy()
            bad[t, row] = 0
            with pytest.raises(AssertionError):
                assert_close(bad, ref, 5e-5, msg="dG with row %d of step %d skipped" % (row, t))


def test_checker_rejects_a_stale_dH_row(small):
    ref, dH0 = small["ref"]["dh1"], small["dH0"].astype(np.float64)
    for row in range(40):
        bad = ref.copy()
        bad[row] = dH0[row]                   # the row still holds what it held on entry
        with pytest.raises(AssertionError):
            assert_close(bad, ref, 5e-5, msg="dH_run with row %d left at its entry value" % row)
