"""CPU: the numpy restatement of cv::findHomography (tests/_homography_oracle.py)
against what the real reference returned (tests/golden/reference_homography.npz,
both dispatch states), under the numerics contract of DESIGN.md §5
"findHomography":

A. exact: validity, the consensus size and the whole mask in every case, and
   the bits of H where the reference exposes the un-refined matrix (4 pairs);
B. the one margin: every niters update's num/denom is further than 1e-6 from
   k + 0.5, so libm's log and pow cannot move an iteration count;
C. the refined H by what it does to the inlier points, within BAR_PX."""
import numpy as np
import pytest

import _homography_cases as HC
import _homography_oracle as HO

# Contract C.  Measured on the CPU over all 42 committed cases, as the largest displacement of a case's inlier
# points between two matrices: d(restatement, recorded noavx2) = 9.64e-9 px, d(recorded default, recorded noavx2)
# = 3.12e-8 px (the largest cases: "status alt" and "truth strong").  Both are the same algorithm in another
# double-precision evaluation order, which is what the device is too; the bar is 8 x the larger maximum.  No case's
# two recorded states lie more than 1e-4 px apart.
MEASURED_RESTATEMENT_PX = 9.64e-9
MEASURED_STATES_PX = 3.12e-8
BAR_PX = 8 * max(MEASURED_RESTATEMENT_PX, MEASURED_STATES_PX)


def _compacted(i):
    return HC.compact(*HC.fixture_inputs(HO.fixture(), i)[:3])


def test_the_case_table_is_whole():
    fx = HO.fixture()
    assert len(HC.cases()) == HC.NCASES == 42
    assert str(fx["state"]) == "noavx2"
    assert all(f"{i}_mask" in fx.files and f"{i}_H" in fx.files and f"src_{i}" in fx.files for i in range(HC.NCASES))
    assert fx["other_ints_equal"].all()  # masks and validity are the same in both dispatch states
    ns = sorted({len(fx[f"src_{i}"]) for i in range(HC.NCASES)})
    assert {0, 3, 4, 5, 8, 63, 64, 65, 200, 1000} <= set(ns)


@pytest.mark.parametrize("i", range(HC.NCASES))
def test_restatement_matches_recording(i):
    s, d = _compacted(i)
    valid, nin, mask, h, _ = HC.fixture_outputs(HO.fixture(), i, len(s))
    r = HO.table_result(i)
    assert (r.valid, r.ninliers) == (valid, nin)
    assert np.array_equal(r.mask, mask)
    if not valid:
        assert np.array_equal(np.array(r.H).reshape(3, 3), np.eye(3))
        return
    if len(s) == 4:
        assert np.array(r.H, np.float64).tobytes() == h.tobytes()
    dist = HO.distance(r.H, h, s[mask != 0])
    print(f"{HC.label(i)}: d(restatement, noavx2) = {dist:.3g} px, iters {r.iters}")
    assert dist <= BAR_PX


def test_margins_of_the_niters_update():
    small = min((m, HC.label(i)) for i in range(HC.NCASES) for m in HO.table_result(i).margins)
    print(f"smallest distance of num/denom from k + 0.5: {small[0]:.3g} ({small[1]})")
    assert small[0] > 1e-6


def test_measured_distances_are_the_documented_ones():
    fx = HO.fixture()
    rest = states = 0.0
    for i in range(HC.NCASES):
        s, _ = _compacted(i)
        valid, _, mask, h, other = HC.fixture_outputs(fx, i, len(s))
        if valid:
            inl = s[mask != 0]
            rest = max(rest, HO.distance(HO.table_result(i).H, h, inl))
            states = max(states, HO.distance(other, h, inl))
    print(f"d(restatement, noavx2) = {rest:.3g} px, d(default, noavx2) = {states:.3g} px, bar {BAR_PX:.3g} px")
    assert rest <= MEASURED_RESTATEMENT_PX * 1.001 and states <= MEASURED_STATES_PX * 1.001
    assert states < 1e-4


def test_the_loop_stops_where_the_table_means_it_to():
    it = {HC.label(i): HO.table_result(i).iters for i in range(HC.NCASES)}
    assert it["outliers 0"] < 64 and it["size 200"] < 64  # inside the first batch
    assert [it[f"max_iters {k}"] for k in (1, 7, 63, 64, 65, 300)] == [1, 7, 63, 64, 65, 300]
    assert 64 < it["outliers 60"] < 2000 and it["outliers 85"] == 500
    assert it["collinear"] == 0 and it["coincident"] == 0  # 10000 attempts, no subset
    assert HO.table_result([HC.label(i) for i in range(HC.NCASES)].index("max_iters 300")).ninliers < 8


def test_refine_off_returns_the_refit():
    i = [HC.label(k) for k in range(HC.NCASES)].index("size 65")
    a, b = HO.table_result(i), HO.table_result(i, refine=False)
    assert b.H == a.H0 and np.array_equal(a.mask, b.mask) and b.H != a.H
