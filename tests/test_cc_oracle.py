"""CPU: the numpy restatement of connectedComponentsWithStats (tests/_cc_oracle.py: flood fill, rank by the scan's
key, stats) against the outputs recorded from the real reference (tests/golden/reference_cc.npz, both dispatch
states): labels, N, stats and centroids, bit for bit (a NaN centroid as NaN)."""
import numpy as np
import pytest

import _cc_cases as LC
import _cc_oracle as CO
import _reference_cases as RC

CASES = LC.cases()


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("cc")


def test_the_fixture_holds_one_recording_for_both_dispatch_states(fx):
    # connectedcomponents.cpp has no dispatched code: the two states' recordings were byte-identical
    assert str(fx["state"]) == "both"
    assert len(CASES) == len(fx["other_ints_equal"]) == 300 and fx["other_ints_equal"].all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: LC.label(i).replace(" ", "_"))
def test_restatement_equals_the_recorded_reference(fx, i):
    content, w, h, conn, t = CASES[i]
    n, labels, stats, cent = CO.connected_components_with_stats(LC.image(content, w, h), conn, t)
    rn, rstats, rcent = LC.unpack_stats(fx[f"{i}_s"])
    assert n == rn, LC.label(i)
    want = fx[f"{i}_labels"]
    got = LC.stored_labels(labels)
    assert got.shape == want.shape and np.array_equal(got, want), LC.label(i)
    assert np.array_equal(stats, rstats), LC.label(i)
    assert CO.same_centroids(cent, rcent), LC.label(i)


def _recorded(fx, content, w, h, conn, t):
    return fx[f"{CASES.index((content, w, h, conn, t))}_labels"]


def test_the_pixel_scan_and_the_block_scan_number_differently(fx):
    # components starting at (row 1, col 0) and (row 0, col 2): Wu numbers the second first, Grana the first
    wu, grana = _recorded(fx, "order", 3, 3, 8, LC.CCL_WU), _recorded(fx, "order", 3, 3, 8, LC.CCL_GRANA)
    assert (wu[0, 2], wu[1, 0]) == (1, 2) and (grana[0, 2], grana[1, 0]) == (2, 1)
    assert np.array_equal(grana, _recorded(fx, "order", 3, 3, 8, LC.CCL_DEFAULT))
    # at connectivity 4 every type is the pixel scan
    for t in (LC.CCL_DEFAULT, LC.CCL_GRANA):
        assert np.array_equal(_recorded(fx, "order", 3, 3, 4, t), _recorded(fx, "order", 3, 3, 4, LC.CCL_WU))


def test_an_image_without_background_keeps_the_initial_row_0(fx):
    i = CASES.index(("full", 17, 13, 8, LC.CCL_DEFAULT))
    n, stats, cent = LC.unpack_stats(fx[f"{i}_s"])
    assert n == 2 and stats[0].tolist() == [2 ** 31 - 1, 2 ** 31 - 1, 2, 2, 0] and np.isnan(cent[0]).all()
    assert stats[1].tolist() == [0, 0, 17, 13, 17 * 13] and cent[1].tolist() == [8.0, 6.0]


def test_the_cases_hold_what_they_are_for(fx):
    # the checkerboard: one component at 8, the reference's own label bound at 4
    for w, h in ((17, 13), (64, 48)):
        assert LC.unpack_stats(fx[f"{CASES.index(('checker', w, h, 8, LC.CCL_WU))}_s"])[0] == 2
        assert LC.unpack_stats(fx[f"{CASES.index(('checker', w, h, 4, LC.CCL_WU))}_s"])[0] == (w * h + 1) // 2 + 1
    # the comb is one component, the spiral's two arms stay apart, the diagonals differ between 4 and 8
    assert LC.unpack_stats(fx[f"{CASES.index(('comb', 130, 121, 4, LC.CCL_WU))}_s"])[0] == 2
    n, stats, _ = LC.unpack_stats(fx[f"{CASES.index(('spiral', 130, 121, 8, LC.CCL_DEFAULT))}_s"])
    assert n >= 3 and sorted(stats[1:, 4])[-2] > 3000
    assert LC.unpack_stats(fx[f"{CASES.index(('diagonals', 17, 13, 8, LC.CCL_WU))}_s"])[0] == 2
    assert LC.unpack_stats(fx[f"{CASES.index(('diagonals', 17, 13, 4, LC.CCL_WU))}_s"])[0] == 26
    assert set(np.unique(LC.image("values", 67, 23))) == {0, 1, 127, 255}
    m = LC.mog2_mask()
    assert m.shape == (48, 64) and set(np.unique(m)) == {0, 127, 255}
