"""CPU: the numpy restatement of BackgroundSubtractorMOG2 (tests/_mog2_oracle.py) against the masks and
background images recorded from the real reference (tests/golden/reference_mog2.npz, both dispatch states),
bit for bit, and the exact counts of the branches the recorded sequences take."""
import time

import numpy as np
import pytest

import _mog2_cases as GC
import _mog2_oracle as MO
import _reference_cases as RC

# the gray base sequence at history 12, automatic rate
BASE_COUNTS = dict(fits=129382, new_modes=18074, replacements=9217, prunes=743, fit_sorts=7116, new_sorts=402,
                   shadows=15034, foreground=2523, var_max_clamps=5094, var_min_clamps=51557,
                   zero_denominators=384)
# all 29 cases
TOTAL_COUNTS = dict(fits=2703910, new_modes=416049, replacements=221145, prunes=13998, fit_sorts=136156,
                    new_sorts=22652, shadows=329809, foreground=133996, var_max_clamps=104340,
                    var_min_clamps=832872, zero_denominators=8432)


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("mog2")


def test_the_fixture_holds_one_recording_for_both_dispatch_states(fx):
    # bgfg_gaussmix2.cpp has no dispatched code: the two states' recordings were byte-identical
    assert str(fx["state"]) == "both"
    assert len(GC.cases()) == GC.NCASES == len(fx["other_ints_equal"])
    assert fx["other_ints_equal"].all()


@pytest.mark.parametrize("i", range(GC.NCASES))
def test_masks_and_backgrounds_equal_the_recorded_reference(fx, i):
    case = GC.cases()[i]
    masks, bgs, _, _ = MO.expected(i)
    assert np.array_equal(GC.stored_masks(case, masks), fx[f"{i}_masks"]), case["name"]
    if case["whole"]:
        p = GC.params(case)
        back = GC.unpack_masks(fx[f"{i}_masks"], case["n"], case["h"], case["w"], p["shadow_value"])
        assert np.array_equal(back, masks), case["name"]
    for t in case["bg"]:
        got, want = GC.stored_background(bgs[t]), fx[f"{i}_bg{t}"]
        assert got.dtype == want.dtype and np.array_equal(got, want), (case["name"], t)


def test_the_branches_the_sequences_take():
    assert MO.expected(0)[3] == BASE_COUNTS
    total = dict.fromkeys(MO.EVENTS, 0)
    for i in range(GC.NCASES):
        for k, v in MO.expected(i)[3].items():
            total[k] += v
    assert total == TOTAL_COUNTS
    assert all(v > 0 for v in total.values())


def test_the_sequence_holds_what_the_cases_need():
    f = GC.frames()
    assert f.shape == (GC.NFRAMES, GC.H, GC.W) and f.dtype == np.uint8
    assert not f[:, :, :8].any()  # the shadow test's zero denominator
    assert len(np.unique(f[:, 0, 56])) == 9  # more levels than nmixtures
    assert f[:, :, 8:56].min() >= 0 and (f[29, :40, 8:56].astype(int) - f[30, :40, 8:56]).mean() < -15  # the step
    c3 = GC.frames(cn=3)
    assert (c3[..., 0] != c3[..., 1]).any() and not c3[:, :, :8].any()
    unit = GC.frames(content="unit")
    assert unit.dtype == np.float32 and 0 <= unit.min() and unit.max() <= 1.01


def test_a_1242x375_frame_takes_a_second_or_two():
    f = GC.frames(1242, 375, 2, 3)
    m = MO.MOG2()
    t0 = time.perf_counter()
    for fr in f:
        m.apply(fr)
    m.background_image()
    assert time.perf_counter() - t0 < 2 * 2.5
