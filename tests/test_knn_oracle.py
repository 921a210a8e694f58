"""CPU: the numpy restatement of BackgroundSubtractorKNN and of cv::randu (tests/_knn_oracle.py) against the
masks, background images, periods and final RNG states recorded from the real reference
(tests/golden/reference_knn.npz, both dispatch states), bit for bit, and the exact counts of the branches the
recorded sequences take.  The recorded RNG state pins the number of steps every fill consumed."""
import numpy as np
import pytest

import _knn_cases as KC
import _knn_oracle as KO
import _reference_cases as RC

# the gray base sequence at history 500, automatic rate
BASE_COUNTS = dict(early_backgrounds=83065, include_by_pbf=29070, shadows=3983, zero_denominators=384,
                   foreground=60408, short_updates=63294, mid_updates=49152, long_updates=24576, fills_small=30,
                   fills_bits=0, fills_div=13)
# all 27 cases
TOTAL_COUNTS = dict(early_backgrounds=1284683, include_by_pbf=471783, shadows=77086, zero_denominators=30869,
                    foreground=1592079, short_updates=1727479, mid_updates=1474425, long_updates=771212,
                    fills_small=825, fills_bits=1, fills_div=192)


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("knn")


def test_the_fixture_holds_one_recording_for_both_dispatch_states(fx):
    # neither bgfg_KNN.cpp nor rand.cpp has dispatched code: the two states' recordings were byte-identical
    assert str(fx["state"]) == "both"
    assert len(KC.cases()) == KC.NCASES == len(fx["other_ints_equal"])
    assert fx["other_ints_equal"].all()


@pytest.mark.parametrize("i", range(KC.NCASES))
def test_masks_backgrounds_and_rng_state_equal_the_recorded_reference(fx, i):
    case = KC.cases()[i]
    masks, bgs, model, _, _, _ = KO.expected(i)
    assert np.array_equal(KC.stored_masks(case, masks), fx[f"{i}_masks"]), case["name"]
    if case["whole"]:
        p = KC.params(case)
        back = KC.unpack_masks(fx[f"{i}_masks"], case["n"], case["h"], case["w"], p["shadow_value"])
        assert np.array_equal(back, masks), case["name"]
    for t in case["bg"]:
        got, want = KC.stored_background(case, bgs[t]), fx[f"{i}_bg{t}"]
        assert got.dtype == want.dtype and np.array_equal(got, want), (case["name"], t)
    assert model[4] == KC.join_state(fx[f"{i}_state"]), (case["name"], hex(model[4]))


@pytest.mark.parametrize("i", range(KC.NCASES))
def test_the_periods_of_math_log_equal_those_recorded(fx, i):
    # the driver evaluates apply()'s expressions with the reference build's log
    got = KO.expected(i)[4]
    assert got.shape == (KC.cases()[i]["n"], 3) and np.array_equal(got, fx[f"{i}_periods"]), KC.label(i)


def test_the_branches_the_sequences_take():
    assert KO.expected(0)[3] == BASE_COUNTS
    total = dict.fromkeys(KO.COUNT_KEYS, 0)
    for i in range(KC.NCASES):
        for k, v in KO.expected(i)[3].items():
            total[k] += v
    assert total == TOTAL_COUNTS
    assert all(v > 0 for v in total.values())


def test_the_sequence_holds_what_the_cases_need():
    f = KC.case_frames(KC.cases()[0])
    assert f.shape == (KC.NFRAMES, KC.H, KC.W) and f.dtype == np.uint8
    assert not f[:, :, :8].any()  # the shadow test's zero denominator
    c3 = KC.case_frames(KC.cases()[2])
    assert (c3[..., 0] != c3[..., 1]).any() and not c3[:, :, :8].any()
    # the base sequence walks the periods: fills with a step per four values (1, 2, 4, 8) and through DivStruct
    fills = KO.expected(0)[5]
    assert sorted({d for _, _, d, _ in fills}) == [1, 2, 3, 4, 5, 6, 7, 8, 13]
    assert {m for _, _, _, m in fills} == {"small", "div"} and KO.expected(0)[3]["long_updates"] > 0
    # a range above 256 needs that many frames: the long case has one DivStruct fill and one power-of-two fill
    # there, both of which saturate
    last = KC.NCASES - 1
    assert KO.periods_of(KC.LONG_RATE, 1) == (327, 512, 1266)
    assert KO.expected(last)[5] == ((327, "short", 327, "div"), (512, "mid", 512, "bits"))
    nxt = KO.expected(last)[2][2]
    assert (nxt[0] == 255).sum() > 1 and (nxt[1] == 255).sum() > 1
    # the history-20000 case never reaches its periods: no fill after the first frame's
    assert KO.expected(15)[5] == () and KO.expected(15)[4][-1].min() > 256
    # 67 x 23 = 1541 values: one full block and a tail of 129 groups and one single value
    assert 67 * 23 == 1024 + 4 * 129 + 1


def test_randu_counts_its_steps():
    # a power of two up to 256 costs a step per group of four and one per value of a block's tail, d = 1 included
    for d, total, steps in ((1, 1541, 256 + 129 + 1), (4, 1024, 256), (256, 7, 1 + 3), (512, 5, 5), (3, 1541, 1541)):
        x = 0xffffffff
        for _ in range(steps):
            x = KO.rng_next(x)
        vals, state = KO.randu(0xffffffff, d, total)
        assert state == x and vals.max() <= min(d - 1, 255), d
