"""CPU: the numpy restatement of the 8-bit GaussianBlur and of threshold (tests/_blur_oracle.py) against the
recordings of the real reference (tests/golden/reference_blur.npz, reference_threshold.npz), bit for bit, with the
counts of the branches the cases take, so that the cases cannot go soft."""
import numpy as np
import pytest

import _blur_cases as UC
import _blur_oracle as BO
import _reference_cases as RC


@pytest.fixture(scope="module")
def blur_fx():
    return RC.fixture("blur")


@pytest.fixture(scope="module")
def thresh_fx():
    return RC.fixture("threshold")


def test_both_dispatch_states_recorded_identical(blur_fx, thresh_fx):
    assert str(blur_fx["state"]) == "both" and str(thresh_fx["state"]) == "both"
    assert blur_fx["other_ints_equal"].all() and thresh_fx["other_ints_equal"].all()


def test_coefficients_equal_the_recorded_sweep(blur_fx):
    pairs = UC.sweep_pairs()
    assert len(pairs) >= 2000 and np.array_equal(blur_fx["coef_pairs"], np.array(pairs, np.float64))
    resp, pos, sums = blur_fx["coef_resp"], 0, []
    for n, sigma in pairs:
        win = resp[pos:pos + 2 * n]
        pos += 2 * n
        k = BO.gaussian_kernel_u8(n, sigma)
        assert np.array_equal(UC.sweep_decode(win, n), k), (n, sigma)
        sums.append(int(k.sum()))
    assert pos == resp.size
    sums = np.array(sums)
    # the sums the recording script printed (tools/record_reference_cases.md): the saturation of the row sums is live
    assert (int((sums >= 258).sum()), int(sums.max()), int(sums.min())) == (237, 262, 250)
    assert pairs[int(sums.argmax())] == (27, 0.3 + 93 * UC.SWEEP_STEP)


def test_kernel_table_and_size_rules():
    k = UC.kernels()
    assert int(BO.gaussian_kernel_u8(11, 3.5).sum()) >= 257
    assert int(BO.gaussian_kernel_u8(*k["25@max"][::2][:2]).sum()) == max(
        int(BO.gaussian_kernel_u8(25, s).sum()) for n, s in UC.sweep_pairs() if n == 25)
    assert [len(a) for a in BO.plan(40, 40, (0, 0), 1.0, 0, BO.REFLECT_101)] == [7, 7]
    assert [len(a) for a in BO.plan(40, 40, (0, 0), 2.2, 0, BO.REFLECT_101)] == [15, 15]
    assert [len(a) for a in BO.plan(40, 40, (0, 5), 5.0, 0, BO.REFLECT_101)] == [31, 5]
    assert BO.plan(1, 1, (5, 5), 1.0, 0, BO.REFLECT_101) is None
    assert [len(a) for a in BO.plan(1, 1, (5, 5), 1.0, 0, BO.CONSTANT)] == [5, 5]
    assert [len(a) for a in BO.plan(9, 1, (5, 7), 1.0, 0, BO.WRAP)] == [5, 1]
    assert [len(a) for a in BO.plan(40, 40, (3, -2), 1.0, 0, BO.REFLECT_101)] == [3, 7]  # any size <= 0 is automatic
    for bad, sigma in (((4, 3), 1.0), ((33, 3), 1.0), ((3, 33), 1.0), ((0, 0), 0.0), ((0, 3), -1.0)):
        with pytest.raises(ValueError):
            BO.plan(40, 40, bad, sigma, 0, BO.REFLECT_101)
    with pytest.raises(ValueError):
        BO.plan(40, 40, (0, 0), 5.2, 0, BO.REFLECT_101)  # the automatic size is 33


def test_blur_equals_every_recording(blur_fx):
    kernels, counts = UC.kernels(), BO.new_counts()
    rows = UC.cases()
    assert len(rows) == 363
    for i, c in enumerate(rows):
        kw, kh, sx, sy = kernels[c["kernel"]]
        got = BO.gaussian_blur(UC.case_image(c), (kw, kh), sx, sy, c["border"], counts)
        RC.assert_pinned(got, blur_fx[f"{i}_d"], UC.label(i))
    print("blur branch counts:", counts)
    assert counts["sat_h"] == SAT_H and counts["clipped"] == CLIPPED
    assert counts["border_terms"] == BORDER_TERMS


# the branches the 363 cases take through the restatement: row sums saturated at 65535, outputs clipped at 255,
# terms fetched by borderInterpolate (left out, under BORDER_CONSTANT) per border mode
SAT_H = 14578
CLIPPED = 13138
BORDER_TERMS = {0: 273748, 1: 228362, 2: 86838, 3: 201150, 4: 753690}


def test_threshold_equals_every_recording(thresh_fx):
    counts = BO.new_counts()
    rows = UC.thresh_cases()
    assert len(rows) == 250
    nan_cases = 0
    for i, c in enumerate(rows):
        img = UC.thresh_image(c)
        if c["kind"] == "f32":
            t, got = BO.threshold_f32(img, c["thresh"], c["maxval"], c["type"])
            got = got.view(np.int32)
            nan_cases += int(np.isnan(img).any())
        else:
            t, got = BO.threshold_u8(img, c["thresh"], c["maxval"], c["type"], counts)
        RC.assert_pinned(got, thresh_fx[f"{i}_d"], UC.thresh_label(i))
        assert np.float64(t).view(np.int64) == thresh_fx[f"{i}_t"][0], UC.thresh_label(i)
    # thresholds -1, 255 and 300 of the seven: 2 images x 5 types x 3 x 3 maxvals
    assert counts["ithresh_special"] == 90 and nan_cases == 30


def test_otsu_values(thresh_fx):
    rows = UC.thresh_cases()
    seen = {}
    for i, c in enumerate(rows):
        if c["kind"] == "otsu":
            seen[c["image"]] = float(thresh_fx[f"{i}_t"].view(np.float64)[0])
            assert seen[c["image"]] == BO.otsu(UC.thresh_image(c))
    assert set(seen) == set(UC.OTSU_IMAGES)
    assert seen["constant"] == 0.0 and seen["two"] == 12.0 and 70 <= seen["bimodal"] < 170
    assert len(set(seen.values())) >= 4
