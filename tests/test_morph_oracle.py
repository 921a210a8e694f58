"""CPU: the numpy restatement of erode / dilate / morphologyEx and getStructuringElement (tests/_morph_oracle.py)
against the outputs recorded from the real reference (tests/golden/reference_morph.npz, both dispatch states),
byte for byte or row CRC for row CRC."""
import numpy as np
import pytest

import _morph_cases as BC
import _morph_oracle as MO
import _reference_cases as RC

CASES = BC.cases()
ELEMENTS = BC.elements()


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("morph")


def test_the_fixture_holds_one_recording_for_both_dispatch_states(fx):
    # morph.simd.hpp is dispatched, but it is integer min / max: the two states' recordings were byte-identical
    assert str(fx["state"]) == "both"
    assert len(CASES) == len(fx["other_ints_equal"]) == 449 and fx["other_ints_equal"].all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: BC.label(i).replace(" ", "_"))
def test_restatement_equals_the_recorded_reference(fx, i):
    c = CASES[i]
    got = MO.morphology_ex(BC.image(c["w"], c["h"], c["content"]), c["op"], ELEMENTS[c["elem"]], c["anchor"], c["it"],
                           c["border"], c["bval"])
    RC.assert_pinned(got, fx[f"{i}_d"], BC.label(i))


def test_structuring_elements_equal_the_recorded_reference(fx):
    for k, (shape, kw, kh, anchor) in enumerate(BC.strel_cases()):
        e = MO.structuring_element(shape, (kw, kh), anchor)
        assert e.shape == (kh, kw) and np.array_equal(np.packbits(e), fx[f"strel_{k}"]), (shape, kw, kh, anchor)


def test_the_cases_hold_what_they_are_for():
    # One pass of the merged rectangle differs from iterating where the anchor is off-centre and the border
    # reflects (with a centred rectangle, and under BORDER_CONSTANT with any value, the two are the same image)
    img = BC.image(37, 23, "noise")
    e = np.ones((6, 4), np.uint8)
    merged = MO.morphology_ex(img, MO.ERODE, e, (0, 0), 2, MO.BORDER_REFLECT)
    once = MO.morphology_ex(img, MO.ERODE, e, (0, 0), 1, MO.BORDER_REFLECT)
    assert not np.array_equal(merged, MO.morphology_ex(once, MO.ERODE, e, (0, 0), 1, MO.BORDER_REFLECT))
    assert any(c["elem"] == "rect4x6" and c["it"] == 2 and c["border"] == BC.REFLECT and c["anchor"] == (0, 0)
               for c in CASES)
    assert any(c["elem"] == "rect3x3" and c["it"] == 2 and c["bval"] == 0 and c["op"] == BC.ERODE for c in CASES)
    # an element with a zero at its anchor, even sizes, an image smaller than its element, every border and op
    z = ELEMENTS["arb6x5z"]
    assert z[z.shape[0] // 2, z.shape[1] // 2] == 0 and 0 < z.sum() < z.size
    assert {c["border"] for c in CASES} == {0, 1, 2, 4} and {c["op"] for c in CASES} == {0, 1, 2, 3}
    assert {c["bval"] for c in CASES} == {-1, 0, 100, 255} and {c["it"] for c in CASES} == {0, 1, 2, 3, 15}
    assert {(c["w"], c["h"]) for c in CASES} == set(BC.SIZES) and any(c["inplace"] for c in CASES)
    assert set(np.unique(BC.image(37, 23, "mask"))) == {0, 127, 255}
