"""The masked-GFTT yardstick (tests/_gftt_mask_oracle.py) on the CPU: it equals
the oracle without a mask, meets the conditions that keep a masked GPU case
from passing by doing nothing, and reproduces what the real reference returned
(tests/golden/reference_gftt_mask.npz)."""
import numpy as np
import pytest

import _gftt_mask_cases as MC
import _gftt_mask_oracle as MO
import _oracle as O
import _reference_cases as RC

CROPS = [(0, 0, 160, 120), (300, 200, 77, 33), (250, 200, 64, 48), (0, 0, 3, 3), (5, 5, 2, 50)]
# (maxCorners, quality, minDistance, block, harris)
PARAMS = [(256, .01, 3.0, 3, False), (1000, .01, 0.0, 3, False), (64, .05, 8.0, 5, True), (300, .001, 2.5, 2, False),
          (40, 1.5, 1.0, 3, True)]
BASE = (256, .01, 3.0)


@pytest.fixture(scope="module")
def bb():
    return RC.basketball()[0]


@pytest.fixture(scope="module")
def synth():
    return O.synth(20261015, 640, 480, 32, 0, 1)[0][0]


def images(bb, synth):
    return [np.ascontiguousarray(bb[y:y + h, x:x + w]) for x, y, w, h in CROPS] + [synth]


def crop(img, roi):
    x, y, w, h = roi
    return np.ascontiguousarray(img[y:y + h, x:x + w])


def post_filter(corners, mask):
    return corners[mask[corners[:, 1].astype(int), corners[:, 0].astype(int)] != 0]


@pytest.mark.parametrize("prm", PARAMS)
def test_unmasked_equals_oracle(bb, synth, prm):
    maxc, q, md, block, harris = prm
    for img in images(bb, synth):
        ref = O.gftt_ex(img, maxc, q, md, block, harris, 0.04)
        assert np.array_equal(MO.gftt_masked(img, None, maxc, q, md, block, harris), ref), (img.shape, prm)


@pytest.mark.parametrize("prm", PARAMS)
def test_ones_is_unmasked_and_zero_is_empty(bb, synth, prm):
    maxc, q, md, block, harris = prm
    for img in images(bb, synth)[:5]:
        h, w = img.shape
        ref = O.gftt_ex(img, maxc, q, md, block, harris, 0.04)
        assert np.array_equal(MO.gftt_masked(img, MC.ones(w, h), maxc, q, md, block, harris), ref)
        assert len(MO.gftt_masked(img, MC.zero(w, h), maxc, q, md, block, harris)) == 0


def test_hole_lowers_the_maximum(bb):
    img = crop(bb, (0, 0, 160, 120))
    m = MC.hole(img)
    resp = MO.response(img)
    assert MO.masked_max(resp, m) < MO.masked_max(resp, None)
    got = MO.gftt_masked(img, m, *BASE)
    assert len(got) == 80
    assert not np.array_equal(got, post_filter(O.gftt_ex(img, *BASE), m))


@pytest.mark.parametrize("mode", [(3, False), (5, True)])
@pytest.mark.parametrize("where", ["basketball", "synth"])
def test_ring_maximum_is_on_the_border(bb, synth, where, mode):
    block, harris = mode
    img = crop(bb, (0, 0, 160, 120)) if where == "basketball" else crop(synth, (100, 100, 113, 90))
    m = MC.ring(img, block, harris)
    h, w = img.shape
    rim = MC.ring_only(w, h)
    resp = MO.response(img, block, harris)
    assert MO.masked_max(resp, m) == MO.masked_max(resp, rim)
    inner = m.copy()
    inner[rim != 0] = 0  # a maximum taken over interior pixels only sees this mask
    assert not np.array_equal(MO.gftt_masked(img, m, *BASE, block, harris),
                              MO.gftt_masked(img, inner, *BASE, block, harris))


def test_checker_is_applied_before_the_walk(bb):
    img = crop(bb, (300, 200, 77, 33))
    m = MC.checker(77, 33)
    assert not np.array_equal(MO.gftt_masked(img, m, *BASE), post_filter(O.gftt_ex(img, *BASE), m))


def test_mask_packing_round_trip(bb):
    img = crop(bb, (300, 200, 77, 33))
    for kind in MC.KINDS:
        m = MC.make(kind, img)
        assert np.array_equal(MC.unpack_mask(*MC.pack_mask(m), 77, 33), m), kind


def test_reproduces_reference_recordings():
    fx = MC.fixture()
    assert str(fx["state"]) in ("both", "noavx2")
    cases, entries = MC.cases(), MC.masks()
    assert np.array_equal(fx["case_mask"], [c[1] for c in cases])
    masks = [MC.fixture_mask(fx, m) for m in range(len(entries))]
    for m, e in enumerate(entries):  # the recorded masks are the generators'
        assert np.array_equal(masks[m], MC.mask_of(e)), e
    n_nonempty = 0
    for i, (r, m, maxc, q, md, block, harris) in enumerate(cases):
        got = MO.gftt_masked(MC.roi_image(r), masks[m], maxc, q, md, block, bool(harris), MC.HARRIS_K)
        assert np.array_equal(got, got.astype(np.uint16))
        RC.assert_pinned(got.astype(np.uint16), fx[f"{i}_c"], f"case {i}: {cases[i]} {entries[m]}")
        n_nonempty += len(got) > 0
    assert n_nonempty >= len(cases) // 2
