"""The CPU oracle against tests/golden/reference_gftt_frame.npz (goodFeaturesToTrack
on whole frames, recorded from the real reference; tests/_gftt_frame_cases.py):
O.gftt / O.gftt_ex give every recorded 8-bit list, the numpy restatements the
masked and the 32F one, and each case marked as overflowing really has more
candidates than the LDS selection holds, so tests/test_gpu_gftt_frame.py cannot
pass through that path."""
import numpy as np
import pytest

import _gftt_f32_oracle as O32
import _gftt_frame_cases as WC
import _gftt_mask_oracle as MO
import _oracle as O


@pytest.fixture(scope="module")
def fx():
    return WC.fixture()


def test_fixture_layout(fx):
    assert str(fx["state"]) == "noavx2"
    assert len(fx["other_ints_equal"]) == len(WC.CASES)
    for i in range(len(WC.CASES)):
        c = fx[f"{i}_c"]
        assert c.dtype == np.int16 and c.ndim == 2 and c.shape[1] == 2 and len(c) <= WC.CASES[i][2], WC.label(i)


@pytest.mark.parametrize("i", range(len(WC.CASES)), ids=WC.label)
def test_oracle_equals_recording(fx, i):
    name, mk, maxc, q, md, block, harris, _ = WC.CASES[i]
    img = WC.frame(name)
    if img.dtype == np.float32:
        got = O32.gftt(img, None, maxc, q, md, block, bool(harris), WC.HARRIS_K)
    elif mk != "none":
        got = MO.gftt_masked(img, WC.mask(mk, name), maxc, q, md, block, bool(harris), WC.HARRIS_K)
    elif block == 3 and not harris:
        got = O.gftt(img, maxc, q, md)
    else:
        got = O.gftt_ex(img, maxc, q, md, block, bool(harris), WC.HARRIS_K)
    want = WC.corners(fx, i)
    assert len(got) == len(want), (WC.label(i), len(got), len(want))
    assert np.array_equal(np.asarray(got, np.float32).reshape(-1, 2), want), WC.label(i)


def candidates(img, mask, q, block, harris):
    """the number of candidates goodFeaturesToTrack sorts: interior pixels above
    (float)(maxVal q), maxVal over the masked-in pixels, equal to their 3x3
    dilation of the thresholded map, masked in"""
    if img.dtype == np.float32:
        resp = O32.response(img, block, harris, WC.HARRIS_K)
    else:
        resp = MO.response(img, block, harris, WC.HARRIS_K)
    on = np.ones(resp.shape, bool) if mask is None else mask != 0
    thr = np.float32(np.float64(resp[on].max()) * q)
    t = np.where(resp > thr, resp, np.float32(0))
    h, w = t.shape
    d = t.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            p = np.pad(t, 1, constant_values=-np.inf)[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            d = np.maximum(d, p)
    c = (t != 0) & (t == d) & on
    return int(c[1:-1, 1:-1].sum())


@pytest.mark.parametrize("i", range(len(WC.CASES)), ids=WC.label)
def test_overflow_cases_overflow(i):
    name, mk, maxc, q, md, block, harris, over = WC.CASES[i]
    n = candidates(WC.frame(name), WC.mask(mk, name), q, block, bool(harris))
    assert (n > WC.LDS_CAP) == over, (WC.label(i), n)


def test_mixed_batch_rois_overflow_as_marked():
    """the two large ROIs of the GPU suite's mixed batch overflow the LDS selection, the others do not"""
    img, q = WC.frame("noise"), WC.MIXED_ROW[1]
    for x, y, w, h, over in WC.MIXED_ROIS:
        n = candidates(np.ascontiguousarray(img[y:y + h, x:x + w]), None, q, 3, False) if w >= 3 and h >= 3 else 0
        assert (n > WC.LDS_CAP) == over, ((x, y, w, h), n)


def test_tied_images_overflow():
    """the GPU suite's tie images have more candidates than the LDS selection holds at the quality they run at"""
    assert candidates(WC.tiled_noise(), None, 0.001, 3, False) > WC.LDS_CAP
    assert candidates(WC.tiled_block(), None, 0.5, 3, False) > WC.LDS_CAP
