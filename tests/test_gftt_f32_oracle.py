"""The numpy restatement of cornerMinEigenVal / cornerHarris /
goodFeaturesToTrack on CV_32F images (tests/_gftt_f32_oracle.py) against what the
real reference returned (tests/golden/reference_gftt_f32.npz, recorded by
tools/record_reference_cases.py): every map and every corner list bit for bit;
and the properties the GPU tests rely on: the `hdr` images defeat every fresh
start of the eigenvalue walk, the `small` ones none, and a uint16 image is its
float32 conversion."""
import numpy as np
import pytest

import _gftt_f32_cases as FC
import _gftt_f32_oracle as O32
import _reference_cases as RC


@pytest.fixture(scope="module")
def fx():
    return FC.fixture()


def test_fixture_layout(fx):
    n = len(FC.map_cases()) + len(FC.list_cases())
    assert str(fx["state"]) == "noavx2"
    assert int(fx["nmaps"]) == len(FC.map_cases())
    for k in ("other_ints_equal", "other_share", "other_maxabs"):
        assert fx[k].shape == (n,), k
    # the default dispatch changes words of some blockSize 3 and 5 maps, never a corner list
    assert fx["other_ints_equal"].all()
    assert (fx["other_share"] < 1).any() and (fx["other_share"][len(FC.map_cases()):] == 1).all()
    assert all(f"{i}_e" in fx for i in range(len(FC.map_cases())))
    assert all(f"{i}_c" in fx for i in range(len(FC.map_cases()), n))


def test_maps_equal_the_recordings(fx):
    for i, (h, w, kind, block, harris) in enumerate(FC.map_cases()):
        with np.errstate(over="ignore", invalid="ignore"):
            e = O32.response(FC.map_image(h, w, kind), block, bool(harris), FC.HARRIS_K)
        assert e.dtype == np.float32 and e.shape == (h, w)
        RC.assert_pinned(e, fx[f"{i}_e"], f"case {i}: {(h, w, kind, block, harris)}")


def test_lists_equal_the_recordings(fx):
    nm = len(FC.map_cases())
    total = 0
    for j, (kind, r, mk, maxc, q, md, block, harris) in enumerate(FC.list_cases()):
        img = FC.list_image(kind, r)
        h, w = img.shape
        c = O32.gftt(img, FC.list_mask(mk, w, h), maxc, q, md, block, bool(harris), FC.HARRIS_K)
        assert np.array_equal(c, c.astype(np.uint16))
        RC.assert_pinned(c.astype(np.uint16), fx[f"{nm + j}_c"], f"case {nm + j}: {FC.list_cases()[j]}")
        if mk == "zero":
            assert len(c) == 0
        total += len(c)
    assert total > 5000


def wide_strips(w):
    """the aligned 56-column strips of a w-column image that hold at least FC.HDR_MIN_STRIP columns"""
    return [s for s in range((w + O32.STRIP - 1) // O32.STRIP) if min(w - s * O32.STRIP, O32.STRIP) >= FC.HDR_MIN_STRIP]


# the ROI list of the GPU tests (tests/test_gpu_gftt_f32.py builds on it), as isolated images
GPU_ROIS = [(0, 0, 160, 120), (300, 200, 77, 33), (250, 200, 64, 48), (401, 203, 57, 40), (20, 30, 56, 20),
            (21, 31, 112, 9), (10, 400, 113, 80), (33, 77, 58, 5), (600, 440, 3, 3), (5, 5, 2, 50), (100, 100, 1, 1),
            (77, 231, 90, 39)]


def test_hdr_defeats_every_fresh_start_and_small_none():
    """where the kernel cuts its row segments does not matter: on `hdr` every row
    >= 2 of every strip (of at least HDR_MIN_STRIP columns) starts a segment on
    another sum than the running one, on `small` no row of any strip does"""
    checked = 0
    for h, w in FC.MAP_SHAPES:
        hdr, small = FC.map_image(h, w, "hdr"), FC.map_image(h, w, "small")
        assert np.isfinite(hdr).all()
        assert not O32.fresh_start_mismatch(small).any(), (w, h)
        mm = O32.fresh_start_mismatch(hdr)
        for s in wide_strips(w):
            assert mm[s, 2:].all(), (w, h, s)
            checked += max(h - 2, 0)
    f = FC.frame("hdr")
    for x, y, w, h in GPU_ROIS + FC.LIST_ROIS:
        mm = O32.fresh_start_mismatch(f[y:y + h, x:x + w])
        for s in wide_strips(w):
            assert mm[s, 2:].all(), (x, y, w, h, s)
            checked += max(h - 2, 0)
    assert checked > 1000
    mm = O32.fresh_start_mismatch(f)
    assert mm.shape == ((640 + 55) // 56, 480) and wide_strips(640) == list(range(12)) and mm[:, 2:].all()
    assert not O32.fresh_start_mismatch(FC.image("small", 640, 480, FC.FRAME_SEED)).any()
    # the content kinds are what they claim to be
    u = FC.frame("unit")
    assert u.dtype == np.float32 and 0 <= u.min() and u.max() < 1.01
    assert (np.frexp(u)[0] * 2 ** 24 % 2 == 1).mean() > 0.3  # full mantissas: the last bit is in use
    assert FC.frame("u16").dtype == np.uint16 and FC.frame("u16").max() > 60000
    ex = np.frexp(f)[1]
    assert ex.max() - ex.min() >= 24 and (f < 0).any() and (f > 0).any()


def test_u16_is_its_float_conversion():
    for h, w in FC.MAP_SHAPES:
        img = FC.map_image(h, w, "u16")
        assert img.dtype == np.uint16
        for block, harris in FC.MAP_MODES:
            a = O32.response(img, block, bool(harris), FC.HARRIS_K)
            b = O32.response(img.astype(np.float32), block, bool(harris), FC.HARRIS_K)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    img = FC.list_image("u16", 0)
    assert np.array_equal(O32.gftt(img, None, 256, .01, 3.0), O32.gftt(img.astype(np.float32), None, 256, .01, 3.0))


def test_oracle_rejects_other_types():
    with pytest.raises(AssertionError):
        O32.response(np.zeros((4, 4), np.uint8))
