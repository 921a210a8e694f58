"""The numpy restatement of cv::cornerSubPix (tests/_subpix_oracle.py) against the
real function's recorded outputs (tests/golden/reference_subpix.npz), the window
mask of tbdk_corner_sub_pix_mask against both, and what the recorded cases
contain, so that no GPU test of tests/test_gpu_subpix.py passes emptily.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import _subpix_cases as SC
import _subpix_oracle as SO


@pytest.fixture(scope="module")
def fx():
    return SC.fixture()


@pytest.fixture(scope="module")
def runs(fx):
    """per case: (refined points of the restatement, its per-point info)"""
    out = []
    for name, depth, win, zero, crit in SC.cases():
        info = {}
        out.append((SO.corner_sub_pix(SC.image(name, depth), fx[f"pts_{name}"], win, zero, crit, info), info))
    return out


def test_fixture_layout(fx):
    assert str(fx["state"]) == "both"  # no dispatched code in cornerSubPix / getRectSubPix
    assert len(SC.cases()) == 52
    for i, (name, *_rest) in enumerate(SC.cases()):
        assert fx[f"{i}_c"].dtype == np.float32 and fx[f"{i}_c"].shape == fx[f"pts_{name}"].shape, SC.label(i)
    assert {n: len(fx[f"pts_{n}"]) for n, *_ in SC.IMAGES} == {"bb": 246, "n37": 198, "n130": 530, "n15": 26, "n25": 84}


def test_restatement_equals_every_recording(fx, runs):
    for i, (got, _) in enumerate(runs):
        ref = fx[f"{i}_c"]
        bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(1))
        assert bad.size == 0, (SC.label(i), f"{bad.size} of {len(ref)} points differ, first", bad[:8].tolist())


def test_expf_is_glibcs(fx):
    t = SC.exp_table(fx)
    numpy_differs = 0
    for w in range(1, 16):
        assert np.array_equal(SO.exp_axis(w)[w:].view(np.uint32), t[w].view(np.uint32)), w
        assert np.array_equal(SO.exp_axis(w)[w::-1].view(np.uint32), t[w].view(np.uint32)), w  # symmetric
        x = np.arange(w + 1, dtype=np.float32) / np.float32(w)
        numpy_differs += int((np.exp(-x * x).view(np.uint32) != t[w].view(np.uint32)).sum())
    assert numpy_differs > 0  # the trap is real: numpy's float32 exp would not have passed


def lib_mask(win, zero):
    from opencv_amd import _lib

    prm = _lib.SubpixParams(win[0], win[1], zero[0], zero[1], 3, 20, 0.03)
    out = np.full((2 * win[1] + 1, 2 * win[0] + 1), np.nan, np.float32)
    rc = _lib.load().tbdk_corner_sub_pix_mask(C.byref(prm), out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_library_mask_equals_restatement_and_table(fx):
    t = SC.exp_table(fx)
    for w in range(1, 16):
        for h in (w, 16 - w):
            rc, m = lib_mask((w, h), (-1, -1))
            assert rc == 0
            assert np.array_equal(m.view(np.uint32), SO.window_mask((w, h)).view(np.uint32)), (w, h)
            # the centre row and column are the recorded exponentials themselves (the other factor is expf(0) = 1)
            assert np.array_equal(m[h, w:].view(np.uint32), t[w].view(np.uint32)), (w, h)
            assert np.array_equal(m[h:, w].view(np.uint32), t[h].view(np.uint32)), (w, h)
    zones = sorted({(win, zero) for _, _, win, zero, _ in SC.cases()} |
                   {((5, 5), (0, 0)), ((5, 5), (4, 4)), ((5, 5), (4, 5)), ((5, 5), (-1, 2)), ((10, 15), (9, 14)),
                    ((10, 15), (10, 3)), ((1, 1), (0, 0)), ((1, 1), (1, 0))})
    zeroed = 0
    for win, zero in zones:
        rc, m = lib_mask(win, zero)
        assert rc == 0
        ref = SO.window_mask(win, zero)
        assert np.array_equal(m.view(np.uint32), ref.view(np.uint32)), (win, zero)
        zeroed += int((m == 0).any())
    assert zeroed == 8 and len(zones) == 17  # zones applied; the others (negative or as large as the window) ignored


def test_library_mask_rejects_bad_windows():
    from opencv_amd import _lib

    for win in ((0, 5), (5, 0), (16, 5), (5, 16), (-1, -1)):
        prm = _lib.SubpixParams(win[0], win[1], -1, -1, 3, 20, 0.03)
        buf = np.zeros((33, 33), np.float32)
        assert _lib.load().tbdk_corner_sub_pix_mask(C.byref(prm), buf.ctypes.data_as(C.c_void_p)) == _lib.TBDK_EINVAL


def test_recorded_cases_cover_the_paths(fx, runs):
    """counted on the restatement's run of the recorded inputs (which equals the
    recordings, above): every stop and every patch path occurs"""
    tot = {k: sum(int(info[k].sum()) for _, info in runs) for k in ("det", "left", "capped", "reverted", "border8")}
    assert tot == {"det": 46, "left": 53, "capped": 8302, "reverted": 4073, "border8": 3031}, tot
    # 8-bit patches strictly inside the image too (the `prev` path), not only border ones
    n8 = sum(len(fx[f"pts_{name}"]) for name, depth, *_ in SC.cases() if depth == "8u")
    assert n8 == 7064 and tot["border8"] < n8
    # a point in n130's constant square stops on det at its first iteration
    i = SC.cases().index(("n130", "8u", *SC.LKDEMO))
    info = runs[i][1]
    k = len(fx["pts_n130"]) - len(SC.special_points("n130")) + 10  # the square's centre
    assert info["det"][k] and info["iters"][k] == 0
    assert np.array_equal(fx[f"{i}_c"][k], fx["pts_n130"][k])
    # (2, ., 0.001) runs to the cap of 100, (1, 1000, .) too, (3, 0, -1) makes one iteration
    by_crit = {}
    for (name, depth, win, zero, crit), (_, info) in zip(SC.cases(), runs):
        by_crit.setdefault(crit, []).append(int(info["iters"].max()))
    assert max(by_crit[(2, 0, 0.001)]) == 100 and max(by_crit[(1, 1000, 0.0)]) == 100
    assert max(by_crit[(3, 0, -1.0)]) == 1 and max(by_crit[(1, 1, 0.0)]) == 1 and max(by_crit[(3, 20, 0.03)]) == 20


def test_basketball_corners_move(fx):
    """lkdemo's call on the basketball crop's own GFTT corners: more than half leave their integer start"""
    i = SC.cases().index(("bb", "8u", *SC.LKDEMO))
    pts, ref = fx["pts_bb"], fx[f"{i}_c"]
    ng = (len(pts) - len(SC.special_points("bb"))) // 2
    assert np.array_equal(pts[:ng], np.round(pts[:ng]))  # integer pixel positions
    moved = int((ref[:ng] != pts[:ng]).any(1).sum())
    assert (ng, moved) == (118, 67), (ng, moved)
    assert 2 * moved > ng


def test_rows_and_counts_of_the_restatement():
    img = SC.image("n37")
    rng = np.random.default_rng(5)
    c = (rng.random((4, 6, 2)) * [30, 50] + 3).astype(np.float32)
    counts = np.array([6, 0, -1, 9], np.int32)
    out = SO.refine_rows(img, c, counts, (5, 5))
    assert np.array_equal(out[1], c[1]) and np.array_equal(out[2], c[2])
    assert np.array_equal(out[0], SO.corner_sub_pix(img, c[0], (5, 5)))
    assert np.array_equal(out[3], SO.corner_sub_pix(img, c[3], (5, 5)))  # 9 clamps to the row's 6
    assert not np.array_equal(out[0], c[0])
