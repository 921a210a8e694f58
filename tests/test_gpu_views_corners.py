"""Corner maps and GFTT on 8-bit pitched, unaligned views (tests/_views.py):
the source is an interior window of a noise-filled allocation in every layout,
the float response map a window too.  Oracles and criteria are those of
test_gpu_gftt.py and test_gpu_gftt_frame.py: bit-exact maps, identical corner
lists."""
import ctypes as C

import numpy as np
import pytest
import torch

import _oracle as O
import _views as V

pytestmark = pytest.mark.gpu

LAYOUTS = list(V.LAYOUTS)


def dwin(arr, layout, seed=0):
    return V.window(arr, layout, seed, device="cuda")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(61093).integers(0, 256, (61, 93), dtype=np.uint8)


@pytest.fixture(scope="module")
def response_refs(noise):
    """computed once: O.min_eig and O.corner_response for every mode below"""
    refs = {"eig": O.min_eig(noise)}
    for block in (3, 5):
        for harris in (False, True):
            refs[block, harris] = O.corner_response(noise, block, harris, 0.04)
    return refs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dlayout", ["odd_both", "a16_pitched"])
def test_corner_maps_on_views(gpu, noise, response_refs, layout, dlayout):
    """tbdk_corner_min_eig_val and tbdk_corner_response (block 3 and 5, Harris on
    and off) at (61, 93), source and float destination both windows: the map is
    bit-exact and the destination's guards stay; with a forced re-walk
    (gftt_eig_redo) too, as test_corner_min_eig_matches_oracle"""
    h, w = noise.shape
    ps, vs = dwin(noise, layout, seed=1)
    s0 = V.snapshot(ps)
    lib = gpu.lib

    def run(call, ref, tag):
        pd, vd = dwin(np.full((h, w), -3.5, np.float32), dlayout, seed=2)
        d0 = V.snapshot(pd)
        st = call(vd)
        torch.cuda.synchronize()
        assert st == 0, tag
        assert np.array_equal(vd.cpu().numpy().view(np.uint32), ref.view(np.uint32)), tag
        assert V.guards_intact(pd, d0, vd), tag

    for redo in (0, 1):
        gpu.set_option("gftt_eig_redo", redo)
        try:
            run(lambda vd: lib.tbdk_corner_min_eig_val(gpu.handle, vs.data_ptr(), w, h, vs.stride(0), vd.data_ptr(),
                                                       vd.stride(0) * 4, _stream()), response_refs["eig"], f"eig {redo}")
        finally:
            gpu.set_option("gftt_eig_redo", 0)
    for block in (3, 5):
        for harris in (False, True):
            run(lambda vd: lib.tbdk_corner_response(gpu.handle, vs.data_ptr(), w, h, vs.stride(0), vd.data_ptr(),
                                                    vd.stride(0) * 4, block, int(harris), 0.04, _stream()),
                response_refs[block, harris], f"block {block} harris {harris}")
    assert torch.equal(ps, s0)


@pytest.fixture(scope="module")
def roi_case():
    fr, _ = O.synth(20261015, 320, 240, 12, 0, 1)
    rois = [(0, 0, 120, 90), (243, 171, 77, 69), (100, 60, 77, 33)]  # the second ends at the frame's last row and column
    modes = [(256, 0.01, 3.0, 3, False), (500, 0.001, 0.0, 5, True)]
    refs = [O.gftt_rois(fr[0], rois, m, q, d, b, hs, 0.04) for m, q, d, b, hs in modes]
    assert all(len(r) > 0 for ref in refs for r in ref)
    return np.ascontiguousarray(fr[0]), rois, modes, refs


@pytest.mark.parametrize("layout", LAYOUTS)
def test_gftt_rois_on_views(gpu, roi_case, layout):
    """GoodFeaturesToTrackDetector over three ROIs of a view, one touching the
    frame's first row and column and one its last: the oracle's corner lists
    (O.gftt_rois, as test_gftt_rois_match_oracle), for the 3x3 minimum eigenvalue
    and for a 5x5 Harris response"""
    from opencv_amd import klt

    img, rois, modes, refs = roi_case
    parent, view = dwin(img, layout, seed=3)
    before = V.snapshot(parent)
    for (maxc, q, md, block, harris), ref in zip(modes, refs):
        det = klt.GoodFeaturesToTrackDetector(maxc, q, md, block, harris, 0.04)
        c, n = det.detect_rois(view, rois)
        torch.cuda.synchronize()
        c, n = c.cpu().numpy(), n.cpu().numpy()
        for i, r in enumerate(ref):
            assert n[i] == len(r), f"roi {i}: count {n[i]} vs {len(r)}"
            assert np.array_equal(c[i, :n[i]], r), f"roi {i}: corners differ"
    assert torch.equal(parent, before)


@pytest.fixture(scope="module")
def frame_case():
    img = np.random.default_rng(120160).integers(0, 256, (120, 160), dtype=np.uint8)
    return img, O.gftt(img, 100000, 0.01, 0.0), O.gftt(img, 100000, 0.01, 3.0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_gftt_whole_frame_on_views(gpu, frame_case, layout):
    """GoodFeaturesToTrackDetector.detect on a (120, 160) noise view with no
    corner limit in reach (the library wants max_corners > 0, so 100000 stands
    for the reference's "0 = all"): an accepted list longer than the LDS
    selection holds, so the wide selection path of test_gpu_gftt_frame.py runs;
    the same list as O.gftt, with and without a minimum distance"""
    from opencv_amd import klt

    img, all_corners, spaced = frame_case
    assert len(all_corners) > 1000
    parent, view = dwin(img, layout, seed=4)
    before = V.snapshot(parent)
    for md, want in ((0.0, all_corners), (3.0, spaced)):
        got = klt.GoodFeaturesToTrackDetector(100000, 0.01, md).detect(view)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert len(got) == len(want)
        assert np.array_equal(got, np.asarray(want, np.float32).reshape(-1, 2))
    assert torch.equal(parent, before)


def test_pitch_below_the_row_is_refused(gpu, noise):
    """pitch < row, dst_pitch < 4 * width: TBDK_EINVAL and an untouched destination"""
    from opencv_amd import _lib

    h, w = noise.shape
    ps, vs = dwin(noise, "odd_both")
    pd, vd = dwin(np.zeros((h, w), np.float32), "odd_both", seed=1)
    d0 = V.snapshot(pd)
    lib, s = gpu.lib, _stream()
    for sp, dp in ((w - 1, vd.stride(0) * 4), (vs.stride(0), 4 * w - 4)):
        assert lib.tbdk_corner_min_eig_val(gpu.handle, vs.data_ptr(), w, h, sp, vd.data_ptr(), dp, s) == _lib.TBDK_EINVAL
        assert lib.tbdk_corner_response(gpu.handle, vs.data_ptr(), w, h, sp, vd.data_ptr(), dp, 5, 1, 0.04, s) == \
            _lib.TBDK_EINVAL
    prm = _lib.GfttParams(10, 0.01, 0.0, 3, 0, 0.04)
    roi = (_lib.Roi * 1)(_lib.Roi(0, 0, w, h))
    corners = torch.full((1, 10, 2), -1.0, device="cuda")
    counts = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    assert lib.tbdk_gftt_rois(gpu.handle, vs.data_ptr(), w, h, w - 1, roi, 1, C.byref(prm), corners.data_ptr(),
                              counts.data_ptr(), s) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(pd, d0) and int(counts[0]) == -5 and bool((corners == -1.0).all())
