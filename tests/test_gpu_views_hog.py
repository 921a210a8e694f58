"""HOG on pitched, unaligned views (tests/_views.py): the image of every stage
(resize, gradient, detect, detectMultiScale) is an interior window of a
noise-filled allocation, 1, 3 and 4 channels (offsets in whole pixels: one BGR
pixel puts the first byte at 3 mod 16), and every caller-supplied output
(resized image, gradient and bin planes) is a window whose guards must stay.
Oracles and criteria are test_gpu_hog.py's: bit-exact stages, equal detections."""
import ctypes as C

import numpy as np
import pytest
import torch

import _oracle as O
import _views as V
from test_gpu_hog import _bgr, _hog, _prm

pytestmark = pytest.mark.gpu

LAYOUTS = list(V.LAYOUTS)
# the gradient plane's pitch must be a multiple of 8 (float2 pixels): the layouts whose pitch is one
GRAD_LAYOUTS = {"a16_pitched": "a16_pitched", "vec4": "vec4", "odd_base": "odd_base", "odd_pitch": "vec4",
                "odd_both": "odd_base"}
# the bin plane's pitch must be even (uchar2 pixels)
BIN_LAYOUTS = dict({k: k for k in LAYOUTS}, odd_pitch="odd_both")


def dwin(arr, layout, seed=0):
    return V.window(arr, layout, seed, device="cuda")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("src,dst", [((97, 61), (31, 20)), ((50, 40), (123, 77))])
def test_resize_exact_on_views(gpu, layout, cn, src, dst):
    """tbdk_hog_resize, shrinking and enlarging ((w, h) sizes as in
    test_resize_exact_bit_exact), source and destination both windows"""
    img = _bgr(sum(src) + cn, *src, cn=cn)
    ps, vs = dwin(img, layout, seed=1)
    dlayout = LAYOUTS[(LAYOUTS.index(layout) + 3) % len(LAYOUTS)]
    shape = (dst[1], dst[0]) if cn == 1 else (dst[1], dst[0], cn)
    pd, vd = dwin(np.full(shape, 0xA5, np.uint8), dlayout, seed=2)
    s0, d0 = V.snapshot(ps), V.snapshot(pd)
    st = gpu.lib.tbdk_hog_resize(gpu.handle, vs.data_ptr(), src[0], src[1], vs.stride(0), cn, vd.data_ptr(), dst[0],
                                 dst[1], vd.stride(0), _stream())
    torch.cuda.synchronize()
    assert st == 0
    assert np.array_equal(vd.cpu().numpy(), O.hog_resize(img, dst))
    assert V.guards_intact(pd, d0, vd) and torch.equal(ps, s0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("w,h", [(130, 77), (6, 5)])
def test_gradient_on_views(gpu, layout, cn, w, h):
    """tbdk_hog_gradient with the image, the gradient plane (pitch a multiple of
    8) and the bin plane (an even pitch) all windows, gamma correction on and off"""
    img = _bgr(w * h + cn, w, h, cn=cn)
    ps, vs = dwin(img, layout, seed=1)
    s0 = V.snapshot(ps)
    for gamma, signed in ((True, False), (False, True)):
        hg = _hog(gpu)
        hg.setGammaCorrection(gamma)
        hg.setSignedGradient(signed)
        pg, vg = dwin(np.full((h, w, 2), -7.25, np.float32), GRAD_LAYOUTS[layout], seed=2)
        pq, vq = dwin(np.full((h, w, 2), 0xA5, np.uint8), BIN_LAYOUTS[layout], seed=3)
        g0, q0 = V.snapshot(pg), V.snapshot(pq)
        assert (vg.stride(0) * 4) % 8 == 0 and vg.stride(0) > 2 * w and vq.stride(0) % 2 == 0
        st = gpu.lib.tbdk_hog_gradient(gpu.handle, vs.data_ptr(), w, h, vs.stride(0), cn, C.byref(hg.p), vg.data_ptr(),
                                       vg.stride(0) * 4, vq.data_ptr(), vq.stride(0), _stream())
        torch.cuda.synchronize()
        assert st == 0
        og, oq = O.hog_gradient(img[..., :3] if cn == 4 else img, nbins=9, gamma=gamma, signed=signed)
        assert np.array_equal(vq.cpu().numpy(), oq)
        assert np.array_equal(vg.cpu().numpy(), og)
        assert V.guards_intact(pg, g0, vg) and V.guards_intact(pq, q0, vq)
    assert torch.equal(ps, s0)


@pytest.fixture(scope="module")
def detect_refs():
    """every window's score on the 200 x 150 image, computed once per channel count"""
    out = {}
    for cn in (1, 3):
        img = _bgr(11 + cn, 200, 150, cn=cn)
        prm = O.hog_params(win=(48, 96))
        from opencv_amd import hog

        svm = hog.HOG.create((48, 96)).getDefaultPeopleDetector()
        out[cn] = (img,) + tuple(O.hog_detect(img, prm, svm, hit_threshold=-1e9))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cn", [1, 3])
def test_detect_on_views(gpu, detect_refs, layout, cn):
    """HOG.detect with hit_threshold -1e9 (every window) on a 200 x 150 view:
    positions and double scores equal the oracle's"""
    img, oxy, osc = detect_refs[cn]
    parent, view = dwin(img, layout, seed=cn)
    before = V.snapshot(parent)
    hg = _hog(gpu, (48, 96))
    hg.setHitThreshold(-1e9)
    xy, sc = hg.detect(view, confidences=True)
    assert len(xy) == len(oxy) > 0
    assert np.array_equal(np.array(xy), oxy) and np.array_equal(np.array(sc), osc)
    assert torch.equal(parent, before)


MS_HIT, MS_LEVELS = -1.0, 6  # the oracle alone finds 8 (BGR) and 7 (BGRA) grouped detections at this threshold


@pytest.fixture(scope="module")
def multiscale_refs():
    from opencv_amd import hog

    svm = hog.HOG.create((48, 96)).getDefaultPeopleDetector()
    out = {}
    for cn in (3, 4):
        img = _bgr(20 + cn, 320, 240, cn=cn)
        r, w = O.hog_detect_multiscale(img[..., :3] if cn == 4 else img, O.hog_params(win=(48, 96)), svm,
                                       hit_threshold=MS_HIT, nlevels=MS_LEVELS, scale0=1.05, group_threshold=2)
        out[cn] = (img, sorted(zip(map(tuple, r.tolist()), w.tolist())))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cn", [3, 4])
def test_detect_multiscale_on_views(gpu, multiscale_refs, layout, cn):
    """HOG.detectMultiScale on a 320 x 240 view, 48 x 96 window, 6 levels: rects
    and weights equal O.hog_detect_multiscale's"""
    img, exp = multiscale_refs[cn]
    assert len(exp) > 0
    parent, view = dwin(img, layout, seed=cn)
    before = V.snapshot(parent)
    hg = _hog(gpu, (48, 96))
    hg.setNumLevels(MS_LEVELS)
    hg.setHitThreshold(MS_HIT)
    hg.setGroupThreshold(2)
    rects, wts = hg.detectMultiScale(view, confidences=True)
    assert sorted(zip(rects, wts)) == exp
    assert torch.equal(parent, before)


def test_pitch_below_the_row_is_refused(gpu):
    from opencv_amd import _lib

    w, h, cn = 130, 77, 3
    img = _bgr(5, w, h, cn=cn)
    ps, vs = dwin(img, "odd_both")
    hg = _hog(gpu, (48, 96))
    lib, s = gpu.lib, _stream()
    pd, vd = dwin(np.zeros((20, 31, cn), np.uint8), "odd_both", seed=1)
    pg, vg = dwin(np.zeros((h, w, 2), np.float32), "odd_base", seed=2)
    pq, vq = dwin(np.zeros((h, w, 2), np.uint8), "odd_both", seed=3)
    d0, g0, q0 = V.snapshot(pd), V.snapshot(pg), V.snapshot(pq)
    row = w * cn
    assert lib.tbdk_hog_resize(gpu.handle, vs.data_ptr(), w, h, row - 1, cn, vd.data_ptr(), 31, 20, vd.stride(0), s) == \
        _lib.TBDK_EINVAL
    assert lib.tbdk_hog_resize(gpu.handle, vs.data_ptr(), w, h, vs.stride(0), cn, vd.data_ptr(), 31, 20, 31 * cn - 1,
                               s) == _lib.TBDK_EINVAL
    for ip, gp, qp in ((row - 1, vg.stride(0) * 4, vq.stride(0)), (vs.stride(0), 8 * w - 8, vq.stride(0)),
                       (vs.stride(0), vg.stride(0) * 4, 2 * w - 2)):
        assert lib.tbdk_hog_gradient(gpu.handle, vs.data_ptr(), w, h, ip, cn, C.byref(hg.p), vg.data_ptr(), gp,
                                     vq.data_ptr(), qp, s) == _lib.TBDK_EINVAL
    n = C.c_int(-1)
    xy, sc = np.zeros((64, 2), np.int32), np.zeros(64, np.float64)
    rects = np.zeros((64, 4), np.int32)
    svm = hg.svm
    assert lib.tbdk_hog_detect(gpu.handle, vs.data_ptr(), w, h, row - 1, cn, C.byref(hg.p),
                               svm.ctypes.data_as(C.c_void_p), svm.size, xy.ctypes.data_as(C.c_void_p),
                               sc.ctypes.data_as(C.c_void_p), 64, C.byref(n), s) == _lib.TBDK_EINVAL
    assert lib.tbdk_hog_detect_multiscale(gpu.handle, vs.data_ptr(), w, h, row - 1, cn, C.byref(hg.p),
                                          svm.ctypes.data_as(C.c_void_p), svm.size, rects.ctypes.data_as(C.c_void_p),
                                          sc.ctypes.data_as(C.c_void_p), 64, C.byref(n), s) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(pd, d0) and torch.equal(pg, g0) and torch.equal(pq, q0)
