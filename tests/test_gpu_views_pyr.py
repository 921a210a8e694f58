"""Pyramids, pyrDown, sparse and dense PyrLK on pitched, unaligned views
(tests/_views.py): every frame is an interior window of a larger noise-filled
allocation, in each layout that selects another load path of the kernels
(klt_pyr.hip: the 16-byte path, the dword path, the scalar paths through the
base or the pitch; klt_lk_multi_body.inc: a borrowed level 0 whose pitch is not
its width).  Oracles and criteria are those of the contiguous tests
(test_gpu_klt.py, test_gpu_klt_cn.py, test_gpu_f16.py, test_gpu_f32.py,
test_gpu_dense_lk.py): bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import _oracle as O
import _views as V
from test_gpu_klt import assert_exact

pytestmark = pytest.mark.gpu

LAYOUTS = list(V.LAYOUTS)
# a float2 plane's pitch must be a multiple of 8: the layouts whose pitch is one
FLOW_LAYOUTS = {"a16_pitched": "a16_pitched", "vec4": "vec4", "odd_base": "odd_base", "odd_pitch": "vec4",
                "odd_both": "odd_base"}
PYR_MODES = ((1, 4, 1), (1, 2, 0), (1, 1, 1), (1, 4, 0), (0, 4, 1))  # pyr_fuse, pyr_rows, pyr_xcd


def dwin(arr, layout, seed=0):
    return V.window(arr, layout, seed, device="cuda")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _reset_pyr_options(gpu):
    gpu.set_option("pyr_fuse", 1)
    gpu.set_option("pyr_rows", 1)
    gpu.set_option("pyr_xcd", 1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,maxlev,win", [((61, 93), 4, 7), ((137, 261), 2, 21), ((77, 124), 2, 21)])
def test_pyramid_u8_on_views(gpu, layout, shape, maxlev, win):
    """klt.build_pyramid / Pyramid.build / tbdk_pyr_build and the levels-only
    build, under pyr_fuse 1 (4 / 2 / 1 rows per thread, with and without XCD
    bands) and pyr_fuse 0 (pad_copy_kernel): every padded level equals
    O.Pyramid's, padding included, every derivative plane O.scharr's.  (77, 124):
    w % 4 == 0, where the dword fast path reaches the row ends."""
    from opencv_amd import klt

    img = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    parent, view = dwin(img, layout, seed=win)
    before = V.snapshot(parent)
    assert view.data_ptr() % 16 == V.LAYOUTS[layout].base and view.stride(0) % 16 == V.LAYOUTS[layout].pitch
    R = None
    try:
        for mode, rows, xcd in PYR_MODES:
            gpu.set_option("pyr_fuse", mode)
            gpu.set_option("pyr_rows", rows)
            gpu.set_option("pyr_xcd", xcd)
            for derivs in (False, True):
                P = klt.build_pyramid(view, (win, win), maxlev, ctx=gpu, derivs=derivs)
                torch.cuda.synchronize()
                if R is None:
                    R = O.Pyramid(img, (win, win), maxlev, pad=P.pyr.lv[0].pad)
                tag = f"fuse {mode} rows {rows} xcd {xcd} derivs {derivs}"
                assert P.nlevels == R.nlevels
                for lvl in range(P.nlevels):
                    assert np.array_equal(P.level(lvl, True), R.level(lvl, True)), f"{tag} level {lvl}"
                    if derivs:
                        assert np.array_equal(P.deriv(lvl), O.scharr(R.level(lvl))), f"{tag} deriv {lvl}"
    finally:
        _reset_pyr_options(gpu)
    assert torch.equal(parent, before)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,maxlev,win", [((61, 93), 4, 7), ((137, 261), 2, 21), ((77, 124), 2, 21)])
def test_pyramid_borrowed_level0_on_views(gpu, layout, shape, maxlev, win):
    """Pyramid.build_borrowed on a view: level 0 is the view itself (its pointer,
    its pitch, no padding), levels 1.. equal the oracle's padded levels (the
    two-role launch only: a borrowed build needs pyr_fuse 1)"""
    from opencv_amd import klt

    img = np.random.default_rng(sum(shape) + 1).integers(0, 256, shape, dtype=np.uint8)
    parent, view = dwin(img, layout, seed=win)
    before = V.snapshot(parent)
    P = klt.Pyramid(gpu, shape[1], shape[0], maxlev, (win, win), derivs=False)
    R = None
    try:
        for mode, rows, xcd in PYR_MODES[:4]:
            gpu.set_option("pyr_rows", rows)
            gpu.set_option("pyr_xcd", xcd)
            P.build_borrowed(view)
            torch.cuda.synchronize()
            L0 = P.pyr.lv[0]
            assert L0.data == view.data_ptr() and L0.pitch == view.stride(0) and L0.pad == 0
            assert L0.pitch != shape[1]
            if R is None:
                R = O.Pyramid(img, (win, win), maxlev, pad=P.pyr.lv[1].pad)
            assert P.nlevels == R.nlevels
            assert np.array_equal(P.level(0), img)
            for lvl in range(1, P.nlevels):
                assert np.array_equal(P.level(lvl, True), R.level(lvl, True)), f"fuse {mode}/{rows}/{xcd} level {lvl}"
    finally:
        _reset_pyr_options(gpu)
    assert torch.equal(parent, before)


@pytest.fixture(scope="module")
def lk_frames():
    fr, _ = O.synth(57, 200, 150, 8, 0, 2)
    rng = np.random.default_rng(21)
    pts = np.concatenate([rng.uniform([-12, -12], [212, 162], (1200, 2)),
                          np.array([[0, 0], [199, 149], [0.5, 75], [199.75, 10.25], [100, 0], [100, 149.5],
                                    [-100, -100], [1e4, 5], [-21.0, 50.0], [219.0, 169.0]])]).astype(np.float32)
    return fr[0], fr[1], pts


_lk_oracle_cache = {}


def _lk_oracle(lk_frames, win, maxlev, flags, pad):
    key = (win, maxlev, flags, pad)
    if key not in _lk_oracle_cache:
        a, b, pts = lk_frames
        Ra, Rb = O.Pyramid(a, (win, win), maxlev, pad), O.Pyramid(b, (win, win), maxlev, pad)
        _lk_oracle_cache[key] = O.lk(Ra, Rb, pts, (win, win), maxlev, 30, 0.01, flags, accum=O.ACCUM_EXACT)
    return _lk_oracle_cache[key]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("win,maxlev", [(21, 2), (7, 3), (31, 2)])
def test_lk_borrowed_level0_on_views(gpu, lk_frames, layout, win, maxlev):
    """SparsePyrLKOpticalFlow (the several-points-per-wave kernel) on two
    pyramids that borrow views as their level 0 (ipitch != w: the exact bound
    L.ipitch * hp and the reflection by coordinates), windows over each edge and
    points outside the frame included: equal to the exact-order oracle as in
    test_gpu_klt.assert_exact, and to the padded pyramids' result bit for bit,
    with and without the minimum-eigenvalue error"""
    from opencv_amd import klt

    a, b, pts = lk_frames
    h, w = a.shape
    pa, va = dwin(a, layout, seed=1)
    pb, vb = dwin(b, layout, seed=2)
    dpts = torch.from_numpy(pts).cuda()
    for flags8 in (False, True):
        lk = klt.SparsePyrLKOpticalFlow((win, win), maxlev, 30, getMinEigenVals=flags8, impl=3)
        out = []
        for borrow in (False, True):
            Pa = klt.Pyramid(gpu, w, h, maxlev, (win, win), derivs=False)
            Pb = klt.Pyramid(gpu, w, h, maxlev, (win, win), derivs=False)
            if borrow:
                Pa.build_borrowed(va)
                Pb.build_borrowed(vb)
                assert Pa.pyr.lv[0].pitch == va.stride(0) != w
            else:
                Pa.build(va)
                Pb.build(vb)
            r = lk.calc(Pa, Pb, dpts, want_iters=True)
            torch.cuda.synchronize()
            out.append((r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()))
            pad = Pa.pyr.lv[1].pad
        ex = _lk_oracle(lk_frames, win, maxlev, 8 if flags8 else 0, pad)
        assert_exact(out[0], ex)
        assert_exact(out[1], ex)
        for u, v in zip(*out):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), f"flags8 {flags8}"
        assert out[0][1].mean() > 0.5


@pytest.mark.parametrize("slayout", LAYOUTS)
@pytest.mark.parametrize("dlayout", ["odd_both", "vec4", "a16_pitched"])
@pytest.mark.parametrize("shape", [(61, 93), (2, 3)])
def test_pyr_down_on_views(gpu, slayout, dlayout, shape):
    """tbdk_pyr_down_u8 with source and destination both windows: the
    destination equals O.pyr_down and its guards stay"""
    h, w = shape
    img = np.random.default_rng(3).integers(0, 256, shape, dtype=np.uint8)
    ps, vs = dwin(img, slayout, seed=1)
    dh, dw = (h + 1) // 2, (w + 1) // 2
    pd, vd = dwin(np.full((dh, dw), 0xA5, np.uint8), dlayout, seed=2)
    s0, d0 = V.snapshot(ps), V.snapshot(pd)
    st = gpu.lib.tbdk_pyr_down_u8(gpu.handle, vs.data_ptr(), w, h, vs.stride(0), vd.data_ptr(), vd.stride(0), _stream())
    torch.cuda.synchronize()
    assert st == 0
    assert np.array_equal(vd.cpu().numpy(), O.pyr_down(img))
    assert V.guards_intact(pd, d0, vd) and torch.equal(ps, s0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cn", [3, 4])
def test_pyramid_and_lk_cn_on_views(gpu, layout, cn):
    """tbdk_pyr_create_cn pyramids of u8 BGR / BGRA views and sparse PyrLK on
    them, against the oracle of test_gpu_klt_cn.py"""
    from opencv_amd import klt
    from test_gpu_klt_cn import _frames

    A, B = _frames(cn, 93, 61)
    win, maxlev = (15, 9), 2
    pa, va = dwin(A, layout, seed=cn)
    pb, vb = dwin(B, layout, seed=cn + 1)
    b0 = V.snapshot(pa)
    Pa = klt.build_pyramid(va, win, maxlev, ctx=gpu)
    Pb = klt.build_pyramid(vb, win, maxlev, ctx=gpu)
    torch.cuda.synchronize()
    pad = Pa.pyr.lv[0].pad
    Ra, Rb = O.Pyramid(A, win, maxlev, pad), O.Pyramid(B, win, maxlev, pad)
    assert Pa.nlevels == Ra.nlevels and Pa.channels == cn
    for lvl in range(Pa.nlevels):
        assert np.array_equal(Pa.level(lvl, True), Ra.level(lvl, True)), lvl
        assert np.array_equal(Pa.deriv(lvl), O.scharr(Ra.level(lvl))), lvl
    ys, xs = np.mgrid[0:61:4, 0:93:4]
    pts = np.concatenate([np.stack([xs.ravel(), ys.ravel()], 1) + [0.37, 0.61],
                          [[-5, 10], [96, 20], [0.5, 0.5], [92.5, 60.5]]]).astype(np.float32)
    lk = klt.SparsePyrLKOpticalFlow(win, maxlev, 30)
    r = lk.calc(Pa, Pb, torch.from_numpy(pts).cuda(), want_iters=True)
    torch.cuda.synchronize()
    g = (r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy())
    assert_exact(g, O.lk(Ra, Rb, pts, win, maxlev, 30, 0.01, 0, accum=O.ACCUM_EXACT))
    assert torch.equal(pa, b0)


def _fp_check(P, R, bits):
    assert P.nlevels == R.nlevels
    for i in range(P.nlevels):
        ref = R.levels[i]
        hh, ww = ref.shape[:2]
        pad = P.pyr.lv[i].pad
        ry = [O.load().orc_reflect101(y - pad, hh) for y in range(hh + 2 * pad)]
        rx = [O.load().orc_reflect101(x - pad, ww) for x in range(ww + 2 * pad)]
        assert np.array_equal(P.level(i, True).view(bits), ref[np.ix_(ry, rx)].view(bits)), f"level {i}"
        assert np.array_equal(P.deriv(i).view(bits), R.derivs[i].view(bits)), f"deriv {i}"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pyramid_f16_from_f16_on_views(gpu, layout):
    """an f16 frame (a view, whole-element offset and pitch) into an f16 pyramid,
    against O.Pyramid16 as test_gpu_f16.py"""
    from opencv_amd import klt

    rng = np.random.default_rng(3)
    img = (rng.uniform(0, 255, (61, 93)) + rng.uniform(0, 1, (61, 93))).astype(np.float16)
    img[:2, :3] = np.float16(1e-6)  # fp16 subnormals
    parent, view = dwin(img, layout, seed=5)
    before = V.snapshot(parent)
    R = O.Pyramid16(img, (15, 15), 3)
    try:
        for mode in (1, 0):
            gpu.set_option("pyr_fuse", mode)
            P = klt.Pyramid(gpu, 93, 61, 3, (15, 15), torch.float16).build(view)
            torch.cuda.synchronize()
            _fp_check(P, R, np.uint16)
    finally:
        _reset_pyr_options(gpu)
    assert torch.equal(parent, before)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_pyramid_f32_cn3_on_views(gpu, layout, kind):
    """the cn = 3 fp32 pyramid (tbdk_pyr_create_f32_cn) from u16 and from f32
    views, against O.Pyramid16(f32=True) as test_gpu_f32.py"""
    from opencv_amd import klt
    from test_gpu_f32 import _cn_frames

    a, _, _ = _cn_frames(kind, 3, 93, 61)
    parent, view = dwin(a, layout, seed=7)
    before = V.snapshot(parent)
    R = O.Pyramid16(a, (21, 21), 3, f32=True)
    P = klt.Pyramid(gpu, 93, 61, 3, (21, 21), torch.float32, channels=3).build(view)
    torch.cuda.synchronize()
    assert P.channels == 3
    _fp_check(P, R, np.uint32)
    assert torch.equal(parent, before)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_dense_lk_on_views(gpu, layout):
    """tbdk_lk_dense at (96, 72), win 13, maxLevel 2: frames, flow and status
    all windows (the flow's pitch a multiple of 8); status exact, flow exact where status is 1
    (test_dense_matches_oracle_at_every_pixel's criterion), guards intact"""
    from opencv_amd import klt

    w, h, win, maxlev = 72, 96, 13, 2
    fr, _ = O.synth(31 + w, w, h, 4, 0, 2)
    pa, va = dwin(fr[0], layout, seed=1)
    pb, vb = dwin(fr[1], layout, seed=2)
    pf, vf = dwin(np.full((h, w, 2), -7.25, np.float32), FLOW_LAYOUTS[layout], seed=3)
    ps, vs = dwin(np.full((h, w), 0xA5, np.uint8), layout, seed=4)
    f0, s0 = V.snapshot(pf), V.snapshot(ps)
    lk = klt.DensePyrLKOpticalFlow.create((win, win), maxlev, 30)
    Pa = klt.build_pyramid(va, (win, win), maxlev, ctx=gpu)
    Pb = klt.build_pyramid(vb, (win, win), maxlev, ctx=gpu)
    prm = lk.params()
    st = gpu.lib.tbdk_lk_dense(gpu.handle, C.byref(Pa.pyr), C.byref(Pb.pyr), vf.data_ptr(), vf.stride(0) * 4,
                               vs.data_ptr(), vs.stride(0), C.byref(prm), _stream())
    torch.cuda.synchronize()
    assert st == 0
    ys, xs = np.mgrid[0:h, 0:w]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    nx, ost, _, _ = O.lk(O.Pyramid(fr[0], (win, win), maxlev), O.Pyramid(fr[1], (win, win), maxlev), pts,
                         win=(win, win), max_level=maxlev, accum=O.ACCUM_EXACT, want_err=False)
    assert np.array_equal(vs.cpu().numpy().ravel(), ost)
    ok = ost == 1
    assert np.array_equal(vf.cpu().numpy().reshape(-1, 2)[ok], (nx - pts).astype(np.float32)[ok])
    assert V.guards_intact(pf, f0, vf) and V.guards_intact(ps, s0, vs)


def test_pitch_below_the_row_is_refused(gpu):
    """pitch < row (and dst_pitch < row): TBDK_EINVAL, and nothing is enqueued
    (the destination keeps every byte)"""
    from opencv_amd import _lib, klt

    img = np.random.default_rng(1).integers(0, 256, (61, 93), dtype=np.uint8)
    parent, view = dwin(img, "odd_both")
    lib, s = gpu.lib, _stream()
    P = klt.build_pyramid(view, (21, 21), 2, ctx=gpu, derivs=False)
    torch.cuda.synchronize()
    lv0 = P.level(0, True)
    other, oview = dwin(255 - img, "odd_both", seed=1)
    for fn in (lib.tbdk_pyr_build, lib.tbdk_pyr_build_borrowed):
        assert fn(gpu.handle, oview.data_ptr(), 92, C.byref(P.pyr), s) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(P.level(0, True), lv0) and P.pyr.lv[0].pad > 0
    pd, vd = dwin(np.full((31, 47), 0xA5, np.uint8), "odd_both", seed=2)
    d0 = V.snapshot(pd)
    assert lib.tbdk_pyr_down_u8(gpu.handle, view.data_ptr(), 93, 61, 92, vd.data_ptr(), vd.stride(0), s) == \
        _lib.TBDK_EINVAL
    assert lib.tbdk_pyr_down_u8(gpu.handle, view.data_ptr(), 93, 61, view.stride(0), vd.data_ptr(), 46, s) == \
        _lib.TBDK_EINVAL
    # dense LK: flow_pitch < 8 * w, status_pitch < w
    Pa = klt.build_pyramid(view, (13, 13), 2, ctx=gpu)
    prm = klt.DensePyrLKOpticalFlow.create((13, 13), 2, 30).params()
    pf, vf = dwin(np.zeros((61, 93, 2), np.float32), "vec4", seed=3)
    ps, vs = dwin(np.zeros((61, 93), np.uint8), "odd_both", seed=4)
    f0, s0 = V.snapshot(pf), V.snapshot(ps)
    assert (vf.stride(0) * 4) % 8 == 0
    assert lib.tbdk_lk_dense(gpu.handle, C.byref(Pa.pyr), C.byref(Pa.pyr), vf.data_ptr(), 8 * 93 - 8, vs.data_ptr(),
                             vs.stride(0), C.byref(prm), s) == _lib.TBDK_EINVAL
    assert lib.tbdk_lk_dense(gpu.handle, C.byref(Pa.pyr), C.byref(Pa.pyr), vf.data_ptr(), vf.stride(0) * 4,
                             vs.data_ptr(), 92, C.byref(prm), s) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(pd, d0) and torch.equal(pf, f0) and torch.equal(ps, s0)
    # the other pyramid kinds: a row is width * cn elements
    h, w = 61, 93
    _, v3 = dwin(np.zeros((h, w, 3), np.uint8), "odd_both", seed=5)
    _, vh = dwin(np.ones((h, w), np.float16), "odd_both", seed=6)
    _, vu = dwin(np.zeros((h, w, 3), np.uint16), "odd_both", seed=7)
    _, vf3 = dwin(np.ones((h, w, 3), np.float32), "odd_both", seed=8)
    P3 = klt.Pyramid(gpu, w, h, 2, (15, 15), channels=3).build(v3)
    Ph = klt.Pyramid(gpu, w, h, 2, (15, 15), torch.float16).build(vh)
    Pf = klt.Pyramid(gpu, w, h, 2, (15, 15), torch.float32, channels=3).build(vf3)
    torch.cuda.synchronize()
    kept = [P3.level(0, True), Ph.level(0, True), Pf.level(0, True)]
    assert lib.tbdk_pyr_build(gpu.handle, v3.data_ptr(), 3 * w - 1, C.byref(P3.pyr), s) == _lib.TBDK_EINVAL
    assert lib.tbdk_pyr_build_f16(gpu.handle, vh.data_ptr(), 2 * w - 2, C.byref(Ph.pyr), s) == _lib.TBDK_EINVAL
    assert lib.tbdk_pyr_build_u16(gpu.handle, vu.data_ptr(), 6 * w - 2, C.byref(Pf.pyr), s) == _lib.TBDK_EINVAL
    assert lib.tbdk_pyr_build_f32(gpu.handle, vf3.data_ptr(), 12 * w - 4, C.byref(Pf.pyr), s) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    for P, k in zip((P3, Ph, Pf), kept):
        assert np.array_equal(P.level(0, True).view(np.uint8), k.view(np.uint8))
