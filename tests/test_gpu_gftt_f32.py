"""GPU GFTT and corner response maps on 32F and 16U images (tbdk_gftt_rois_px,
tbdk_corner_response_px) against the numpy restatement of the reference's CV_32F
path (tests/_gftt_f32_oracle.py) and the real reference's recordings
(tests/golden/reference_gftt_f32.npz).  Every comparison is exact: the maps word
for word, the corner lists per ROI in order and count."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gftt_f32_cases as FC
import _gftt_f32_oracle as O32
import _gftt_mask_cases as MC
import _reference_cases as RC

pytestmark = pytest.mark.gpu

# the ROI list of tests/test_gpu_gftt_mask.py (widths 56/57/58/112/113 straddle the 56-column
# strip; 3x3, 2x50 and 1x1 are the degenerate shapes), and a ROI of 4 * 8 + 7 rows at an odd x:
# segments of 10 rows, so the dense kernel's eight-rows-in-flight loop runs exactly once in the two
# middle segments and not at all in the outer two (7 steady rows), the compact kernel's (four rows) in all
ROIS = [(0, 0, 160, 120), (300, 200, 77, 33), (250, 200, 64, 48), (401, 203, 57, 40), (20, 30, 56, 20),
        (21, 31, 112, 9), (10, 400, 113, 80), (33, 77, 58, 5), (600, 440, 3, 3), (5, 5, 2, 50), (100, 100, 1, 1),
        (77, 231, 90, 39)]
# a non-overlapping subset for the masks built per ROI
PASTE_ROIS = [(0, 0, 160, 120), (300, 200, 77, 33), (401, 203, 57, 40), (10, 400, 113, 80), (600, 440, 3, 3),
              (200, 5, 2, 50)]
# (maxCorners, quality, minDistance); quality 1.5 > 1 takes the dense eigenvalue plane whatever gftt_compact says
PARAMS = [(256, .01, 3.0), (1000, .01, 0.0), (64, .05, 8.0), (40, 1.0, 1.0), (256, 1.5, 3.0)]
DEFAULTS = {"gftt_compact": 1, "gftt_eig_redo": 0}

_cache = {}


def cached(key, make):
    """a reference computed once and shared (read only)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read only)


def frame_dev(kind):
    return cached(("dev", kind), lambda: dev(FC.frame(kind)))


def ref_lists(kind, rois, maxc, q, md, mask=None, mask_key=None, block=3, harris=False):
    return cached(("ref", kind, tuple(rois), maxc, q, md, mask_key, block, harris),
                  lambda: O32.gftt_rois(FC.frame(kind), mask, rois, maxc, q, md, block, harris, FC.HARRIS_K))


def detect(img, mask, rois, maxc, q, md, block=3, harris=False, k=FC.HARRIS_K):
    from opencv_amd import klt

    det = klt.GoodFeaturesToTrackDetector(maxc, q, md, block, harris, k)
    if isinstance(mask, np.ndarray):
        mask = dev(mask)
    c, n = det.detect_rois(img, rois, mask=mask)
    torch.cuda.synchronize()
    return c.cpu().numpy(), n.cpu().numpy()


def check(ref, c, n, what=""):
    assert len(ref) == len(n)
    for i, r in enumerate(ref):
        assert n[i] == len(r), f"{what} roi {i}: count {n[i]} vs {len(r)}"
        assert np.array_equal(c[i, :n[i]], r), f"{what} roi {i}: corners differ"


class options:
    def __init__(self, gpu, **kw):
        self.gpu, self.kw = gpu, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.gpu.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.gpu.set_option(k, DEFAULTS[k])


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- response maps --------------------------------------------------------------------

def map_tensor(h, w, kind):
    """the case's image on the device; the 113 x 40 one as a slice of a wider
    tensor from an odd column, so its pitch is not w pixels"""
    img = FC.map_image(h, w, kind)
    if (h, w) != (113, 40):
        return dev(img)
    big = np.zeros((h + 2, w + 13), img.dtype)
    big[1:1 + h, 5:5 + w] = img
    view = dev(big)[1:1 + h, 5:5 + w]
    assert view.stride(0) == w + 13 and view.stride(1) == 1
    return view


@pytest.mark.parametrize("kind", FC.KINDS)
def test_maps_match_restatement_and_recordings(gpu, kind):
    from opencv_amd import klt

    fx = FC.fixture()
    cases = FC.map_cases()
    for h, w in FC.MAP_SHAPES:
        t = map_tensor(h, w, kind)
        img = FC.map_image(h, w, kind)
        for block, harris in FC.MAP_MODES:
            got = klt.corner_response(t, block, bool(harris), FC.HARRIS_K, ctx=gpu).cpu().numpy()
            with np.errstate(over="ignore", invalid="ignore"):
                ref = O32.response(img, block, bool(harris), FC.HARRIS_K)
            what = f"{kind} {h}x{w} block {block} harris {harris}"
            assert got.shape == (h, w) and np.array_equal(words(got), words(ref)), what
            RC.assert_pinned(got, fx[f"{cases.index((h, w, kind, block, harris))}_e"], what)
            if block == 3 and not harris:
                with options(gpu, gftt_eig_redo=1):
                    again = klt.corner_min_eigen_val(t, ctx=gpu).cpu().numpy()
                assert np.array_equal(words(again), words(got)), what + " (segments walked in sequence)"


def test_small_images_take_no_second_walk_and_match(gpu):
    """`small` images: no fresh start differs (tests/test_gftt_f32_oracle.py), so
    the first concurrent walk stands; forcing the sequential one gives the same map"""
    from opencv_amd import klt

    for h, w in FC.MAP_SHAPES:
        img = FC.map_image(h, w, "small")
        ref = O32.response(img)
        got = klt.corner_min_eigen_val(dev(img), ctx=gpu).cpu().numpy()
        assert np.array_equal(words(got), words(ref)), (h, w)
        with options(gpu, gftt_eig_redo=1):
            got = klt.corner_min_eigen_val(dev(img), ctx=gpu).cpu().numpy()
        assert np.array_equal(words(got), words(ref)), (h, w)
    f = FC.image("small", 640, 480, FC.FRAME_SEED)
    ref = O32.gftt_rois(f, None, ROIS, 256, .01, 3.0)
    c, n = detect(dev(f), None, ROIS, 256, .01, 3.0)
    check(ref, c, n, "small")
    assert n.sum() > 0


# ---- ROI lists ------------------------------------------------------------------------

@pytest.mark.parametrize("compact,redo", [(1, 0), (1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize("kind", FC.KINDS)
def test_roi_lists_match_restatement(gpu, kind, compact, redo):
    img = frame_dev(kind)
    total = 0
    for maxc, q, md in PARAMS:
        with options(gpu, gftt_compact=compact, gftt_eig_redo=redo):
            c, n = detect(img, None, ROIS, maxc, q, md)
        check(ref_lists(kind, ROIS, maxc, q, md), c, n, f"{kind} ({maxc}, {q}, {md}) compact {compact} redo {redo}")
        if q > 1:
            assert (n == 0).all()  # the threshold lies above the maximum
        total += int(n.sum())
    assert total > 1000


@pytest.mark.parametrize("compact", [0, 1])
def test_hdr_natural_and_forced_second_walks_agree(gpu, compact):
    """on `hdr` every fresh start differs from the running sum, so the default
    call already walks segments again; forcing every boundary must change nothing"""
    img = frame_dev("hdr")
    for maxc, q, md in PARAMS[:3]:
        with options(gpu, gftt_compact=compact, gftt_eig_redo=0):
            c0, n0 = detect(img, None, ROIS, maxc, q, md)
        with options(gpu, gftt_compact=compact, gftt_eig_redo=1):
            c1, n1 = detect(img, None, ROIS, maxc, q, md)
        assert np.array_equal(n0, n1) and np.array_equal(c0, c1)
        assert n0.sum() > 0


@pytest.mark.parametrize("block,harris", [(5, False), (2, False), (3, True)])
@pytest.mark.parametrize("kind", FC.KINDS)
def test_block_and_harris_modes(gpu, kind, block, harris):
    for maxc, q, md in ((256, .01, 3.0), (1000, .001, 0.0)):
        c, n = detect(frame_dev(kind), None, ROIS, maxc, q, md, block, harris)
        check(ref_lists(kind, ROIS, maxc, q, md, block=block, harris=harris), c, n, f"{kind} block {block} harris {harris}")
        assert n.sum() > 0


# ---- masked ---------------------------------------------------------------------------

def hole(img, radius=6):
    """255 except a disc around the image's strongest unmasked corner"""
    h, w = img.shape
    m = MC.ones(w, h)
    c = O32.gftt(img, None, 1, 0.01, 0.0)
    if len(c):
        yy, xx = np.mgrid[0:h, 0:w]
        m[(xx - int(c[0, 0])) ** 2 + (yy - int(c[0, 1])) ** 2 <= radius * radius] = 0
    return m


def frame_mask(kind, mask_kind):
    if mask_kind == "hole":  # built per ROI as an isolated image, pasted into a zero plane
        def make():
            m = np.zeros((480, 640), np.uint8)
            for x, y, w, h in PASTE_ROIS:
                m[y:y + h, x:x + w] = hole(np.ascontiguousarray(FC.frame(kind)[y:y + h, x:x + w]))
            return m
        return cached(("hole", kind), make), PASTE_ROIS
    return {"rect1": MC.rect1, "checker": MC.checker, "zero": MC.zero}[mask_kind](640, 480), ROIS


@pytest.mark.parametrize("mask_kind", ["rect1", "checker", "zero", "hole"])
@pytest.mark.parametrize("kind", ["unit", "hdr"])
def test_masked_rois_match_restatement(gpu, kind, mask_kind):
    m, rois = frame_mask(kind, mask_kind)
    md = dev(m)
    total = 0
    for (maxc, q, dist), compact in zip(PARAMS[:4], (1, 0, 1, 0)):
        with options(gpu, gftt_compact=compact):
            c, n = detect(frame_dev(kind), md, rois, maxc, q, dist)
        check(ref_lists(kind, rois, maxc, q, dist, m, mask_kind), c, n, f"{kind} {mask_kind} ({maxc}, {q}, {dist})")
        total += int(n.sum())
    if mask_kind == "zero":
        assert total == 0
    else:
        assert total > 0
    if mask_kind == "hole":  # the strongest corner is masked out: another list than the unmasked one
        c, n = detect(frame_dev(kind), md, rois, 256, .01, 3.0)
        c0, n0 = detect(frame_dev(kind), None, rois, 256, .01, 3.0)
        assert not (np.array_equal(n, n0) and np.array_equal(c, c0))
    # the generic response under a mask
    c, n = detect(frame_dev(kind), md, rois, 64, .05, 8.0, 5, True)
    check(ref_lists(kind, rois, 64, .05, 8.0, m, mask_kind, 5, True), c, n, f"{kind} {mask_kind} harris")


# ---- 16U is 32F on the converted image -----------------------------------------------------

def test_u16_equals_f32_on_the_converted_tensor(gpu):
    from opencv_amd import klt

    f16 = FC.frame("u16")
    a, b = dev(f16), dev(f16.astype(np.float32))
    assert a.dtype == torch.uint16 and b.dtype == torch.float32
    m = dev(MC.checker(640, 480))
    for maxc, q, md in PARAMS[:3]:
        for mask in (None, m):
            for block, harris in ((3, False), (5, True)):
                det = klt.GoodFeaturesToTrackDetector(maxc, q, md, block, harris)
                ca, na = det.detect_rois(a, ROIS, mask=mask)
                cb, nb = det.detect_rois(b, ROIS, mask=mask)
                assert torch.equal(na, nb) and torch.equal(ca.view(torch.int32), cb.view(torch.int32))
                assert int(na.sum()) > 0
    for block, harris in FC.MAP_MODES:
        ea, eb = klt.corner_response(a, block, bool(harris)), klt.corner_response(b, block, bool(harris))
        assert torch.equal(ea.view(torch.int32), eb.view(torch.int32))
    assert torch.equal(klt.corner_min_eigen_val(a).view(torch.int32), klt.corner_min_eigen_val(b).view(torch.int32))
    # the whole-image form
    det = klt.GoodFeaturesToTrackDetector(64, .05, 8.0)
    crop = f16[:120, :160]
    got = det.detect(dev(crop)).cpu().numpy()
    assert np.array_equal(got, O32.gftt(crop, None, 64, .05, 8.0)) and len(got) > 0
    assert torch.equal(det.detect(dev(crop)), det.detect(dev(crop.astype(np.float32))))


# ---- pix = TBDK_PIX_U8 forwards to the 8-bit entries ------------------------------------------

def test_pix_u8_is_the_8bit_entries(gpu):
    from opencv_amd import _lib, klt

    bb = np.ascontiguousarray(RC.basketball()[0])
    H, W = bb.shape
    img, m = dev(bb), dev(MC.checker(W, H))
    arr = (_lib.Roi * len(ROIS))(*[_lib.Roi(*r) for r in ROIS])
    for maxc, q, md, block, harris in ((256, .01, 3.0, 3, 0), (64, .05, 8.0, 5, 1)):
        det = klt.GoodFeaturesToTrackDetector(maxc, q, md, block, bool(harris))
        for mask in (None, m):
            c0, n0 = det.detect_rois(img, ROIS, mask=mask)
            c1 = torch.zeros_like(c0)
            n1 = torch.zeros_like(n0)
            rc = gpu.lib.tbdk_gftt_rois_px(gpu.handle, C.c_void_p(img.data_ptr()), _lib.TBDK_PIX_U8, W, H, W,
                                           C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                           W if mask is not None else 0, arr, len(ROIS), C.byref(det.prm),
                                           C.c_void_p(c1.data_ptr()), C.c_void_p(n1.data_ptr()), None)
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(n0, n1) and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
            assert int(n0.sum()) > 0
    for block, harris in FC.MAP_MODES:
        e0 = klt.corner_response(img, block, bool(harris))
        e1 = torch.empty_like(e0)
        rc = gpu.lib.tbdk_corner_response_px(gpu.handle, C.c_void_p(img.data_ptr()), _lib.TBDK_PIX_U8, W, H, W,
                                             C.c_void_p(e1.data_ptr()), W * 4, block, harris, 0.04, None)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(e0.view(torch.int32), e1.view(torch.int32))


# ---- arguments ----------------------------------------------------------------------------

def test_bad_images_rejected(gpu):
    from opencv_amd import _lib, klt

    det = klt.GoodFeaturesToTrackDetector(10, .01, 0.0)
    W, H = 64, 48
    f32 = torch.zeros((H + 1, W + 2), dtype=torch.float32, device="cuda")
    u16 = torch.zeros((H + 1, W + 2), dtype=torch.uint16, device="cuda")
    roi = (_lib.Roi * 1)(_lib.Roi(0, 0, 20, 20))
    corners = torch.zeros((1, 10, 2), dtype=torch.float32, device="cuda")
    counts = torch.zeros((1,), dtype=torch.int32, device="cuda")
    dst = torch.zeros((H, W), dtype=torch.float32, device="cuda")

    def gftt(ptr, pix, pitch):
        return gpu.lib.tbdk_gftt_rois_px(gpu.handle, C.c_void_p(ptr), pix, W, H, pitch, None, 0, roi, 1,
                                         C.byref(det.prm), C.c_void_p(corners.data_ptr()),
                                         C.c_void_p(counts.data_ptr()), None)

    def cmap(ptr, pix, pitch, block=3):
        return gpu.lib.tbdk_corner_response_px(gpu.handle, C.c_void_p(ptr), pix, W, H, pitch,
                                               C.c_void_p(dst.data_ptr()), W * 4, block, 0, 0.04, None)

    p32, p16 = f32.data_ptr(), u16.data_ptr()
    pitch32, pitch16 = (W + 2) * 4, (W + 2) * 2
    F, U = _lib.TBDK_PIX_F32, _lib.TBDK_PIX_U16
    bad = [(p32 + 2, F, pitch32),   # a float image viewed 2 bytes off
           (p32 + 1, F, pitch32), (p32, F, pitch32 + 2), (p32, F, pitch32 + 1), (p32, F, W * 4 - 4),
           (p16 + 1, U, pitch16),   # a 16-bit image from an odd address
           (p16, U, pitch16 + 1),   # an odd byte pitch
           (p16, U, W * 2 - 2),
           (p32, 3, pitch32), (p32, -1, pitch32)]  # an unknown pix
    for ptr, pix, pitch in bad:
        for call in (gftt, cmap, lambda *a: cmap(*a, block=5)):
            rc = call(ptr, pix, pitch)
            assert rc == _lib.TBDK_EINVAL, (ptr - p32, pix, pitch)
            with pytest.raises(_lib.TbdkError):
                _lib.check(rc, "tbdk_*_px")
    # the same calls, well formed (a 16-bit image 2 bytes off is fine)
    for ptr, pix, pitch in ((p32 + 4, F, pitch32), (p16 + 2, U, pitch16)):
        assert gftt(ptr, pix, pitch) == 0 and cmap(ptr, pix, pitch) == 0 and cmap(ptr, pix, pitch, 5) == 0
    torch.cuda.synchronize()
    # the Python layer: dtype, rank, device, layout
    good = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    for img in (good.to(torch.int32), good.to(torch.float16), good.to(torch.float64), good[None], good.cpu(),
                torch.zeros((H, 2 * W), dtype=torch.float32, device="cuda")[:, ::2], good.cpu().numpy()):
        with pytest.raises(_lib.TbdkError):
            det.detect_rois(img, [(0, 0, 20, 20)])
        with pytest.raises(_lib.TbdkError):
            klt.corner_response(img, 5)
        with pytest.raises(_lib.TbdkError):
            klt.corner_min_eigen_val(img)
    with pytest.raises(_lib.TbdkError):  # whatever the 8-bit entries reject: a ROI outside the image
        det.detect_rois(good, [(60, 0, 20, 20)])


# ---- the recorded corner lists -----------------------------------------------------------------

@pytest.mark.parametrize("kind", FC.KINDS)
def test_reference_recordings_reproduced(gpu, kind):
    """every list case of reference_gftt_f32.npz: what the real reference returned
    (the maps are pinned in test_maps_match_restatement_and_recordings)"""
    fx = FC.fixture()
    nm = len(FC.map_cases())
    imgs = [dev(FC.list_image(kind, r)) for r in range(len(FC.LIST_ROIS))]
    seen = 0
    for j, (k, r, mk, maxc, q, md, block, harris) in enumerate(FC.list_cases()):
        if k != kind:
            continue
        _, _, w, h = FC.LIST_ROIS[r]
        c, n = detect(imgs[r], FC.list_mask(mk, w, h), [(0, 0, w, h)], maxc, q, md, block, bool(harris))
        got = c[0, :n[0]]
        assert n[0] >= 0 and np.array_equal(got, got.astype(np.uint16))
        RC.assert_pinned(got.astype(np.uint16), fx[f"{nm + j}_c"], f"case {nm + j}: {FC.list_cases()[j]}")
        seen += 1
    assert seen == len(FC.list_cases()) // len(FC.KINDS)
