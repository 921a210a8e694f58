"""GPU GFTT under an arbitrary 8-bit mask (tbdk_gftt_rois_masked) against the
numpy restatement of goodFeaturesToTrack's mask semantics
(tests/_gftt_mask_oracle.py) and the real reference's recordings
(tests/golden/reference_gftt_mask.npz): identical corner lists per ROI, same
order, same count."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gftt_mask_cases as MC
import _gftt_mask_oracle as MO
import _oracle as O
import _reference_cases as RC

pytestmark = pytest.mark.gpu

# widths 56/57/58/112/113 straddle the 56-column strip; the last four are the degenerate shapes
ROIS = [(0, 0, 160, 120), (300, 200, 77, 33), (250, 200, 64, 48), (401, 203, 57, 40), (20, 30, 56, 20),
        (21, 31, 112, 9), (10, 400, 113, 80), (33, 77, 58, 5), (600, 440, 3, 3), (5, 5, 2, 50), (100, 100, 1, 1)]
# a non-overlapping subset for the masks pasted per ROI
PASTE_ROIS = [(0, 0, 160, 120), (300, 200, 77, 33), (401, 203, 57, 40), (10, 400, 113, 80), (600, 440, 3, 3),
              (200, 5, 2, 50)]
PARAMS = [(256, .01, 3.0), (1000, .01, 0.0), (64, .05, 8.0), (40, 1.0, 1.0)]


@pytest.fixture(scope="module")
def bb():
    return np.ascontiguousarray(RC.basketball()[0])


@pytest.fixture(scope="module")
def synth():
    fr, gt = O.synth(20261015, 640, 480, 32, 0, 1)
    return np.ascontiguousarray(fr[0]), [tuple(int(v) for v in g[1:]) for g in gt[0] if g[0]]


def detect(frame, mask, rois, maxc, q, md, block=3, harris=False, k=0.04):
    from opencv_amd import klt

    det = klt.GoodFeaturesToTrackDetector(maxc, q, md, block, harris, k)
    img = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(frame).cuda()
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    c, n = det.detect_rois(img, rois, mask=mask)
    torch.cuda.synchronize()
    return c.cpu().numpy(), n.cpu().numpy()


def check(ref, c, n, what=""):
    assert len(ref) == len(n)
    for i, r in enumerate(ref):
        assert n[i] == len(r), f"{what} roi {i}: count {n[i]} vs {len(r)}"
        assert np.array_equal(c[i, :n[i]], r), f"{what} roi {i}: corners differ"


def frame_mask(kind, shape, sq=8):
    h, w = shape
    return {"ones": MC.ones, "zero": MC.zero, "rect1": MC.rect1, "sparse": MC.sparse}[kind](w, h) \
        if kind != "checker" else MC.checker(w, h, sq)


def pasted_mask(kind, frame, rois, block=3, harris=False, k=0.04):
    """`kind` built for each ROI as an isolated image, pasted into a zero plane"""
    m = np.zeros(frame.shape, np.uint8)
    for x, y, w, h in rois:
        m[y:y + h, x:x + w] = MC.make(kind, np.ascontiguousarray(frame[y:y + h, x:x + w]), block, harris, k)
    return m


@pytest.mark.parametrize("maxc,q,md", PARAMS)
def test_masked_rois_match_restatement(gpu, bb, maxc, q, md):
    img = torch.from_numpy(bb).cuda()
    total = 0
    for kind in ("rect1", "checker", "sparse", "zero", "ones"):
        m = frame_mask(kind, bb.shape)
        ref = MO.gftt_rois_masked(bb, m, ROIS, maxc, q, md)
        c, n = detect(img, m, ROIS, maxc, q, md)
        check(ref, c, n, kind)
        if kind == "zero":
            assert (n == 0).all()
        total += int(n.sum())
    for kind in ("hole", "ring"):
        m = pasted_mask(kind, bb, PASTE_ROIS)
        ref = MO.gftt_rois_masked(bb, m, PASTE_ROIS, maxc, q, md)
        c, n = detect(img, m, PASTE_ROIS, maxc, q, md)
        check(ref, c, n, kind)
        total += int(n.sum())
    assert total > 0 or q >= 1  # (at quality 1 the threshold is the maximum itself: no corner anywhere)


@pytest.mark.parametrize("block,harris", [(5, False), (2, False), (1, False), (3, True), (6, True)])
def test_masked_block_and_harris_modes(gpu, synth, block, harris):
    frame, boxes = synth
    rois = boxes + [(0, 0, 3, 3), (5, 5, 2, 50)]
    img = torch.from_numpy(frame).cuda()
    # the boxes overlap: the ring is built per box and pasted for a non-overlapping choice of them
    apart = []
    for r in rois:
        if all(r[0] + r[2] <= o[0] or o[0] + o[2] <= r[0] or r[1] + r[3] <= o[1] or o[1] + o[3] <= r[1]
               for o in apart):
            apart.append(r)
    assert len(apart) >= 8
    for maxc, q, md in ((256, .01, 3.0), (1000, .001, 0.0)):
        m = MC.checker(640, 480)
        check(MO.gftt_rois_masked(frame, m, rois, maxc, q, md, block, harris), *detect(img, m, rois, maxc, q, md, block, harris),
              "checker")
        m = pasted_mask("ring", frame, apart, block, harris)
        ref = MO.gftt_rois_masked(frame, m, apart, maxc, q, md, block, harris)
        c, n = detect(img, m, apart, maxc, q, md, block, harris)
        check(ref, c, n, "ring")
        assert n.sum() > 0 or block == 1  # (a single pixel's covariance has rank 1: its min eigenvalue is ~0)


@pytest.mark.parametrize("option,value,nroi", [("gftt_compact", 0, 0), ("gftt_compact", 1, 0), ("gftt_inline", 0, 0),
                                               ("gftt_inline", 1, 200), ("gftt_eig_redo", 1, 0)])
def test_masked_routing_options(gpu, bb, option, value, nroi):
    defaults = {"gftt_compact": 1, "gftt_inline": 1, "gftt_eig_redo": 0}
    rois = list(ROIS)
    if nroi:  # more ROIs than the kernel arguments hold: the table is read from memory
        rois = [(7 * (i % 80), 5 * (i // 4), 20 + i % 50, 12 + i % 31) for i in range(nroi)]
    m = MC.checker(640, 480)
    m[:, 320:] = MC.sparse(320, 480)
    gpu.set_option(option, value)
    try:
        c, n = detect(bb, m, rois, 256, .01, 3.0)
    finally:
        gpu.set_option(option, defaults[option])
    check(MO.gftt_rois_masked(bb, m, rois, 256, .01, 3.0), c, n, f"{option}={value}")
    assert n.sum() > 0


def test_mask_as_a_slice_of_a_larger_tensor(gpu, bb):
    H, W = bb.shape
    m = MC.sparse(W, H)
    m[:240] = MC.checker(W, 240)
    big = torch.zeros((H + 9, W + 12), dtype=torch.uint8, device="cuda")
    big[3:3 + H, 5:5 + W] = torch.from_numpy(m).cuda()
    view = big[3:3 + H, 5:5 + W]
    assert view.stride(0) > W and view.data_ptr() % 2 == 1
    c0, n0 = detect(bb, m, ROIS, 256, .01, 3.0)
    c1, n1 = detect(bb, view, ROIS, 256, .01, 3.0)
    assert np.array_equal(n0, n1) and np.array_equal(c0, c1)
    check(MO.gftt_rois_masked(bb, m, ROIS, 256, .01, 3.0), c1, n1)


def test_null_mask_is_the_unmasked_call(gpu, bb):
    from opencv_amd import klt

    img = torch.from_numpy(bb).cuda()
    for prm in PARAMS:
        det = klt.GoodFeaturesToTrackDetector(*prm)
        c0, n0 = det.detect_rois(img, ROIS)
        c1, n1 = det.detect_rois(img, ROIS, mask=None)
        assert torch.equal(c0, c1) and torch.equal(n0, n1)
    det = klt.GoodFeaturesToTrackDetector(64, .05, 8.0)
    assert torch.equal(det.detect(img[:120, :160].contiguous()), det.detect(img[:120, :160].contiguous(), mask=None))
    hole = MC.hole(bb[:120, :160])
    got = det.detect(img[:120, :160].contiguous(), mask=torch.from_numpy(hole).cuda()).cpu().numpy()
    assert np.array_equal(got, MO.gftt_masked(bb[:120, :160], hole, 64, .05, 8.0))


def test_scratch_reuse_across_masked_and_unmasked_calls(gpu, bb):
    """the context's scratch is reused: masked, unmasked, masked, each its own oracle's"""
    img = torch.from_numpy(bb).cuda()
    hole = pasted_mask("hole", bb, PASTE_ROIS)
    ring = pasted_mask("ring", bb, PASTE_ROIS)
    for block, harris in ((3, False), (5, True)):
        for m in (hole, None, ring, None, MC.zero(640, 480), None, hole):
            ref = MO.gftt_rois_masked(bb, m, PASTE_ROIS, 256, .01, 3.0, block, harris)
            check(ref, *detect(img, m, PASTE_ROIS, 256, .01, 3.0, block, harris), "masked" if m is not None else "plain")


def test_masked_1080p_128_boxes(gpu):
    fr, gt = O.synth(20261015, 1920, 1080, 128, 0, 1)
    frame = np.ascontiguousarray(fr[0])
    rois = [tuple(int(v) for v in g[1:]) for g in gt[0] if g[0]]
    m = MC.checker(1920, 1080, 16)
    c, n = detect(frame, m, rois, 256, .01, 3.0)
    check(MO.gftt_rois_masked(frame, m, rois, 256, .01, 3.0), c, n)
    assert (n > 0).sum() > len(rois) // 2


def test_reference_recordings_reproduced(gpu):
    """every case of reference_gftt_mask.npz: what the real reference returned"""
    fx = MC.fixture()
    cases, entries = MC.cases(), MC.masks()
    imgs = [torch.from_numpy(MC.roi_image(r)).cuda() for r in range(len(MC.ROIS))]
    masks = [torch.from_numpy(MC.fixture_mask(fx, m)).cuda() for m in range(len(entries))]
    for i, (r, m, maxc, q, md, block, harris) in enumerate(cases):
        _, _, _, w, h = MC.ROIS[r]
        c, n = detect(imgs[r], masks[m], [(0, 0, w, h)], maxc, q, md, block, bool(harris), MC.HARRIS_K)
        got = c[0, :n[0]]
        assert n[0] >= 0 and np.array_equal(got, got.astype(np.uint16))
        RC.assert_pinned(got.astype(np.uint16), fx[f"{i}_c"], f"case {i}: {cases[i]} {entries[m]}")


def test_bad_masks_rejected(gpu, bb):
    from opencv_amd import _lib, klt

    img = torch.from_numpy(bb).cuda()
    H, W = bb.shape
    det = klt.GoodFeaturesToTrackDetector(10, .01, 0.0)
    good = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
    for bad in (good.to(torch.int32), good[:, :W - 1], good[:H - 1], good.cpu(), good[None],
                torch.full((H, 2 * W), 255, dtype=torch.uint8, device="cuda")[:, ::2], bb):
        with pytest.raises(_lib.TbdkError):
            det.detect_rois(img, [(0, 0, 20, 20)], mask=bad)
    # the C ABI: mask_pitch < width
    roi = (_lib.Roi * 1)(_lib.Roi(0, 0, 20, 20))
    corners = torch.zeros((1, 10, 2), dtype=torch.float32, device="cuda")
    counts = torch.zeros((1,), dtype=torch.int32, device="cuda")
    rc = gpu.lib.tbdk_gftt_rois_masked(gpu.handle, C.c_void_p(img.data_ptr()), W, H, W, C.c_void_p(good.data_ptr()),
                                       W - 1, roi, 1, C.byref(det.prm), C.c_void_p(corners.data_ptr()),
                                       C.c_void_p(counts.data_ptr()), None)
    assert rc == _lib.TBDK_EINVAL
    rc = gpu.lib.tbdk_gftt_rois_masked(gpu.handle, C.c_void_p(img.data_ptr()), W, H, W, C.c_void_p(good.data_ptr()),
                                       W, roi, 1, C.byref(det.prm), C.c_void_p(corners.data_ptr()),
                                       C.c_void_p(counts.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0
