"""GPU: the chain morphology and connected components are for, on the 64x48 base sequence of tests/_mog2_cases.py:
BackgroundSubtractorMOG2.apply -> mask == 255 -> morphology_ex(OPEN, 3x3) -> connected_components_with_stats ->
detections_from_stats(min_area=6) -> TbdLoop.step.  Per frame the boxes equal the numpy chain's (_mog2_oracle ->
_morph_oracle -> _cc_oracle), the loop accepts them, and it holds a track on the moving rectangle once the
rectangle has been detected for the loop's confirmation delay."""
import numpy as np
import pytest
import torch

import _cc_oracle as CO
import _mog2_cases as GC
import _mog2_oracle as M2
import _morph_oracle as MO

pytestmark = pytest.mark.gpu

MIN_AREA = 6


def rectangle(t):
    """the bright 10 x 12 rectangle of _mog2_cases.gray_frame: (x, y, w, h)"""
    return 8 + (3 * t) % 40, 6, 10, 12


def overlap(a, b):
    w = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
    h = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    return max(w, 0) * max(h, 0)


def numpy_boxes(mask):
    opened = MO.morphology_ex(((mask == 255) * 255).astype(np.uint8), MO.OPEN, np.ones((3, 3), np.uint8))
    n, _, stats, _ = CO.connected_components_with_stats(opened, 8, CO.CCL_DEFAULT)
    return [(l, *stats[l, :4].tolist()) for l in range(1, n) if stats[l, 4] >= MIN_AREA]


def test_mog2_mask_to_boxes_to_the_tbd_loop(gpu):
    from opencv_amd import bgsegm, imgproc, tbd

    case = GC.cases()[0]
    assert case["name"] == "8UC1 history 12" and (case["w"], case["h"]) == (GC.W, GC.H)
    frames = GC.case_frames(case)
    want_masks = M2.expected(0)[0]
    sub = bgsegm.BackgroundSubtractorMOG2(history=12, ctx=gpu)
    cfg = tbd.default_config(GC.W, GC.H)
    loop = tbd.TbdLoop(cfg, ctx=gpu)
    delay = cfg.track_age_threshold
    kernel = imgproc.get_structuring_element(imgproc.MORPH_RECT, (3, 3))
    seen, confirmed, total = 0, 0, 0
    for t, frame in enumerate(frames):
        img = torch.from_numpy(frame).cuda()
        mask = sub.apply(img)
        fg = ((mask == 255) * 255).to(torch.uint8)
        opened = imgproc.morphology_ex(fg, imgproc.MORPH_OPEN, kernel, ctx=gpu)
        n, labels, stats, cent = imgproc.connected_components_with_stats(opened, max_labels=256, ctx=gpu)
        dets = bgsegm.detections_from_stats(stats, n, min_area=MIN_AREA)
        assert np.array_equal(mask.cpu().numpy(), want_masks[t]), t
        want = numpy_boxes(want_masks[t])
        assert [(int(d["id"]), int(d["x"]), int(d["y"]), int(d["width"]), int(d["height"])) for d in dets] == want, t
        assert (dets["confidence"] == 1.0).all()
        total += len(dets)
        loop.step(img, t, dets)  # raises unless TBDK_OK
        rect = rectangle(t)
        # what the subtractor sees of the rectangle is its leading edge, a strip 3 pixels wide and 12 high
        hit = any(overlap(rect, (d["x"], d["y"], d["width"], d["height"])) >= 30 for d in dets)
        seen = seen + 1 if hit else 0
        if seen > delay:
            tracks = [k for k in loop.tracks() if k["age"] >= delay and
                      overlap(rect, (k["x"], k["y"], k["width"], k["height"])) > 0]
            assert tracks, (t, loop.tracks())
            confirmed += 1
    # the chain is not empty, and the rectangle's edge was seen long enough to be confirmed (frames 5..12)
    assert total >= 10 and confirmed >= 1 and delay >= 1, (total, confirmed, delay)
