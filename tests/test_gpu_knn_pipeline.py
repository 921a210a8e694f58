"""GPU: the fixed-camera chain with the KNN background model, on the 64x48 base sequence of tests/_mog2_cases.py:
BackgroundSubtractorKNN.apply -> mask == 255 -> morphology_ex(OPEN, 3x3) -> connected_components_with_stats ->
detections_from_stats(min_area=6) -> TbdLoop.step.  Per frame the mask and the boxes equal the numpy chain's
(_knn_oracle -> _morph_oracle -> _cc_oracle) and the loop accepts them; the chain sees the moving rectangle."""
import numpy as np
import pytest
import torch

import _knn_cases as KC
import _knn_oracle as KO
from test_gpu_blobs_pipeline import MIN_AREA, numpy_boxes, overlap, rectangle

pytestmark = pytest.mark.gpu


def test_knn_mask_to_boxes_to_the_tbd_loop(gpu):
    from opencv_amd import bgsegm, imgproc, tbd

    case = KC.cases()[0]
    assert case["name"] == "8UC1 history 500" and (case["w"], case["h"]) == (KC.W, KC.H)
    frames = KC.case_frames(case)
    want_masks = KO.expected(0)[0]
    sub = bgsegm.createBackgroundSubtractorKNN(ctx=gpu)
    loop = tbd.TbdLoop(tbd.default_config(KC.W, KC.H), ctx=gpu)
    kernel = imgproc.get_structuring_element(imgproc.MORPH_RECT, (3, 3))
    total, hits = 0, 0
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
        hits += any(overlap(rectangle(t), (d["x"], d["y"], d["width"], d["height"])) >= 30 for d in dets)
    # the chain is not empty, and it sees the rectangle's leading edge in most frames (the numpy chain says how many)
    assert total >= 48 and hits >= 24, (total, hits)
