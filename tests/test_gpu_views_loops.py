"""The frame loops on pitched, unaligned frames (tests/_views.py): the TBD
loop's step / run (tests/_loop_pair.run_pair with its layout argument: the
frames are windows of one noise-filled buffer with a common pitch), with and
without the borrowed level 0 (ctx option tbd_borrow_l0: PyrLK reads the frame
itself, ipitch != w); tbd_step_image on a BGR window; the KLT tracker with every
frame a window.  Oracles and criteria are those of test_gpu_tbd_configs.py
(run_pair, PRED_TOL included), test_gpu_tbd_detect.py and
test_gpu_klt_tracker.py, unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import _klt_tracker_oracle as KO
import _loop_pair as LP
import _views as V
import test_gpu_tbd_detect as TD
from test_gpu_klt_tracker import assert_state, tracker

pytestmark = pytest.mark.gpu

# the default case and one each with window 9 and 31 (tests/test_tbd_loop_oracle.py holds
# check_oracle_activity for every case of LP.CASES on the CPU)
LOOP_CASES = ["baseline", "win9_level4", "win31_level1"]


@pytest.mark.parametrize("layout", ["odd_both", "vec4"])
@pytest.mark.parametrize("borrow", [0, 1])
@pytest.mark.parametrize("cid", LOOP_CASES)
def test_tbd_loop_on_views(gpu, cid, borrow, layout):
    """step(next_frame=...) and run() over pitched frames equal the oracle pipeline frame by frame"""
    case = LP.BY_ID[cid]
    LP.check_oracle_activity(case)  # on the oracle alone
    stats = LP.run_pair(gpu, case.W, case.H, case.N, case.F, case.seed, case.drop, case.cfg,
                        dict(case.options, tbd_borrow_l0=borrow), layout=layout)
    assert stats["preds"] > 0 and stats["pred_err"] <= LP.PRED_TOL


@pytest.mark.parametrize("layout", ["odd_both", "odd_base"])
def test_step_image_on_views(gpu, layout):
    """tbdk_tbd_step_image, the "colour" row of test_gpu_tbd_detect.py's table (HOG on the
    BGR frame itself), every frame a cn = 3 window (one BGR pixel in: first byte 3 mod
    16): detections, metrics, predictions and track rows equal the oracle pipeline's"""
    case, mode, thr = "colour", 1, -1.0
    assert (case, mode, thr) in TD.RUNS
    TD.check_conditions()
    size, make_gray = TD.CASES[case]
    loop = TD.gpu_loop(gpu, thr)
    loop.attach_detector(TD.gpu_hog(gpu), src_size=size, make_gray=make_gray, confidence_mode=mode)
    front, ref = TD.oracle_front(case), TD.oracle_run(case, mode, thr)
    for f, bgr in enumerate(TD.bgr_frames(size)):
        parent, view = V.window(bgr, layout, seed=f, device="cuda")
        before = V.snapshot(parent)
        m, dets = loop.step_image(view, f)
        _, rects, wts = front[f]
        got = np.stack([dets["x"], dets["y"], dets["width"], dets["height"]], 1) if len(dets) else np.zeros((0, 4))
        assert np.array_equal(got, rects), f"frame {f}: rects differ"
        assert np.array_equal(dets["confidence"], wts), f"frame {f}: confidences differ"
        om, op, orows = ref[f]
        assert TD.metrics_of(m) == om, f"frame {f}: metrics {TD.metrics_of(m)} vs oracle {om}"
        gp = loop.predictions()
        assert gp.keys() == op.keys(), f"frame {f}: predicted tracks differ"
        for k, (cx, cy) in gp.items():
            assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= 1e-4, f"frame {f} track {k}"
        assert TD.gpu_rows(loop.tracks()) == orows, f"frame {f}: tracks differ"
        torch.cuda.synchronize()
        assert torch.equal(parent, before)


@pytest.mark.parametrize("layout", list(V.LAYOUTS))
def test_klt_tracker_on_views(gpu, layout):
    """the "small" case of test_cases_frame_by_frame with every frame a window: ids,
    lengths, points, histories and statistics equal the oracle's after every step"""
    case = KO.CASES["small"]
    fr = KO.frames(case.seq)
    ref = KO.run_case(case)
    views = [V.window(fr[f], layout, seed=f, device="cuda") for f in range(case.nframes)]
    before = [V.snapshot(p) for p, _ in views]
    t = tracker(gpu, fr.shape[2], fr.shape[1], **case.cfg)
    for f in range(case.nframes):
        t.step(views[f][1])
        assert_state(t, ref.states[f], ref.stats[f], f"{layout} frame {f}")
    assert all(torch.equal(p, b) for (p, _), b in zip(views, before))


def test_pitch_below_the_row_is_refused(gpu):
    """tbdk_tbd_step / _step_ahead / _run, tbdk_tbd_step_image and tbdk_klt_tracker_step
    with pitch < row: TBDK_EINVAL, and the loop has not taken a step"""
    from opencv_amd import _lib, tbd

    W, H = 320, 240
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _, frame = V.window(np.zeros((H, W), np.uint8), "odd_both", device="cuda")
    _, bgr = V.window(np.zeros((H, W, 3), np.uint8), "odd_both", device="cuda")
    loop = TD.gpu_loop(gpu, -1.0)
    lib = gpu.lib
    m = _lib.FrameMetrics()
    dets = (_lib.Detection * 1)()
    assert lib.tbdk_tbd_step(loop.handle, frame.data_ptr(), W - 1, 0, dets, 0, C.byref(m), s) == _lib.TBDK_EINVAL
    for p, pn in ((W - 1, frame.stride(0)), (frame.stride(0), W - 1)):
        assert lib.tbdk_tbd_step_ahead(loop.handle, frame.data_ptr(), p, 0, dets, 0, frame.data_ptr(), pn, C.byref(m),
                                       s) == _lib.TBDK_EINVAL
    ptrs = (C.c_void_p * 1)(frame.data_ptr())
    offs = (C.c_int32 * 2)(0, 0)
    ms = (_lib.FrameMetrics * 1)()
    assert lib.tbdk_tbd_run(loop.handle, ptrs, W - 1, 0, dets, offs, 1, ms, s) == _lib.TBDK_EINVAL
    loop.attach_detector(TD.gpu_hog(gpu), make_gray=False, confidence_mode=1)
    n = C.c_int(-1)
    out = (_lib.Detection * 8)()
    assert lib.tbdk_tbd_step_image(loop._det, bgr.data_ptr(), 3 * W - 1, 0, out, 8, C.byref(n), C.byref(m), s) == \
        _lib.TBDK_EINVAL
    assert loop.tracks() == [] and loop.predictions() == {}
    t = tracker(gpu, W, H)
    assert lib.tbdk_klt_tracker_step(t.handle, frame.data_ptr(), W - 1, 0, s) == _lib.TBDK_EINVAL
    st = t.read()
    assert len(st.ids) == 0 and st.stats["frame_idx"] == -1
