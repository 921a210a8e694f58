"""The TBD loop with ctx option "tbd_fit_ransac" = 500: each track's KLT fit is
cv::estimateRigidTransform's RANSAC consensus over its tracked corners instead
of the least-squares fit over all of them.

The GPU loop is compared with the independent oracle pipeline
(oracle/tbd_loop_oracle.KltTbdLoop) whose fit module is replaced, here in the
test, by a shim over the restatement tests/_rigid_oracle.py (a NaN matrix when
there is no transform: the pipeline then makes no prediction for that track).
Per frame, the equalities of tests/test_gpu_tbd_e2e.run_pair: metrics and track
rows exact, prediction centres within 1e-4 px; tbdk_tbd_run equals stepping.

640x480, 16 objects, 8 frames (re-detection at frames 0 and 5).  The seed was
chosen on the CPU from the two oracle pipelines alone: the RANSAC loop's
predictions differ from the least-squares loop's by up to 1.4 px (8 track-frames
by more than 0.01 px), and no residual of any evaluated hypothesis is within
2.5e-3 px of the inlier threshold, so the exact comparison is well posed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tbd_loop_oracle as L  # noqa: E402
import _rigid_oracle as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, N, F, SEED = 640, 480, 16, 8, 20261021
METRIC_KEYS = ("tp", "fn", "fp", "gt", "ntracks", "lk_points", "klt_points", "klt_predicted", "redetected")


class RansacFitShim:
    """stands in for oracle/box_fit_oracle inside tbd_loop_oracle"""
    margins = [np.inf, np.inf]
    propagate_box = staticmethod(R.BF.propagate_box)

    @classmethod
    def get_rt_matrix(cls, a, b):
        r = R.estimate(a, b, 500, 0.5)
        cls.margins = [min(cls.margins[0], r.resid_margin), min(cls.margins[1], r.collin_margin)]
        return r.M if r.found else np.full((2, 3), np.nan)


def _rows(tracks):
    return [(t["id"], t["x"], t["y"], t["width"], t["height"], t["pred_x"], t["pred_y"], t["pred_w"],
             t["pred_h"], t["age"], t["total_visible"], t["npoints"]) for t in tracks]


@pytest.fixture(scope="module")
def sequence(gpu):
    from opencv_amd import klt, tbd

    frames, gt = klt.synth_render(SEED, W, H, N, 0, F, ctx=gpu)
    ofr, ogt = L.O.synth(SEED, W, H, N, 0, F)
    assert np.array_equal(frames.cpu().numpy(), ofr) and np.array_equal(gt.numpy(), ogt)
    dets = [tbd.detections_from_gt(ogt[f]) for f in range(F)]
    return frames, ofr, ogt, dets


def gpu_loop(gpu, sequence, ransac):
    """step the GPU loop; ransac None: the option is never touched"""
    from opencv_amd import tbd

    frames, _, _, dets = sequence
    if ransac is not None:
        gpu.set_option("tbd_fit_ransac", ransac)
    try:
        loop = tbd.TbdLoop(tbd.default_config(W, H), ctx=gpu)
        batch = tbd.TbdLoop(tbd.default_config(W, H), ctx=gpu)
    finally:
        if ransac is not None:
            gpu.set_option("tbd_fit_ransac", 0)  # taken at create; the shared context goes back to its default
    out = []
    for f in range(F):
        m = loop.step(frames[f], f, dets[f], next_frame=frames[f + 1] if f + 1 < F else None)
        out.append(({k: getattr(m, k) for k in METRIC_KEYS}, loop.predictions(), _rows(loop.tracks())))
    ms = batch.run([frames[f] for f in range(F)], 0, dets)  # tbdk_tbd_run equals stepping
    assert [{k: getattr(m, k) for k in METRIC_KEYS} for m in ms] == [o[0] for o in out]
    assert _rows(batch.tracks()) == out[-1][2]
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def default_loop(gpu, sequence):
    return gpu_loop(gpu, sequence, None)


def test_ransac_loop_equals_oracle_pipeline(gpu, sequence, default_loop, monkeypatch):
    _, ofr, ogt, _ = sequence
    got = gpu_loop(gpu, sequence, 500)
    RansacFitShim.margins = [np.inf, np.inf]
    monkeypatch.setattr(L, "BF", RansacFitShim)
    ora = L.KltTbdLoop(W, H, nthreads=min(16, os.cpu_count() or 1))
    npred = 0
    for f in range(F):
        om = ora.step(ofr[f], f, L.detections(ogt[f], f, None))
        gm, gp, rows = got[f]
        assert gm == om, f"frame {f}: metrics {gm} vs oracle {om}"
        assert gp.keys() == ora.preds.keys(), f"frame {f}: predicted tracks differ"
        for k, (cx, cy) in gp.items():
            assert max(abs(cx - ora.preds[k][0]), abs(cy - ora.preds[k][1])) <= 1e-4, (f, k)
        assert rows == ora.track_rows(), f"frame {f}: tracks differ"
        npred += len(gp)
    assert npred > 6 * N
    # the precondition of the exact comparison (module docstring)
    assert RansacFitShim.margins[0] >= 1e-4 and RansacFitShim.margins[1] >= 1e-9, RansacFitShim.margins
    # the option is not a no-op: some track-frame's prediction moved by more than 0.01 px
    worst = max(max(abs(a[k][0] - b[k][0]), abs(a[k][1] - b[k][1]))
                for (_, a, _), (_, b, _) in zip(got, default_loop) for k in a.keys() & b.keys())
    print(f"largest prediction change vs the least-squares loop: {worst:.4f} px")
    assert worst > 0.01


def test_option_zero_is_the_default_loop(gpu, sequence, default_loop):
    assert gpu_loop(gpu, sequence, 0) == default_loop


def test_option_range(gpu):
    from opencv_amd import _lib

    for bad in (-1, 10001):
        with pytest.raises(_lib.TbdkError, match="TBDK_EINVAL"):
            gpu.set_option("tbd_fit_ransac", bad)
    gpu.set_option("tbd_fit_ransac", 10000)
    gpu.set_option("tbd_fit_ransac", 0)
