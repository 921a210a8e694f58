"""The TBD loop with ctx option "tbd_subpix": every corner set the loop's GFTT
produces is refined by cornerSubPix on the whole frame before PyrLK reads it.
Against the oracle pipeline: oracle/tbd_loop_oracle.KltTbdLoop unchanged, its
GFTT pointed at tests/_subpix_oracle.gftt_rois_subpix (the oracle's gftt_rois
followed by the numpy restatement of cornerSubPix).  The case is _loop_pair's
baseline: 320x240, 12 objects, 12 frames, seed 31, a tenth of the detections
dropped, bounds at the frame."""
import pytest

import _loop_pair as LP
import _subpix_oracle as SO

pytestmark = pytest.mark.gpu

W, H, N, F, SEED, DROP = 320, 240, 12, 12, 31, 0.1
CFG = {"bounds_xmax": W, "bounds_ymax": H}
WIN = 10  # lkdemo's window
# found on the oracle alone (the unrefined run enters 31343 PyrLK points and loses 11):
ORACLE_SEEN = (8814, 5254)           # corners the oracle's GFTT calls returned, and how many the refinement moved
ORACLE_ACTIVITY = (31352, 8, 125)    # the refined run's PyrLK points entered, lost, and predictions made


def oracle_subpix_run(monkeypatch, win):
    """The oracle pipeline over the sequence with every GFTT followed by
    cornerSubPix (win, win) on the frame.  A runner of its own:
    _loop_pair.oracle_run's cache key knows no refinement."""
    seen = {"corners": 0, "moved": 0}

    def gftt_rois(frame, rois, max_corners=256, quality=0.01, min_distance=3.0):
        plain = SO._gftt_rois(frame, rois, max_corners, quality, min_distance)
        out = SO.gftt_rois_subpix(frame, rois, max_corners, quality, min_distance, win=(win, win))
        seen["corners"] += sum(len(c) for c in out)  # (GIL: the oracle's pool may call this from several threads)
        seen["moved"] += sum(int((a != b).any(1).sum()) for a, b in zip(plain, out))
        return out

    monkeypatch.setattr(LP.L.O, "gftt_rois", gftt_rois)
    ofr, ogt, keep = LP.sequence(SEED, W, H, N, F, DROP)
    ora = LP.L.KltTbdLoop(W, H, nthreads=1, **LP.oracle_kwargs(CFG))
    ms, ps, rs = [], [], []
    for f in range(F):
        ms.append(dict(ora.step(ofr[f], f, LP.L.detections(ogt[f], f, keep[f]))))
        ps.append(dict(ora.preds))
        rs.append(tuple(ora.track_rows()))
    monkeypatch.undo()
    return LP.OracleRun(tuple(ms), tuple(ps), tuple(rs), ()), seen


@pytest.fixture(scope="module")
def inputs(gpu):
    return LP.gpu_inputs(gpu, W, H, N, F, SEED, DROP)


_refined = []  # the refined oracle run, computed once


@pytest.fixture
def refined_oracle(monkeypatch):
    if not _refined:
        _refined.append(oracle_subpix_run(monkeypatch, WIN))
    run, seen = _refined[0]
    # what the oracle alone does on this input: the refinement moves corners, and
    # the loop that tracks them differs from the unrefined one
    a, base = LP.activity(run), LP.activity(LP.oracle_run(W, H, N, F, SEED, DROP, CFG))
    assert (seen["corners"], seen["moved"]) == ORACLE_SEEN, seen
    assert base["lk_points"] == 31343, base
    assert (a["lk_points"], a["lost"], a["preds"]) == ORACLE_ACTIVITY, a
    plain = LP.oracle_run(W, H, N, F, SEED, DROP, CFG)
    assert run.preds != plain.preds and (a["lk_points"], a["lost"]) != (base["lk_points"], base["lost"])
    return run




@pytest.fixture
def subpix_on(gpu):
    """tbd_subpix = WIN for the loops a test creates (read by tbdk_tbd_create), 0 again after it: the context is shared"""
    gpu.set_option("tbd_subpix", WIN)
    yield
    gpu.set_option("tbd_subpix", 0)


def check_frame(loop, m, ora, f):
    gm, om = LP.gpu_metrics(m), ora.metrics[f]
    assert gm == om, f"frame {f}: metrics {gm} vs oracle {om}"
    gp, op = loop.predictions(), ora.preds[f]
    assert gp.keys() == op.keys(), f"frame {f}: predicted tracks differ"
    for k, (cx, cy) in gp.items():
        assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= LP.PRED_TOL, f"frame {f} track {k}"
    assert LP.gpu_rows(loop.tracks()) == list(ora.rows[f]), f"frame {f}: tracks differ"


def test_step_ahead_with_subpix(gpu, inputs, refined_oracle, subpix_on):
    import torch
    from opencv_amd import tbd

    frames, dets, _ = inputs
    loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    for f in range(F):
        m = loop.step(frames[f], f, dets[f], next_frame=frames[f + 1] if f + 1 < F else None)
        check_frame(loop, m, refined_oracle, f)
    torch.cuda.synchronize()


def test_run_with_subpix(gpu, inputs, refined_oracle, subpix_on):
    import torch
    from opencv_amd import tbd

    frames, dets, _ = inputs
    loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    ms = loop.run([frames[f] for f in range(F)], 0, dets)
    assert [LP.gpu_metrics(m) for m in ms] == list(refined_oracle.metrics)
    assert LP.gpu_rows(loop.tracks()) == list(refined_oracle.rows[F - 1])
    gp, op = loop.predictions(), refined_oracle.preds[F - 1]
    assert gp.keys() == op.keys()
    for k, (cx, cy) in gp.items():
        assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= LP.PRED_TOL, k
    torch.cuda.synchronize()


def test_option_off_is_the_unrefined_loop(gpu, inputs):
    import torch
    from opencv_amd import tbd

    frames, dets, seq = inputs
    ora = LP.oracle_run(W, H, N, F, SEED, DROP, CFG, seq)
    gpu.set_option("tbd_subpix", WIN)
    gpu.set_option("tbd_subpix", 0)  # back at the default before the loop is created
    loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    gpu.timing_enable(True)
    try:
        for f in range(F):
            m = loop.step(frames[f], f, dets[f], next_frame=frames[f + 1] if f + 1 < F else None)
            check_frame(loop, m, ora, f)
        torch.cuda.synchronize()
        assert gpu.timing_calls("corner_sub_pix") == 0 and gpu.timing_calls("gftt") > 0  # nothing new is launched
    finally:
        gpu.timing_enable(False)


def test_option_is_read_at_create_and_validated(gpu, inputs):
    import torch
    from opencv_amd import _lib, tbd

    frames, dets, _ = inputs
    for bad in (-1, 16):
        with pytest.raises(_lib.TbdkError):
            gpu.set_option("tbd_subpix", bad)
    try:
        gpu.set_option("tbd_subpix", 15)
        with pytest.raises(_lib.TbdkError):  # 32 < 2 * 15 + 5 rows: cornerSubPix's size rule
            tbd.TbdLoop(tbd.default_config(64, 32), ctx=gpu)
        gpu.set_option("tbd_subpix", WIN)
        loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    finally:
        gpu.set_option("tbd_subpix", 0)
    gpu.timing_enable(True)
    try:
        for f in range(3):  # the loop keeps the value it was created with
            loop.step(frames[f], f, dets[f])
        torch.cuda.synchronize()
        assert gpu.timing_calls("corner_sub_pix") > 0
    finally:
        gpu.timing_enable(False)
