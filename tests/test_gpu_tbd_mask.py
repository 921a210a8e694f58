"""The TBD loop under a static corner mask (tbdk_tbd_set_corner_mask) against the
oracle pipeline: oracle/tbd_loop_oracle.KltTbdLoop unchanged, its GFTT pointed
at the masked restatement (tests/_gftt_mask_oracle.py).  The case is
_loop_pair's baseline: 320x240, 12 objects, 12 frames, seed 31, a tenth of the
detections dropped, bounds at the frame."""
import numpy as np
import pytest

import _gftt_mask_oracle as MO
import _loop_pair as LP

pytestmark = pytest.mark.gpu

W, H, N, F, SEED, DROP = 320, 240, 12, 12, 31, 0.1
CFG = {"bounds_xmax": W, "bounds_ymax": H}


def static_mask():
    """byte 1 everywhere except x < 100 or y >= H - 40"""
    m = np.ones((H, W), np.uint8)
    m[:, :100] = 0
    m[H - 40:, :] = 0
    return m


def oracle_masked_run(monkeypatch, mask):
    """The oracle pipeline over the sequence with every GFTT under `mask`
    (None: unmasked), and what its GFTT calls saw: (ROIs, ROIs without a corner).
    A runner of its own: _loop_pair.oracle_run's cache key knows no mask."""
    seen = {"rois": 0, "empty": 0}

    def gftt_rois(frame, rois, max_corners=256, quality=0.01, min_distance=3.0):
        out = MO.gftt_rois_masked(frame, mask, rois, max_corners, quality, min_distance)
        seen["rois"] += len(out)  # (GIL: the oracle's pool calls this from several threads)
        seen["empty"] += sum(len(c) == 0 for c in out)
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


_masked = []  # the masked oracle run, computed once


@pytest.fixture
def masked_oracle(monkeypatch):
    if not _masked:
        _masked.append(oracle_masked_run(monkeypatch, static_mask()))
    run, seen = _masked[0]
    # what the oracle alone does on this input: the mask removes corners, empties
    # some refreshed sets, and the loop still predicts
    a = LP.activity(run)
    assert (seen["rois"], seen["empty"]) == (42, 4), seen
    assert a["preds"] == 121 and sum(m["ntracks"] for m in run.metrics) == 137, (a, run.metrics)
    assert a["lk_points"] == 25184, a
    base = LP.activity(LP.oracle_run(W, H, N, F, SEED, DROP, CFG))
    assert base["lk_points"] == 31343, base
    return run


def check_frame(loop, m, ora, f):
    gm, om = LP.gpu_metrics(m), ora.metrics[f]
    assert gm == om, f"frame {f}: metrics {gm} vs oracle {om}"
    gp, op = loop.predictions(), ora.preds[f]
    assert gp.keys() == op.keys(), f"frame {f}: predicted tracks differ"
    for k, (cx, cy) in gp.items():
        assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= LP.PRED_TOL, f"frame {f} track {k}"
    assert LP.gpu_rows(loop.tracks()) == list(ora.rows[f]), f"frame {f}: tracks differ"


def test_step_ahead_under_mask(gpu, inputs, masked_oracle):
    import torch
    from opencv_amd import tbd

    frames, dets, _ = inputs
    loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    loop.set_corner_mask(torch.from_numpy(static_mask()).cuda())
    for f in range(F):
        m = loop.step(frames[f], f, dets[f], next_frame=frames[f + 1] if f + 1 < F else None)
        check_frame(loop, m, masked_oracle, f)
    torch.cuda.synchronize()


def test_run_under_mask(gpu, inputs, masked_oracle):
    import torch
    from opencv_amd import tbd

    frames, dets, _ = inputs
    loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    # a slice of a larger plane: odd offset, pitch > width
    big = torch.zeros((H + 7, W + 11), dtype=torch.uint8, device=frames.device)
    big[3:3 + H, 5:5 + W] = torch.from_numpy(static_mask()).cuda()
    loop.set_corner_mask(big[3:3 + H, 5:5 + W])
    ms = loop.run([frames[f] for f in range(F)], 0, dets)
    assert [LP.gpu_metrics(m) for m in ms] == list(masked_oracle.metrics)
    assert LP.gpu_rows(loop.tracks()) == list(masked_oracle.rows[F - 1])
    torch.cuda.synchronize()


def test_all_255_mask_is_the_unmasked_loop(gpu, inputs):
    import torch
    from opencv_amd import tbd

    frames, dets, seq = inputs
    ora = LP.oracle_run(W, H, N, F, SEED, DROP, CFG, seq)
    loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    loop.set_corner_mask(torch.full((H, W), 255, dtype=torch.uint8, device=frames.device))
    plain = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    for f in range(F):
        nxt = frames[f + 1] if f + 1 < F else None
        m = loop.step(frames[f], f, dets[f], next_frame=nxt)
        mp = plain.step(frames[f], f, dets[f], next_frame=nxt)
        assert LP.gpu_metrics(m) == LP.gpu_metrics(mp) == ora.metrics[f], f
        assert LP.gpu_rows(loop.tracks()) == LP.gpu_rows(plain.tracks()) == list(ora.rows[f]), f
    torch.cuda.synchronize()


def test_set_corner_mask_only_before_the_first_step(gpu, inputs):
    import torch
    from opencv_amd import _lib, tbd

    frames, dets, _ = inputs
    loop = tbd.TbdLoop(tbd.default_config(W, H, **CFG), ctx=gpu)
    mask = torch.from_numpy(static_mask()).cuda()
    loop.set_corner_mask(mask)
    loop.set_corner_mask(None)  # cleared again before the first step
    loop.set_corner_mask(mask)
    for bad in (mask[:, :W - 1], mask.to(torch.int32), mask.cpu(), mask[:, ::2]):
        with pytest.raises(_lib.TbdkError):
            loop.set_corner_mask(bad)
    loop.step(frames[0], 0, dets[0])
    with pytest.raises(_lib.TbdkError):
        loop.set_corner_mask(mask)
    with pytest.raises(_lib.TbdkError):
        loop.set_corner_mask(None)
    torch.cuda.synchronize()
