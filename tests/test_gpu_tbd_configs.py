"""The native TBD loop against the independent oracle pipeline across its
configuration space (tests/test_gpu_tbd_e2e.py compares them at
tbdk_tbd_default_config only).

The case table is tests/_loop_pair.py's CASES: windows that send the loop's
segmented PyrLK launches to the generic LDS kernel (3, 5, even) or to other
lk_multi instances (7 points per wave at window 9, 2 at 31), pyramid depths 0
to 4 with frames too small for the requested depth, GFTT / refresh / PyrLK
termination / fit gate settings, a slot pool smaller than the track count,
kernel routing and launch paths by context option.  Small inputs (12 frames,
12 objects, 320x240 unless the case says otherwise, seed 31, 10 % of the
detections dropped, bounds = the frame).  Per frame, as run_pair states:
metrics equal, the same tracks predicted with centres within 1e-4 px, every
track row equal, through step(next_frame=...) and through tbdk_tbd_run.  The
oracle alone must be active in every case (check_oracle_activity; also
checked without a GPU by tests/test_tbd_loop_oracle.py).

Then the borrowed level 0 (ctx option tbd_borrow_l0) over the same space: a
window or kernel the several-points-per-wave kernel does not cover falls back
to the padded copy, supported windows other than 21 borrow and agree with the
padded path and the oracle, and the frame-size gate holds.  And
tbdk_tbd_create's documented argument limits (include/tbdk.h)."""
import ctypes as C

import pytest
import torch

import _loop_pair as LP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", LP.CASE_IDS)
def test_tbd_loop_equals_oracle_pipeline_config(gpu, cid):
    case = LP.BY_ID[cid]
    act = LP.check_oracle_activity(case)  # the case does something, by the oracle's account alone
    s = LP.run_pair(gpu, case.W, case.H, case.N, case.F, case.seed, case.drop, cfg=case.cfg, options=case.options)
    print(f"{cid}: oracle {act}, worst prediction error {s['pred_err']:.3g} px (bound {LP.PRED_TOL})")


def _run_split(gpu, case_args, cfg, options):
    """tbdk_tbd_run over a sequence as two run calls and a final step (a
    borrowing run hands its last frame's level 0 over when it ends): per-frame
    metrics and the final track rows, compared with the oracle's."""
    from opencv_amd import tbd

    W, H, N, F, seed, drop = case_args
    frames, dets, seq = LP.gpu_inputs(gpu, W, H, N, F, seed, drop)
    ora = LP.oracle_run(W, H, N, F, seed, drop, cfg, seq)
    assert LP.activity(ora)["preds"] > 0 and LP.activity(ora)["lk_points"] > 0
    k = F // 3
    with LP.ctx_options(gpu, options):
        loop = tbd.TbdLoop(tbd.default_config(W, H, **cfg), ctx=gpu)
        ms = list(loop.run([frames[f] for f in range(k)], 0, dets[:k]))
        ms += list(loop.run([frames[f] for f in range(k, F - 1)], k, dets[k:F - 1]))
        ms.append(loop.step(frames[F - 1], F - 1, dets[F - 1]))
        got = ([LP.gpu_metrics(m) for m in ms], LP.gpu_rows(loop.tracks()))
        torch.cuda.synchronize()
        del loop
    assert got[0] == list(ora.metrics), "metrics differ from the oracle's"
    assert got[1] == list(ora.rows[F - 1]), "final tracks differ from the oracle's"
    return got


def _frame_cfg(W, H, **cfg):
    return dict({"bounds_xmax": W, "bounds_ymax": H}, **cfg)


@pytest.mark.parametrize("cfg,options", [
    ({"win": 5}, {}),
    ({"win": 8}, {}),
    ({}, {"lk_impl": 1}),
    ({}, {"lk_impl": 2}),
], ids=["win5", "win8", "lk_impl1", "lk_impl2"])
def test_tbd_run_borrow_falls_back_on_unsupported_kernel(gpu, cfg, options):
    """tbd_borrow_l0 = 1 with a window lk_multi has no instance for, or with
    lk_impl naming another kernel: tbdk_tbd_run keeps the padded copy (it
    returned TBDK_EINVAL at its first PyrLK) and gives the results of
    tbd_borrow_l0 = 0, which are the oracle's."""
    args = (320, 240, 12, 12, 31, 0.1)
    c = _frame_cfg(320, 240, **cfg)
    off = _run_split(gpu, args, c, dict(options, tbd_borrow_l0=0))
    on = _run_split(gpu, args, c, dict(options, tbd_borrow_l0=1))
    assert on == off


@pytest.mark.parametrize("W,H,N,F,seed,drop,win,extra", [
    (320, 240, 48, 18, 15, 0.0, 7, {}),   # many objects on a small frame: windows on every edge
    (96, 80, 3, 12, 31, 0.1, 31, {}),     # passes the 2 * (win + 2) gate; almost every window crosses an edge
    (320, 240, 12, 12, 31, 0.1, 21, {"max_level": 0}),  # one level: the borrowed frame is the whole pyramid
    (333, 251, 12, 12, 31, 0.1, 9, {"max_level": 3}),   # odd pitch and size under levels 1..3
], ids=["win7_320x240", "win31_96x80", "win21_level0", "win9_level3_333x251"])
def test_tbd_run_borrowed_level0_other_windows(gpu, W, H, N, F, seed, drop, win, extra):
    """The borrowed level 0 at supported windows other than 21 (and at window
    21 with other depths): the same frames as the padded copy, across
    consecutive run calls and a step after them, and both equal to the oracle
    pipeline."""
    assert W >= 2 * (win + 2) and H >= 2 * (win + 2)  # the loop does borrow
    c = _frame_cfg(W, H, win=win, **extra)
    off = _run_split(gpu, (W, H, N, F, seed, drop), c, {"tbd_borrow_l0": 0})
    on = _run_split(gpu, (W, H, N, F, seed, drop), c, {"tbd_borrow_l0": 1})
    assert on == off


def test_tbd_run_borrow_size_gate(gpu):
    """A frame narrower than 2 * (win + 2) (64x60, window 31): the option on equals the option off."""
    W, H, win = 64, 60, 31
    assert W < 2 * (win + 2)
    c = _frame_cfg(W, H, win=win)
    off = _run_split(gpu, (W, H, 2, 12, 31, 0.0), c, {"tbd_borrow_l0": 0})
    on = _run_split(gpu, (W, H, 2, 12, 31, 0.0), c, {"tbd_borrow_l0": 1})
    assert on == off


@pytest.mark.parametrize("field,value", [
    ("win", 2), ("win", 32),
    ("max_corners", 0), ("max_corners", 257),
    ("max_tracks", 0),
    ("redetect_every", 0),
    ("time_window_size", 0), ("time_window_size", 65),  # kMaxTimeWindow = 64 (tbd_tracker.hpp)
    ("max_level", -1),
    ("min_distance", -1.0), ("min_distance", float("nan")),
    ("quality_level", 0.0), ("quality_level", -0.01), ("quality_level", float("nan")),
    ("width", 0), ("height", -4),
])
def test_tbd_create_rejects_out_of_range(gpu, field, value):
    """The limits include/tbdk.h states for tbdk_tbd_config: TBDK_EINVAL and
    no loop, at creation (a negative min_distance or a quality_level <= 0
    failed only at the first step's GFTT)."""
    from opencv_amd import _lib, tbd

    c = tbd.default_config(320, 240)
    assert hasattr(c, field)
    setattr(c, field, value)
    h = C.c_void_p(0xDEAD)
    rc = gpu.lib.tbdk_tbd_create(gpu.handle, C.byref(c), C.byref(h))
    assert rc == _lib.TBDK_EINVAL and not h.value


@pytest.mark.parametrize("field,value", [
    ("win", 3), ("win", 31), ("max_corners", 1), ("max_corners", 256), ("max_tracks", 1), ("redetect_every", 1),
    ("time_window_size", 1), ("time_window_size", 64), ("max_level", 0), ("min_distance", 0.0),
])
def test_tbd_create_accepts_the_limits(gpu, field, value):
    from opencv_amd import tbd

    loop = tbd.TbdLoop(tbd.default_config(320, 240, **{field: value}), ctx=gpu)
    assert loop.handle.value
    del loop
