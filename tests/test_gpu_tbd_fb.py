"""The TBD loop with ctx option "tbd_fb_check": every PyrLK launch of the loop is
followed by the backward pass of the forward-backward check, and a corner that
fails it leaves its track's set before the fit.

The GPU loop is compared with the independent oracle pipeline with the check
(tests/_fb_oracle.FbKltTbdLoop, composed from the oracle's PyrLK).  Per frame,
the equalities of tests/_loop_pair.run_pair: metrics and track rows exact, the
same tracks predicted, centres within _loop_pair.PRED_TOL (1e-4 px, the fit's
closed form against the oracle's eigen-solve).

640x480, 16 objects, 8 frames (re-detection at frames 0 and 5): seed 20261022
at option 1024 (1.0 px) and seed 20261023 at 256 (0.25 px), then one run each
for the generic kernel (window 5, max_level 1), window 9, lk_impl 2, loop
pyramids with derivative planes, no speculative look-ahead, early look-ahead on
every frame, borrowed level 0 through tbdk_tbd_run, a pool of 10 slots,
max_level 0, and the RANSAC fit together with the check.
tests/test_fb_oracle.py shows on the CPU that the oracle rejects points of
every kind in each of them and that its predictions move by more than 0.01 px."""
import pytest
import torch

import _fb_oracle as F
import _loop_pair as LP

pytestmark = pytest.mark.gpu

W, H, N, NF = F.TW, F.TH, F.TN, F.TF


class options:
    """ctx options for a block: tbd_fb_check / tbd_fit_ransac (taken at loop
    creation) and a case's others, all back at their defaults afterwards"""

    def __init__(self, gpu, fb=None, ransac=0, other=None):
        self.gpu = gpu
        self.set = dict(other or {})
        self.back = {k: LP.CTX_DEFAULTS[k] for k in self.set}
        if fb is not None:
            self.set["tbd_fb_check"], self.back["tbd_fb_check"] = fb, 0
        if ransac:
            self.set["tbd_fit_ransac"], self.back["tbd_fit_ransac"] = ransac, 0

    def __enter__(self):
        for k, v in self.set.items():
            self.gpu.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.back.items():
            self.gpu.set_option(k, v)
        return False


_inputs = {}


def inputs(gpu, seed):
    if seed not in _inputs:
        from opencv_amd import klt, tbd
        import numpy as np

        frames, gt = klt.synth_render(seed, W, H, N, 0, NF, ctx=gpu)
        ofr, ogt = F.loop_sequence(seed)
        assert np.array_equal(frames.cpu().numpy(), ofr) and np.array_equal(gt.numpy(), ogt)
        _inputs[seed] = (frames, [tbd.detections_from_gt(ogt[f]) for f in range(NF)])
    return _inputs[seed]


def gpu_loop(gpu, seed, fb, cfg=None, other=None, ransac=0, how="ahead"):
    """per frame (metrics, predictions, track rows); how: "ahead" steps with
    next_frame, "step" without, "run" tbdk_tbd_run, "run_host" tbdk_tbd_run_host
    (the last two: predictions and rows of the last frame only)"""
    from opencv_amd import tbd

    frames, dets = inputs(gpu, seed)
    out = []
    with options(gpu, fb, ransac, other):
        loop = tbd.TbdLoop(tbd.default_config(W, H, **(cfg or {})), ctx=gpu)
        if how in ("run", "run_host"):
            ms = loop.run([frames[f] for f in range(NF)], 0, dets) if how == "run" else \
                loop.run_host(frames.cpu().contiguous(), 0, dets)
            out = [(LP.gpu_metrics(m), None, None) for m in ms]
            out[-1] = (out[-1][0], loop.predictions(), LP.gpu_rows(loop.tracks()))
        else:
            for f in range(NF):
                nxt = frames[f + 1] if how == "ahead" and f + 1 < NF else None
                m = loop.step(frames[f], f, dets[f], next_frame=nxt)
                out.append((LP.gpu_metrics(m), loop.predictions(), LP.gpu_rows(loop.tracks())))
        torch.cuda.synchronize()
        del loop
    return out


def assert_equals_oracle(got, ora, what):
    npred = 0
    for f, (gm, gp, rows) in enumerate(got):
        assert gm == ora.metrics[f], f"{what} frame {f}: metrics {gm} vs oracle {ora.metrics[f]}"
        if gp is None:
            continue
        op = ora.preds[f]
        assert gp.keys() == op.keys(), f"{what} frame {f}: predicted tracks differ"
        for k, (cx, cy) in gp.items():
            assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= LP.PRED_TOL, (what, f, k, (cx, cy), op[k])
        assert rows == list(ora.rows[f]), f"{what} frame {f}: tracks differ"
        npred += len(gp)
    return npred


@pytest.fixture(scope="module")
def untouched(gpu):
    """the loop on a context whose tbd_fb_check was never touched by this module"""
    return gpu_loop(gpu, 20261022, None)


def test_untouched_loop_is_the_plain_oracle_pipeline(gpu, untouched):
    """(first in the module: the fixture runs before any test here sets the option)"""
    assert_equals_oracle(untouched, F.loop_oracle(20261022, 0, {}), "option never set")


@pytest.mark.parametrize("cid", [c.id for c in F.LOOP_CASES])
def test_checked_loop_equals_oracle_pipeline(gpu, cid):
    c = F.LOOP_BY_ID[cid]
    ora = F.loop_oracle(c.seed, c.opt, c.cfg, c.ransac)
    tot = {k: sum(x[k] for x in ora.log) for k in ora.log[0]}
    print(f"{cid}: oracle {tot}")
    if c.via_run:
        got = gpu_loop(gpu, c.seed, c.opt, c.cfg, c.options, c.ransac, how="run")
        assert_equals_oracle(got, ora, cid + " run")
        return
    got = gpu_loop(gpu, c.seed, c.opt, c.cfg, c.options, c.ransac)
    assert assert_equals_oracle(got, ora, cid) == sum(m["klt_predicted"] for m in ora.metrics) > 0
    # tbdk_tbd_run agrees with stepping
    run = gpu_loop(gpu, c.seed, c.opt, c.cfg, c.options, c.ransac, how="run")
    assert [r[0] for r in run] == [g[0] for g in got] and run[-1][2] == got[-1][2] and run[-1][1] == got[-1][1]


def test_entry_points_agree(gpu):
    """tbdk_tbd_step, _step_ahead, _run and _run_host with the option on"""
    ahead = gpu_loop(gpu, 20261022, 1024)
    assert gpu_loop(gpu, 20261022, 1024, how="step") == ahead
    for how in ("run", "run_host"):
        r = gpu_loop(gpu, 20261022, 1024, how=how)
        assert [x[0] for x in r] == [x[0] for x in ahead] and r[-1][1:] == ahead[-1][1:], how


def test_option_is_not_a_no_op(gpu, untouched):
    got = gpu_loop(gpu, 20261022, 1024)
    assert sum(g[0]["klt_points"] for g in got) < sum(u[0]["klt_points"] for u in untouched)
    worst = max(max(abs(a[k][0] - b[k][0]), abs(a[k][1] - b[k][1]))
                for (_, a, _), (_, b, _) in zip(got, untouched) for k in a.keys() & b.keys())
    print(f"largest prediction change vs the unchecked loop: {worst:.4f} px")
    assert worst > 0.01


def test_option_zero_is_the_untouched_loop(gpu, untouched):
    assert gpu_loop(gpu, 20261022, 0) == untouched


def test_option_range(gpu):
    from opencv_amd import _lib

    for bad in (-1, 1048577):
        with pytest.raises(_lib.TbdkError, match="TBDK_EINVAL"):
            gpu.set_option("tbd_fb_check", bad)
    gpu.set_option("tbd_fb_check", 1048576)
    gpu.set_option("tbd_fb_check", 0)
