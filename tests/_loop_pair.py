"""The GPU frame loop against the independent oracle pipeline, one sequence at
a time: the shared driver of tests/test_gpu_tbd_e2e.py (the bench's
configurations) and tests/test_gpu_tbd_configs.py (the configuration matrix),
and the matrix's case table with the conditions the oracle alone must meet
(tests/test_tbd_loop_oracle.py checks them without a GPU).

Both sides are built from the same loop-config overrides: tbd.default_config(W,
H, **cfg) for libtbdk, oracle/tbd_loop_oracle.py's KltTbdLoop(W, H, ...) for
the oracle (oracle_kwargs maps the field names that differ).  Nothing of the
GPU's output feeds the oracle: it runs the whole sequence first (oracle_run),
driving itself with its own predictions, and its per-frame records are what
every GPU frame is compared with."""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tbd_loop_oracle as L  # noqa: E402

METRIC_KEYS = ("tp", "fn", "fp", "gt", "ntracks", "lk_points", "klt_points", "klt_predicted", "redetected")
PRED_TOL = 1e-4  # px: the fit's closed form vs the oracle's eigen-solve (tests/test_gpu_box_fit.py)

# tbdk_tbd_config fields the oracle names differently, and the tracker's
_RENAMED = {"min_eig_threshold": "min_eig", "quality_level": "quality"}
_SAME = ("win", "max_level", "lk_iters", "lk_epsilon", "max_corners", "min_distance", "redetect_every", "min_points",
         "min_fit_points", "max_tracks")
_TRACKER = ("cost_of_non_assignment", "time_window_size", "track_age_threshold", "track_visibility_threshold",
            "track_confidence_threshold")
_BOUNDS = ("bounds_xmin", "bounds_xmax", "bounds_ymin", "bounds_ymax")

# the context options' defaults (opencv_amd/csrc/tbdk_internal.hpp, struct tbdk_ctx)
CTX_DEFAULTS = {
    "lk_impl": 0, "lk_scharr_fly": 0, "lk_seg_inline": 1, "lk_solo": 4, "pyr_fuse": 1, "gftt_inline": 1,
    "gftt_compact": 1, "tbd_pyr_derivs": 0, "tbd_zero_copy": 1, "tbd_fit_inline": 1, "tbd_fit_flag": 1,
    "tbd_early_gftt": 2, "tbd_borrow_l0": 0, "tbd_spec_lookahead": 1,
    "tbd_early_la": 1, "tbd_gftt_ahead": 1,
}


def oracle_kwargs(cfg):
    """Loop-config overrides (tbdk_tbd_config field names) -> KltTbdLoop keyword arguments."""
    kw = {}
    bounds = [0, 1280, 0, 720]  # tbdk_tbd_default_config's, the reference's hard-coded filter
    for k, v in cfg.items():
        if k in _BOUNDS:
            bounds[_BOUNDS.index(k)] = int(v)
        elif k in _RENAMED:
            kw[_RENAMED[k]] = v
        elif k in _SAME or k in _TRACKER:  # the tracker's go on as tracker_args
            kw[k] = v
        else:
            raise KeyError(f"loop-config field {k} has no oracle counterpart")
    kw["bounds"] = tuple(bounds)
    return kw


def sequence(seed, W, H, N, F, drop):
    """The oracle's rendering of the sequence, its ground truth and the kept detections' masks."""
    ofr, ogt = L.O.synth(seed, W, H, N, 0, F)
    rng = np.random.default_rng(seed)
    keep = [rng.random(N) >= drop for _ in range(F)]
    return ofr, ogt, keep


OracleRun = namedtuple("OracleRun", "metrics preds rows slots")  # one entry per frame each
_runs = {}


def oracle_run(W, H, N, F, seed, drop, cfg, seq=None):
    """The oracle pipeline over the whole sequence, computed once per
    (sequence, overrides) and shared: per frame its metrics, its predictions
    {track id: (cx, cy)}, its track rows and the slots in use."""
    key = (W, H, N, F, seed, drop, tuple(sorted(cfg.items())))
    if key not in _runs:
        ofr, ogt, keep = seq if seq is not None else sequence(seed, W, H, N, F, drop)
        ora = L.KltTbdLoop(W, H, nthreads=min(16, os.cpu_count() or 1), **oracle_kwargs(cfg))
        ms, ps, rs, ss = [], [], [], []
        for f in range(F):
            ms.append(dict(ora.step(ofr[f], f, L.detections(ogt[f], f, keep[f]))))
            ps.append(dict(ora.preds))
            rs.append(tuple(ora.track_rows()))
            ss.append(len(ora.slot))
        _runs[key] = OracleRun(tuple(ms), tuple(ps), tuple(rs), tuple(ss))
    return _runs[key]


def activity(run):
    """What the oracle did over a run, from its own metrics: predictions made,
    point sets refreshed, PyrLK points entered and lost."""
    m = run.metrics
    lk = sum(x["lk_points"] for x in m)
    return {"preds": sum(x["klt_predicted"] for x in m), "refreshed": sum(x["redetected"] for x in m),
            "lk_points": lk, "lost": lk - sum(x["klt_points"] for x in m)}


def gpu_rows(tracks):
    return [(t["id"], t["x"], t["y"], t["width"], t["height"], t["pred_x"], t["pred_y"], t["pred_w"],
             t["pred_h"], t["age"], t["total_visible"], t["npoints"]) for t in tracks]


def gpu_metrics(m):
    return {k: getattr(m, k) for k in METRIC_KEYS}


FRAME_GUARD = 3  # noise rows between the frames of a pitched buffer (gpu_inputs with a layout)


def gpu_inputs(gpu, W, H, N, F, seed, drop, layout=None):
    """The GPU-rendered frames (checked equal to the oracle's rendering), the
    per-frame detections with `drop` of them left out at random, and the
    oracle's sequence for oracle_run.  With `layout` (a name of
    tests/_views.py's LAYOUTS) the frames are windows of one noise-filled
    (F, H + guard, pitch) buffer instead: a common pitch larger than the row,
    the layout's base offset, guard rows between and around the frames."""
    from opencv_amd import klt, tbd

    frames, gt = klt.synth_render(seed, W, H, N, 0, F, ctx=gpu)
    seq = sequence(seed, W, H, N, F, drop)
    ofr, ogt, keep = seq
    assert np.array_equal(frames.cpu().numpy(), ofr) and np.array_equal(gt.numpy(), ogt)
    if layout is not None:
        import _views as V

        step = H + FRAME_GUARD
        tall = np.random.default_rng(seed).integers(0, 256, (F * step - FRAME_GUARD, W), dtype=np.uint8)
        for f in range(F):
            tall[f * step:f * step + H] = ofr[f]
        _, view = V.window(tall, layout, seed, device=frames.device)
        frames = [view[f * step:f * step + H] for f in range(F)]
        assert all(np.array_equal(frames[f].cpu().numpy(), ofr[f]) and frames[f].stride(0) > W for f in range(F))
    dets = []
    for f in range(F):
        d = tbd.detections_from_gt(ogt[f])
        dets.append(np.ascontiguousarray(d[keep[f][d["id"]]]))
    return frames, dets, seq


class ctx_options:
    """Context options on for a block (before any loop is created: several are
    read by tbdk_tbd_create), every known option back at its default after it."""

    def __init__(self, gpu, options):
        self.gpu, self.options = gpu, dict(options or {})

    def __enter__(self):
        for k in self.options:
            if k not in CTX_DEFAULTS:
                raise KeyError(f"context option {k}: default not listed in CTX_DEFAULTS")
        for k, v in self.options.items():
            self.gpu.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.options:
            self.gpu.set_option(k, CTX_DEFAULTS[k])
        return False


def run_pair(gpu, W, H, N, F, seed, drop=0.0, cfg=None, options=None, layout=None):
    """The GPU loop (step with next_frame, then a second loop through
    tbdk_tbd_run) against the oracle pipeline, every frame: metrics equal, the
    same tracks predicted with centres within PRED_TOL, every track row equal.
    Returns the oracle's activity and the worst prediction error.  layout: the
    frames as pitched windows (gpu_inputs)."""
    import torch
    from opencv_amd import tbd

    cfg = dict(cfg or {})
    frames, dets, seq = gpu_inputs(gpu, W, H, N, F, seed, drop, layout)
    ora = oracle_run(W, H, N, F, seed, drop, cfg, seq)
    stats = dict(activity(ora), pred_err=0.0)
    with ctx_options(gpu, options):
        c = tbd.default_config(W, H, **cfg)
        loop = tbd.TbdLoop(c, ctx=gpu)
        gms = []
        for f in range(F):
            m = loop.step(frames[f], f, dets[f], next_frame=frames[f + 1] if f + 1 < F else None)
            gm, om = gpu_metrics(m), ora.metrics[f]
            gms.append(gm)
            assert gm == om, f"frame {f}: metrics {gm} vs oracle {om}"
            gp, op = loop.predictions(), ora.preds[f]
            assert gp.keys() == op.keys(), f"frame {f}: predicted tracks differ"
            for k, (cx, cy) in gp.items():
                e = max(abs(cx - op[k][0]), abs(cy - op[k][1]))
                assert e <= PRED_TOL, f"frame {f} track {k}: centre {cx, cy} vs {op[k]}"
                stats["pred_err"] = max(stats["pred_err"], e)
            assert gpu_rows(loop.tracks()) == list(ora.rows[f]), f"frame {f}: tracks differ"
        # the native frame loop (tbdk_tbd_run) over the same frames: the same frames out
        batch = tbd.TbdLoop(c, ctx=gpu)
        ms = batch.run([frames[f] for f in range(F)], 0, dets)
        assert [gpu_metrics(m) for m in ms] == gms
        assert gpu_rows(batch.tracks()) == list(ora.rows[F - 1])
        torch.cuda.synchronize()
        del loop, batch
    return stats


# ---- the configuration matrix (tests/test_gpu_tbd_configs.py) ----------------

Case = namedtuple("Case", "id W H N F seed drop cfg options")


def _case(cid, cfg=None, options=None, W=320, H=240, N=12, F=12, drop=0.1, seed=31):
    full = {"bounds_xmax": W, "bounds_ymax": H}  # bounds: the frame
    full.update(cfg or {})
    return Case(cid, W, H, N, F, seed, drop, full, dict(options or {}))


_W9 = {"win": 9, "max_level": 3}  # the non-default window the launch-path options are crossed with

CASES = [
    _case("baseline"),
    # the generic LDS kernel (no lk_multi instance: window 3, 5, even)
    _case("win3", {"win": 3}),
    _case("win5", {"win": 5}),
    _case("win8", {"win": 8}),
    _case("win5_iters2_level0", {"win": 5, "lk_iters": 2, "max_level": 0}),
    # other lk_multi instances (points per wave) and pyramid depths
    _case("win7", {"win": 7}),
    _case("win9_level4", {"win": 9, "max_level": 4}),
    _case("win15_level3", {"win": 15, "max_level": 3}),
    _case("win31_level1", {"win": 31, "max_level": 1}),
    _case("win21_level0", {"win": 21, "max_level": 0}),
    # frame shapes: odd sizes, and frames too small for the requested depth
    _case("333x251_win9_level3", _W9, W=333, H=251),
    _case("333x251_win8", {"win": 8}, W=333, H=251),
    _case("160x120_win21_level3", {"win": 21, "max_level": 3}, W=160, H=120, N=6),
    _case("96x80_win21_level3", {"win": 21, "max_level": 3}, W=96, H=80, N=3, drop=0.0),  # stop rule: two levels
    _case("96x80_win31", {"win": 31}, W=96, H=80, N=3),
    # GFTT
    _case("corners17", {"max_corners": 17, "min_points": 8}),
    _case("min_distance0", {"min_distance": 0.0}),
    _case("min_distance10_quality0.2", {"min_distance": 10.0, "quality_level": 0.2}),
    # refresh rules
    _case("redetect1", {"redetect_every": 1}),
    _case("redetect3_min_points120", {"redetect_every": 3, "min_points": 120}),
    # PyrLK termination and gates
    _case("iters3", {"lk_iters": 3}),
    _case("iters1_eps0.5", {"lk_iters": 1, "lk_epsilon": 0.5}),
    _case("min_eig0.05", {"min_eig_threshold": 0.05}),
    _case("min_eig0.2_min_points200", {"min_eig_threshold": 0.2, "min_points": 200}),
    # fit gate
    _case("min_fit250", {"min_fit_points": 250}),
    # slot pool smaller than the track count
    _case("pool24_of_40", {"max_tracks": 24, "track_age_threshold": 2}, N=40),
    # kernel routing by context option
    _case("lk_impl2_win21", None, {"lk_impl": 2}),
    _case("strip_win21", None, {"lk_impl": 1, "tbd_pyr_derivs": 1}),
    _case("derivs_win9", {"win": 9}, {"tbd_pyr_derivs": 1}),
    _case("derivs_fly_win9", {"win": 9}, {"lk_scharr_fly": 1, "tbd_pyr_derivs": 1}),
    # launch-path options at a non-default window
    _case("w9_seg_list", _W9, {"lk_seg_inline": 0}),
    _case("w9_staged_tables", _W9, {"tbd_zero_copy": 0}),
    _case("w9_table_args", _W9, {"tbd_fit_inline": 0, "gftt_inline": 0}),
    _case("w9_gftt_full", _W9, {"gftt_compact": 0}),
    _case("w9_no_early_gftt", _W9, {"tbd_early_gftt": 0}),
]
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


def case_oracle(case):
    return oracle_run(case.W, case.H, case.N, case.F, case.seed, case.drop, case.cfg)


def check_oracle_activity(case):
    """A case must not pass by doing nothing: the conditions the oracle alone
    (never the GPU) must meet on the case's inputs.  Returns its activity."""
    run = case_oracle(case)
    a, m = activity(run), run.metrics
    assert a["preds"] > 0 and a["refreshed"] > 0 and a["lk_points"] > 0, (case.id, a)
    base = activity(case_oracle(BY_ID["baseline"]))
    cid = case.id
    if cid == "min_fit250":  # the fit gate holds predictions back
        assert a["preds"] < base["preds"], (a, base)
    elif cid == "min_eig0.2_min_points200":  # the eigenvalue gate drops most points, the sets are refreshed for it
        assert 2 * a["lost"] > a["lk_points"] and a["refreshed"] > base["refreshed"], (a, base)
    elif cid == "min_eig0.05":
        assert a["lost"] > base["lost"], (a, base)
    elif cid == "corners17":  # no set enters PyrLK with more than max_corners points
        assert all(m[f]["lk_points"] <= 17 * m[f - 1]["ntracks"] for f in range(1, case.F)), m
        assert a["lk_points"] <= 17 * max(x["ntracks"] for x in m) * case.F
    elif cid == "min_distance10_quality0.2":
        assert a["lk_points"] < base["lk_points"], (a, base)
    elif cid == "win3":
        assert a["lost"] > base["lost"], (a, base)
    elif cid == "pool24_of_40":  # pool exhausted: tracks left without a point set
        assert any(m[f]["ntracks"] > m[f]["klt_predicted"] and m[f - 1]["ntracks"] > 24 for f in range(1, case.F)), m
        assert max(run.slots) == 24 and all(x["klt_predicted"] <= 24 for x in m)
    elif cid == "redetect1":  # every frame refreshes every track's set
        assert a["refreshed"] >= sum(m[f]["ntracks"] for f in range(1, case.F)), (a, m)
    return a
