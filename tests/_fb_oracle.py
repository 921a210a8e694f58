"""The forward-backward checked PyrLK composed from the oracle's pieces: the
standalone call (checked_trace, the reference samples' checkedTrace with both
statuses gating) and the TBD loop with the check (FbKltTbdLoop), the references
of tests/test_gpu_lk_fb.py and tests/test_gpu_tbd_fb.py.  tests/test_fb_oracle.py
checks on the CPU that their inputs exercise every way a point can fail.

Semantics: forward (p1, st) = lk(A, B, p0); backward (p0r, stb) = lk(B, A,
p1[st == 1]) with the same window, levels, criteria and minEig threshold,
flags 0 and no error output; d = max(|p0.x - p0r.x|, |p0.y - p0r.y|) in
float32; kept iff st == 1, stb == 1 and d < thr."""
import math
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tbd_loop_oracle as L  # noqa: E402
import _loop_pair as LP  # noqa: E402

O = L.O

Checked = namedtuple("Checked", "next_pts status fwd_status err iters back_pts back_status fb_err")


def _win(win):
    return (int(win), int(win)) if np.isscalar(win) else (int(win[0]), int(win[1]))


def fb_distance(p0, p0r):
    """max(|dx|, |dy|) in float32"""
    p0, p0r = np.asarray(p0, np.float32), np.asarray(p0r, np.float32)
    return np.maximum(np.abs(p0[:, 0] - p0r[:, 0]), np.abs(p0[:, 1] - p0r[:, 1])).astype(np.float32)


def checked_trace(Pa, Pb, pts, win, max_level, iters, eps, min_eig, thr, accum, flags=0, init=None, want_err=True,
                  nthreads=8):
    """pts tracked Pa -> Pb and back.  flags / init / want_err are the forward
    pass's only.  Returns Checked: the forward pass's next_pts / err / iters and
    status (fwd_status), the checked status, the points tracked back (pts where
    the forward pass lost the point; back_status 0 there) and fb_err (d where
    both statuses are 1, +inf elsewhere)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    w = _win(win)
    nxt, st, err, it = O.lk(Pa, Pb, pts, w, max_level, iters, eps, flags, min_eig, accum, nthreads, init=init,
                            want_err=want_err)
    f = st == 1
    back, bst = pts.copy(), np.zeros(len(pts), np.uint8)
    fb = np.full(len(pts), np.inf, np.float32)
    if f.any():
        b, sb, _, _ = O.lk(Pb, Pa, nxt[f], w, max_level, iters, eps, 0, min_eig, accum, nthreads, want_err=False)
        back[f], bst[f] = b, sb
        d = fb_distance(pts[f], b)
        fb[f] = np.where(sb == 1, d, np.float32(np.inf))
    keep = f & (bst == 1) & (fb < np.float32(thr))
    return Checked(nxt, keep.astype(np.uint8), st, err, it, back, bst, fb)


def kinds(c):
    """(forward-lost, backward-lost, too-far, kept) counts of a Checked"""
    f, b = c.fwd_status == 1, c.back_status == 1
    return int((~f).sum()), int((f & ~b).sum()), int((f & b & (c.status == 0)).sum()), int(c.status.sum())


class FbKltTbdLoop(L.KltTbdLoop):
    """The KLT TBD loop with ctx option tbd_fb_check: every frame's PyrLK call is
    followed by the backward call over the points it tracked, and only the kept
    pairs stay in a track's set and enter its fit.  fb_log: per PyrLK frame the
    counts of forward-lost, backward-lost and too-far points and of kept pairs."""

    def __init__(self, width, height, fb_thr=1.0, **kw):
        super().__init__(width, height, **kw)
        self.fb_thr = np.float32(fb_thr)
        self.fb_log = []

    def _klt(self, P):
        ids = [t.id for t in self.tracker.tracks if t.id in self.slot]
        counts = [len(self.sets.get(i, ())) for i in ids]
        pts = np.concatenate([self.sets[i] for i in ids if len(self.sets.get(i, ()))]) if sum(counts) else \
            np.zeros((0, 2), np.float32)
        w = (self.win, self.win)
        nxt, st, _, _ = O.lk(self.prev, P, pts, w, self.ml, self.iters, self.eps, 0, self.min_eig, self.accum,
                             self.nthreads, want_err=False)
        f = st == 1
        bst = np.zeros(len(pts), np.uint8)
        far = np.zeros(len(pts), bool)
        if f.any():
            b, sb, _, _ = O.lk(P, self.prev, nxt[f], w, self.ml, self.iters, self.eps, 0, self.min_eig, self.accum,
                               self.nthreads, want_err=False)
            bst[f] = sb
            far[f] = ~(fb_distance(pts[f], b) < self.fb_thr)
        keep = f & (bst == 1) & ~far
        self.fb_log.append(dict(fwd_lost=int((~f).sum()), back_lost=int((f & (bst == 0)).sum()),
                                too_far=int((f & (bst == 1) & far).sum()), kept=int(keep.sum()), pairs=int(f.sum())))
        preds, off, tracked = {}, 0, 0
        boxes = {t.id: t.bboxes[-1] for t in self.tracker.tracks}
        for i, n in zip(ids, counts):
            ok = keep[off:off + n]
            a, b = pts[off:off + n][ok], nxt[off:off + n][ok]
            off += n
            self.sets[i] = b
            self.npts[i] = len(b)
            tracked += len(b)
            if len(b) < self.min_fit:
                continue
            M = L.BF.get_rt_matrix(a, b)
            bb = boxes[i]
            cx, cy = L.BF.propagate_box(M, (bb.x, bb.y, bb.width, bb.height))
            scale = math.hypot(M[0, 0], M[1, 0])
            if 0.5 < scale < 2.0 and math.isfinite(cx) and math.isfinite(cy):
                preds[i] = (cx, cy)
        return preds, int(sum(counts)), tracked


# ---- the inputs of the GPU tests ---------------------------------------------

# standalone call (tests/test_gpu_lk_fb.py): frames 0 and 3 of a 320x240 sequence
LK_SEQ = (20261022, 320, 240, 6, 0, 4)
LK_CASES = [(21, 2), (9, 2), (5, 1), (21, 0), (8, 2)]  # (window, max_level)
LK_THRS = (1.0, 0.25)
LK_ITERS, LK_EPS, LK_MIN_EIG = 30, 0.01, 1e-4
_lk = {}


def lk_inputs():
    """frames 0 and 3, and 616 points: GFTT corners of frame 0 plus 16 points
    1.5 px inside the top and bottom edges (no multiple of any points-per-wave)"""
    if "in" not in _lk:
        fr, _ = O.synth(*LK_SEQ)
        f0, f3 = np.ascontiguousarray(fr[0]), np.ascontiguousarray(fr[3])
        c = O.gftt(f0, 600, 0.01, 3.0)
        xs = np.linspace(10.0, 310.0, 8, dtype=np.float32)
        edge = np.array([(x, y) for y in (1.5, 240 - 2.5) for x in xs], np.float32)
        _lk["in"] = (f0, f3, np.ascontiguousarray(np.concatenate([c, edge]), np.float32))
    return _lk["in"]


def lk_pyramids(win, max_level):
    key = ("pyr", win, max_level)
    if key not in _lk:
        f0, f3, _ = lk_inputs()
        _lk[key] = (O.Pyramid(f0, (win, win), max_level), O.Pyramid(f3, (win, win), max_level))
    return _lk[key]


def lk_reference(win, max_level, thr):
    """checked_trace of the standalone inputs in ACCUM_EXACT, computed once"""
    key = ("ref", win, max_level, thr)
    if key not in _lk:
        Pa, Pb = lk_pyramids(win, max_level)
        _lk[key] = checked_trace(Pa, Pb, lk_inputs()[2], win, max_level, LK_ITERS, LK_EPS, LK_MIN_EIG, thr,
                                 O.ACCUM_EXACT)
    return _lk[key]


# the loop (tests/test_gpu_tbd_fb.py): 640x480, 16 objects, 8 frames
TW, TH, TN, TF = 640, 480, 16, 8
LoopCase = namedtuple("LoopCase", "id seed opt cfg options ransac via_run")


def _lc(cid, seed=20261022, opt=1024, cfg=None, options=None, ransac=0, via_run=False):
    return LoopCase(cid, seed, opt, dict(cfg or {}), dict(options or {}), ransac, via_run)


LOOP_CASES = [
    _lc("default_1px"),
    _lc("seed23_quarter_px", seed=20261023, opt=256),
    _lc("win5_level1", cfg={"win": 5, "max_level": 1}),  # the generic kernel
    _lc("win9", cfg={"win": 9}),
    _lc("lk_impl2", options={"lk_impl": 2}),
    _lc("pyr_derivs", options={"tbd_pyr_derivs": 1}),
    _lc("no_spec_lookahead", options={"tbd_spec_lookahead": 0}),
    _lc("early_la2", options={"tbd_early_la": 2}),
    _lc("borrow_l0_run", options={"tbd_borrow_l0": 1}, via_run=True),
    _lc("max_tracks10", cfg={"max_tracks": 10}),
    _lc("level0", cfg={"max_level": 0}),
    _lc("ransac500", ransac=500),
]
LOOP_BY_ID = {c.id: c for c in LOOP_CASES}

FbRun = namedtuple("FbRun", "metrics preds rows log")
_runs = {}


def loop_sequence(seed):
    key = ("seq", seed)
    if key not in _runs:
        _runs[key] = L.O.synth(seed, TW, TH, TN, 0, TF)
    return _runs[key]


def loop_oracle(seed, opt, cfg, ransac=0):
    """The oracle loop over the sequence, once per (seed, option, overrides):
    opt 0 is the plain KltTbdLoop, else FbKltTbdLoop at opt / 1024 px; ransac > 0
    replaces the fit module by tests/test_gpu_tbd_ransac.py's shim for the run."""
    key = (seed, opt, tuple(sorted(cfg.items())), ransac)
    if key in _runs:
        return _runs[key]
    ofr, ogt = loop_sequence(seed)
    kw = dict(nthreads=min(16, os.cpu_count() or 1), **LP.oracle_kwargs(cfg))
    saved = L.BF
    if ransac:
        import test_gpu_tbd_ransac as TR

        assert ransac == 500  # the shim's rounds
        L.BF = TR.RansacFitShim
    try:
        ora = FbKltTbdLoop(TW, TH, fb_thr=opt / 1024.0, **kw) if opt else L.KltTbdLoop(TW, TH, **kw)
        ms, ps, rs = [], [], []
        for f in range(TF):
            ms.append(dict(ora.step(ofr[f], f, L.detections(ogt[f], f, None))))
            ps.append(dict(ora.preds))
            rs.append(tuple(ora.track_rows()))
    finally:
        L.BF = saved
    _runs[key] = FbRun(tuple(ms), tuple(ps), tuple(rs), tuple(getattr(ora, "fb_log", ())))
    return _runs[key]


def largest_change(a, b):
    """largest centre difference between two runs' predictions of the same track-frames"""
    return max((max(abs(p[k][0] - q[k][0]), abs(p[k][1] - q[k][1]))
                for p, q in zip(a.preds, b.preds) for k in p.keys() & q.keys()), default=0.0)
