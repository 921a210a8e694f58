"""The KLT point tracker (samples/python/lk_track.py App.run:48-86 minus the
drawing; lkdemo.cpp's cornerSubPix and click-to-add) composed from the oracle's
pieces, the reference of tests/test_gpu_klt_tracker.py:

  pyramid      O.Pyramid
  tracking     _fb_oracle.checked_trace(..., accum=O.ACCUM_EXACT, want_err=False):
               both statuses gate and d < back_threshold in float32 (lk_track
               ignores the statuses; the tracker keeps tbdk_lk_sparse_fb's)
  detection    _gftt_mask_oracle.gftt_masked on the whole frame under the disc mask
  refinement   _subpix_oracle.corner_sub_pix, criteria (COUNT|EPS, 20, 0.03)
  the discs    circle_half_widths / draw_discs below: cv::circle(img, c, r, 0, -1)
               restated (imgproc/src/drawing.cpp:1486-1628, Circle() with fill),
               pinned to the real function by tests/golden/reference_circle.npz

Nothing of the GPU's output feeds it."""
from collections import namedtuple

import numpy as np

import _fb_oracle as FB
import _gftt_mask_oracle as GM
import _subpix_oracle as SP

O = FB.O


def circle_half_widths(radius):
    """Per |dy| = 0..radius the half width of the filled circle's row: Circle()'s
    midpoint walk draws, per iteration, rows cy -+ dy with half width dx and rows
    cy -+ dx with half width dy; a row's span is the widest it was given."""
    hw = np.full(radius + 1, -1, np.int64)
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1  # 0 or -1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    assert (hw >= 0).all()
    return hw


def trunc_centres(pts):
    """(int)x, (int)y as np.int32 casts them (toward zero)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(pts, np.float32).reshape(-1, 2).astype(np.int32)


def draw_discs(mask, pts, radius, value=0):
    """cv::circle(mask, (int(x), int(y)), radius, value, -1) for every point, in
    place, clipped to the mask; every disc writes the same value, so their order
    does not matter"""
    h, w = mask.shape
    hw = circle_half_widths(radius)
    for cx, cy in trunc_centres(pts).astype(np.int64).tolist():
        for dy in range(-radius, radius + 1):
            y = cy + dy
            if 0 <= y < h:
                x0, x1 = max(cx - hw[abs(dy)], 0), min(cx + hw[abs(dy)], w - 1)
                if x0 <= x1:
                    mask[y, x0:x1 + 1] = value
    return mask


# tests/golden/reference_circle.npz (tools/record_reference_cases.py): cv::circle(img, c, r, 0, -1) on a
# 255-filled CIRCLE_SIZE image, one case per (cx, cy, r), stored bit-packed (1 = drawn)
CIRCLE_SIZE = (48, 40)  # width, height
CIRCLE_CASES = [(24, 20, r) for r in range(17)] + \
    [(cx, cy, r) for r in (5, 9) for cx, cy in ((-3, 2), (0, 0), (47, 39), (53, 20), (20, -6), (-9, -9), (24, 45))]


DEFAULTS = dict(win=15, max_level=2, lk_iters=10, lk_epsilon=0.03, min_eig_threshold=1e-4, back_threshold=1.0,
                max_corners=500, quality_level=0.3, min_distance=7.0, block_size=7, use_harris=0, harris_k=0.04,
                detect_interval=5, track_len=10, mask_radius=5, subpix_win=0, max_tracks=8192)

Stats = namedtuple("Stats", "tracks_in kept detected appended dropped next_id frame_idx")


class KltTracker:
    """State: ids (list of int), hist (list of (len, 2) float32 arrays, oldest
    first, len <= track_len); the last point of track i is hist[i][-1]."""

    def __init__(self, width, height, **cfg):
        unknown = set(cfg) - set(DEFAULTS)
        assert not unknown, unknown
        self.w, self.h = int(width), int(height)
        self.cfg = dict(DEFAULTS, **cfg)
        self.log = []  # per tracked frame: FB.kinds of the check
        self.det_log = []  # per detection: (frame_idx, corners returned, live points whose disc is clipped)
        self.reset()

    def reset(self):
        self.ids, self.hist = [], []
        self.next_id = 0
        self.frame_idx = 0
        self.prev = None
        self.stats = Stats(0, 0, 0, 0, 0, 0, -1)
        self.last_mask = None

    def last_points(self):
        return np.array([h[-1] for h in self.hist], np.float32).reshape(-1, 2)

    def _append(self, pts, detected):
        c = self.cfg
        pts = np.asarray(pts, np.float32).reshape(-1, 2)
        take = min(len(pts), c["max_tracks"] - len(self.ids))
        for p in pts[:take]:
            self.ids.append(self.next_id)
            self.hist.append(p.reshape(1, 2).copy())
            self.next_id += 1
        s = self.stats
        self.stats = s._replace(detected=s.detected + (len(pts) if detected else 0), appended=s.appended + take,
                                dropped=s.dropped + len(pts) - take, next_id=self.next_id)

    def add_points(self, pts):
        self._append(pts, detected=False)

    def mask(self):
        """the detection mask of the live tracks (None without one)"""
        r = self.cfg["mask_radius"]
        if r < 0:
            return None
        return draw_discs(np.full((self.h, self.w), 255, np.uint8), self.last_points(), r)

    def step(self, frame, detect_now=False):
        c = self.cfg
        frame = np.ascontiguousarray(frame, np.uint8)
        assert frame.shape == (self.h, self.w)
        P = O.Pyramid(frame, (c["win"], c["win"]), c["max_level"])
        n_in = len(self.ids)
        self.last_mask = None
        if self.prev is not None and n_in:
            r = FB.checked_trace(self.prev, P, self.last_points(), c["win"], c["max_level"], c["lk_iters"],
                                 c["lk_epsilon"], c["min_eig_threshold"], c["back_threshold"], O.ACCUM_EXACT,
                                 want_err=False)
            self.log.append(FB.kinds(r))
            ids, hist = [], []
            for i in np.flatnonzero(r.status == 1):
                ids.append(self.ids[i])
                hist.append(np.concatenate([self.hist[i], r.next_pts[i].reshape(1, 2)])[-c["track_len"]:])
            self.ids, self.hist = ids, hist
        self.stats = Stats(n_in, len(self.ids), 0, 0, 0, self.next_id, self.frame_idx)
        if self.frame_idx % c["detect_interval"] == 0 or detect_now:
            m = self.mask()
            self.last_mask = m
            found = GM.gftt_masked(frame, m, c["max_corners"], c["quality_level"], c["min_distance"], c["block_size"],
                                   bool(c["use_harris"]), c["harris_k"])
            if c["subpix_win"] > 0 and len(found):
                found = SP.refine_rows(frame, found[None], None, (c["subpix_win"], c["subpix_win"]))[0]
            r = c["mask_radius"]
            lp = trunc_centres(self.last_points())
            clipped = int(((lp[:, 0] < r) | (lp[:, 1] < r) | (lp[:, 0] >= self.w - r) | (lp[:, 1] >= self.h - r)).sum()) \
                if r >= 0 and len(lp) else 0
            self.det_log.append((self.frame_idx, len(found), clipped))
            self._append(found, detected=True)
        self.frame_idx += 1
        self.prev = P
        return self.stats

    def state(self):
        """(ids int32 (n,), last float32 (n, 2), lens int32 (n,), hist float32 (n, track_len, 2) zero beyond len)"""
        L = self.cfg["track_len"]
        n = len(self.ids)
        hist = np.zeros((n, L, 2), np.float32)
        for i, h in enumerate(self.hist):
            hist[i, :len(h)] = h
        return (np.array(self.ids, np.int32), self.last_points(), np.array([len(h) for h in self.hist], np.int32), hist)


# ---- the cases of the GPU tests -----------------------------------------------

Case = namedtuple("Case", "id seq nframes cfg")
CASES = {
    "lk_track": Case("lk_track", (31, 320, 240, 12, 0, 13), 13, {}),
    "small": Case("small", (31, 320, 240, 12, 0, 13), 9,
                  dict(win=9, max_level=3, lk_iters=30, lk_epsilon=0.01, max_corners=60, quality_level=0.05,
                       min_distance=3.0, block_size=3, track_len=3, detect_interval=2, mask_radius=3)),
    "cap": Case("cap", (31, 333, 251, 12, 0, 7), 7,
                dict(win=21, max_corners=100, quality_level=0.01, min_distance=4.0, block_size=3, track_len=4,
                     detect_interval=2, mask_radius=4, max_tracks=150)),
}
_cache = {}


def frames(seq):
    if ("seq",) + tuple(seq) not in _cache:
        fr, _ = O.synth(*seq)
        _cache[("seq",) + tuple(seq)] = np.ascontiguousarray(fr)
    return _cache[("seq",) + tuple(seq)]


Run = namedtuple("Run", "states stats log det_log masks")


def run_case(case, **override):
    """The oracle over a case, once per (case, overrides): per frame the state
    after the step and its stats; left unchanged by the tests that share it."""
    key = (case.id, tuple(sorted(override.items())))
    if key not in _cache:
        fr = frames(case.seq)
        t = KltTracker(fr.shape[2], fr.shape[1], **dict(case.cfg, **override))
        states, stats, masks = [], [], []
        for f in range(case.nframes):
            stats.append(t.step(fr[f]))
            states.append(t.state())
            masks.append(t.last_mask)
        _cache[key] = Run(tuple(states), tuple(stats), tuple(t.log), tuple(t.det_log), tuple(masks))
    return _cache[key]
