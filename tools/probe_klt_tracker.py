"""KLT point tracker timing probe on the benchmark's 1080p sequence: the
device-resident tracker (klt.KltTracker.step, nothing read back) against the same
per-frame work composed from the public Python calls with the host in the middle
of every frame (calc_checked, status and points to the host, compaction in numpy,
the mask drawn in numpy and uploaded, detect(mask=), append in numpy).

    python tools/probe_klt_tracker.py [--tag NAME] [--frames 20] [--blocks 6] [--out FILE]

A block is one pass over the sequence from an empty tracker; the two sides take
turns block by block within the run, after one unmeasured block each.  Per step,
separately for detection and non-detection frames, over all measured blocks
(median, and the 10th and 90th percentile):

    us_events   HIP events recorded on the stream before and after the step's work.
                For the tracker that is the enqueued device work; for the composed
                side it includes the time the device waits for the host.
    us_wall     host clock around the step with a stream synchronise at its end

and us_wall_pipelined for the tracker: a block's steps enqueued back to back, one
synchronise at the end, over the number of steps; and us_per_launch: after the
measured blocks, two more tracker blocks with the context's timing records on,
the mean time of a launch bracket by name (launches in brackets).  One JSON line
per parameter row and side; --out appends them to the JSON list in FILE
(profiles/klt_tracker_probe.json holds the rows of one run)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _klt_tracker_oracle as KO  # noqa: E402  (the circle's half widths, on the host)
from opencv_amd import klt  # noqa: E402

ROWS = [("lk_track", dict()), ("4000 corners at 0.01", dict(max_corners=4000, quality_level=0.01))]

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="")
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--out", default="")
args = ap.parse_args()

W, H = 1920, 1080
ctx = klt.Context.get(0)
frames, _ = klt.synth_render(20261015, W, H, 128, 0, args.frames, ctx=ctx)
torch.cuda.synchronize()


def emit(row):
    print(json.dumps(row), flush=True)
    if args.out:
        rows = json.load(open(args.out)) if os.path.exists(args.out) else []
        rows.append(row)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


class Composed:
    """lk_track's loop on the public calls, the host between them"""

    def __init__(self, cfg):
        self.c = cfg
        self.lk = klt.SparsePyrLKOpticalFlow((cfg.win, cfg.win), cfg.max_level, cfg.lk_iters, epsilon=cfg.lk_epsilon,
                                             minEigThreshold=cfg.min_eig_threshold)
        self.det = klt.GoodFeaturesToTrackDetector(cfg.max_corners, cfg.quality_level, cfg.min_distance,
                                                   cfg.block_size, bool(cfg.use_harris), cfg.harris_k)
        self.pyr = [klt.Pyramid(ctx, W, H, cfg.max_level, (cfg.win, cfg.win), derivs=False) for _ in range(2)]
        hw = KO.circle_half_widths(cfg.mask_radius)
        r = cfg.mask_radius
        self.stamp = np.abs(np.arange(-r, r + 1))[None, :] <= hw[np.abs(np.arange(-r, r + 1))][:, None]
        self.reset()

    def reset(self):
        L = self.c.track_len
        self.hist, self.lens = np.zeros((0, L, 2), np.float32), np.zeros(0, np.int64)
        self.ids, self.next_id, self.frame_idx, self.cur = np.zeros(0, np.int64), 0, 0, 0

    def last(self):
        return self.hist[np.arange(len(self.lens)), self.lens - 1]

    def step(self, frame):
        c, L, r = self.c, self.c.track_len, self.c.mask_radius
        P = self.pyr[self.cur].build(frame)
        if self.frame_idx > 0 and len(self.ids):
            res = self.lk.calc_checked(self.pyr[self.cur ^ 1], P, torch.from_numpy(self.last()).cuda(),
                                       back_threshold=c.back_threshold, want_err=False)
            keep = res.status.cpu().numpy() == 1
            nxt = res.next_pts.cpu().numpy()[keep]
            hist, lens = self.hist[keep], self.lens[keep]
            full = lens == L
            hist[full, :-1] = hist[full, 1:]
            lens = np.minimum(lens + 1, L)
            hist[np.arange(len(lens)), lens - 1] = nxt
            self.hist, self.lens, self.ids = hist, lens, self.ids[keep]
        if self.frame_idx % c.detect_interval == 0:
            mask = np.full((H + 4 * r, W + 4 * r), 255, np.uint8)  # 2r pixels of margin instead of clipping
            for x, y in self.last().astype(np.int32).tolist():
                if -r <= x < W + r and -r <= y < H + r:
                    mask[y + r:y + 3 * r + 1, x + r:x + 3 * r + 1][self.stamp] = 0
            m = torch.from_numpy(np.ascontiguousarray(mask[2 * r:2 * r + H, 2 * r:2 * r + W])).cuda()
            new = self.det.detect(frame, mask=m).cpu().numpy()
            new = new[:c.max_tracks - len(self.ids)]
            h = np.zeros((len(new), L, 2), np.float32)
            h[:, 0] = new
            self.hist = np.concatenate([self.hist, h])
            self.lens = np.concatenate([self.lens, np.ones(len(new), np.int64)])
            self.ids = np.concatenate([self.ids, self.next_id + np.arange(len(new))])
            self.next_id += len(new)
        self.frame_idx += 1
        self.cur ^= 1

    def count(self):
        return len(self.ids)


class Resident:
    def __init__(self, cfg):
        self.t = klt.KltTracker(cfg, ctx=ctx)

    def reset(self):
        self.t.reset()

    def step(self, frame):
        self.t.step(frame)

    def count(self):
        return len(self.t.read().ids)


def block(side, sync_each):
    """one pass over the sequence -> per step (event ms, wall s), the block's wall time"""
    side.reset()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.frames)]
    wall = []
    t_block = time.perf_counter()
    for f in range(args.frames):
        t0 = time.perf_counter()
        ev[f][0].record()
        side.step(frames[f])
        ev[f][1].record()
        if sync_each:
            torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    t_block = time.perf_counter() - t_block
    return [a.elapsed_time(b) * 1e3 for a, b in ev], [w * 1e6 for w in wall], t_block * 1e6 / args.frames


def pct(v):
    v = np.asarray(v, np.float64)
    return [round(float(np.percentile(v, q)), 1) for q in (50, 10, 90)] if len(v) else None


for name, over in ROWS:
    cfg = klt.KltTracker.default_config(W, H)
    for k, v in over.items():
        setattr(cfg, k, v)
    det = np.array([f % cfg.detect_interval == 0 for f in range(args.frames)])
    sides = {"tracker": Resident(cfg), "composed": Composed(cfg)}
    acc = {s: dict(ev=[], wall=[], pipe=[]) for s in sides}
    counts = {}
    for b in range(-1, args.blocks):  # block -1: unmeasured (code objects loaded, scratch grown)
        for s, side in sides.items():
            e, w, _ = block(side, True)
            counts[s] = side.count()
            p = block(side, False)[2] if s == "tracker" else None
            if b >= 0:
                acc[s]["ev"].append(e)
                acc[s]["wall"].append(w)
                if p is not None:
                    acc[s]["pipe"].append(p)
    names = ["pyr_build", "lk_sparse", "lk_sparse_back", "klt_compact", "klt_mask", "gftt", "gftt_wide", "klt_append"]
    ctx.timing_select(names)
    ctx.timing_enable(True)
    base = {k: ctx.timing_query(k) for k in names}
    for _ in range(2):
        block(sides["tracker"], True)
    per_launch = {k: tuple(a - b for a, b in zip(ctx.timing_query(k), base[k])) for k in names}
    ctx.timing_enable(False)
    ctx.timing_select(None)
    for s in sides:
        e, w = np.array(acc[s]["ev"]), np.array(acc[s]["wall"])
        row = {"tag": args.tag, "what": f"1080p, {name}", "side": s, "frames": args.frames, "blocks": args.blocks,
               "tracks_at_end": counts[s],
               "same_tracks_on_both_sides": counts["tracker"] == counts["composed"], "stat": "median, p10, p90 over blocks x frames",
               "us_events_detect": pct(e[:, det]), "us_events_track": pct(e[:, ~det]),
               "us_wall_detect": pct(w[:, det]), "us_wall_track": pct(w[:, ~det])}
        if acc[s]["pipe"]:
            row["us_wall_pipelined_per_step"] = pct(acc[s]["pipe"])
            row["us_per_launch"] = {k: [round(1e3 * ms / n, 1), n] for k, (n, ms) in per_launch.items() if n}
        emit(row)
