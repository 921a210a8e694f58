#!/usr/bin/env python3
"""Per-launch time of tbdk_box_propagate_ransac next to tbdk_box_propagate on the
same inputs: 128 boxes x 256 points, (a) clean similarity sets, (b) 40 % of the
pairs moved by up to +-40 px, (c) sets without consensus (every pair moved) at
max_iters 500 and 64.  Times are the library's per-kernel HIP events
(tbdk_timing_*), over `--reps` launches after `--warmup`.

    python tools/probe_box_ransac.py [--out profiles/box_ransac_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_amd import _lib, klt  # noqa: E402


def make(rng, nboxes, npts, frac, shift=40.0):
    prev, nxt, boxes = [], [], []
    for _ in range(nboxes):
        x, y = rng.uniform(0, 1700), rng.uniform(0, 900)
        w, h = int(rng.integers(60, 220)), int(rng.integers(60, 220))
        a = np.stack([rng.uniform(x, x + w, npts), rng.uniform(y, y + h, npts)], 1)
        ang, s = rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.1)
        R = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        b = a @ R.T + rng.uniform(-8, 8, 2) + rng.normal(0, 0.3, (npts, 2))
        out = rng.random(npts) < frac
        b[out] += rng.uniform(-shift, shift, (int(out.sum()), 2))
        prev.append(a)
        nxt.append(b)
        boxes.append((int(x), int(y), w, h))
    return (np.concatenate(prev).astype(np.float32), np.concatenate(nxt).astype(np.float32),
            np.asarray(boxes, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=128)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    rng = np.random.default_rng(20261019)
    nb, npts = args.boxes, args.points
    offs = torch.arange(0, (nb + 1) * npts, npts, dtype=torch.int32).cuda()
    out = torch.zeros(nb * klt.BOX_FIT_DTYPE.itemsize, dtype=torch.uint8).cuda()
    iters = torch.zeros(nb, dtype=torch.int32).cuda()
    inl = torch.zeros(nb * npts, dtype=torch.uint8).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for name, frac, max_iters in (("clean", 0.0, 500), ("outliers_40pct", 0.4, 500), ("no_consensus", 1.0, 500),
                                  ("no_consensus", 1.0, 64)):
        a, b, boxes = make(rng, nb, npts, frac)
        da, db, dbx = (torch.from_numpy(v).cuda() for v in (a, b, boxes))
        par = _lib.RansacParams(max_iters, 0.5)

        def ransac():
            _lib.check(ctx.lib.tbdk_box_propagate_ransac(ctx.handle, p(da), p(db), None, p(offs), p(dbx), nb, 4,
                                                         C.byref(par), p(out), p(iters), p(inl), None), "ransac")

        def lsq():
            _lib.check(ctx.lib.tbdk_box_propagate(ctx.handle, p(da), p(db), None, p(offs), p(dbx), nb, 4, p(out),
                                                  None), "lsq")

        row = {"input": name, "boxes": nb, "points_per_box": npts, "max_iters": max_iters, "reps": args.reps}
        for kern, fn in (("box_propagate_ransac", ransac), ("box_propagate", lsq)):
            ctx.timing_enable(False)
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ctx.timing_enable(True)
            ctx.timing_select([kern])
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            n, ms = ctx.timing_query(kern)
            ctx.timing_enable(False)
            row[kern + "_us"] = round(1e3 * ms / max(n, 1), 2)
            row[kern + "_timed"] = n
        it = iters.cpu().numpy()
        row["boxes_with_consensus"] = int((it >= 0).sum())
        row["mean_round"] = float(it[it >= 0].mean()) if (it >= 0).any() else None
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
