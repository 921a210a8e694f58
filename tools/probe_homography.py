#!/usr/bin/env python3
"""Per-launch time of tbdk_find_homography: one set and 64 sets per launch of the
case table's shapes (tests/_homography_cases.py generators): 200 and 1000 pairs at
30 % outliers (the loop stops inside the first batch of 64 iterations), 200 pairs
at 60 % (about 200 iterations) and at 85 % with threshold 1 (all max_iters
iterations), method 0 on 1000 pairs, each with and without the LM step; then
tbdk_warp_perspective_dev beside tbdk_warp_perspective at 640x480 8UC1.  Times are
the library's per-kernel HIP events (tbdk_timing_*), over `--reps` launches after
`--warmup`; the median of `--rounds` rounds with the range.

    python tools/probe_homography.py [--out profiles/homography_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _homography_cases as HC  # noqa: E402
from opencv_amd import klt  # noqa: E402


def timed(ctx, kern, fn, reps, warmup, rounds):
    us = []
    for _ in range(rounds):
        ctx.timing_enable(False)
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ctx.timing_enable(True)
        ctx.timing_select([kern])
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        n, ms = ctx.timing_query(kern)
        ctx.timing_enable(False)
        us.append(1e3 * ms / max(n, 1))
    return {"us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    rows = []
    shapes = (("200 pairs, 30 % outliers", 200, 30, 3.0, 2000, HC.RANSAC), ("1000 pairs, 30 % outliers", 1000, 30, 3.0, 2000, HC.RANSAC),
              ("200 pairs, 60 % outliers", 200, 60, 3.0, 2000, HC.RANSAC),
              ("200 pairs, 85 % outliers, threshold 1, 300 iterations", 200, 85, 1.0, 300, HC.RANSAC),
              ("200 pairs, 85 % outliers, threshold 1, 2000 iterations", 200, 85, 1.0, 2000, HC.RANSAC),
              ("method 0, 1000 pairs", 1000, 0, 3.0, 2000, HC.LSQ))
    for name, n, out, thr, iters, method in shapes:
        src, dst = HC.points("plane", n, out, "mild", 4242 + n + out)
        for nsets in (1, 64):
            ds, dd = (torch.from_numpy(np.tile(a, (nsets, 1))).cuda() for a in (src, dst))
            offs = (torch.arange(nsets + 1, dtype=torch.int32) * n).cuda()
            for refine in (True, False):
                r = []

                def fn():
                    r[:] = [klt.find_homography(ds, dd, method, thr, iters, 0.995, offsets=offs, refine=refine, ctx=ctx)]

                row = {"input": name, "sets": nsets, "refine": refine, "reps": args.reps, "rounds": args.rounds}
                row.update(timed(ctx, "find_homography", fn, args.reps, args.warmup, args.rounds))
                row["iters"], row["ninliers"] = int(r[0].iters[0]), int(r[0].ninliers[0])
                rows.append(row)
                print(json.dumps(row), flush=True)
    # the warp by a device matrix beside the warp by a host matrix
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (480, 640), dtype=np.uint8)).cuda()
    dst = torch.empty_like(img)
    M = HC.TRUTHS["mild"]
    Md = torch.from_numpy(M.reshape(9).copy()).cuda()
    for kern, m in (("warp_perspective_dev", Md), ("warp_perspective", M)):
        row = {"input": "640x480 8UC1 LINEAR", "kernel": kern, "reps": args.reps, "rounds": args.rounds}
        row.update(timed(ctx, kern, lambda: klt.warp_perspective(img, m, (640, 480), dst=dst, ctx=ctx), args.reps,
                         args.warmup, args.rounds))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
