#!/usr/bin/env python3
"""Per-launch time of tbdk_estimate_affine_2d: both models under RANSAC and
LMEDS on 200 and 1000 pairs at 30, 60 and 85 % outliers
(tests/_affine2d_cases.py generators), 1, 64 and 128 sets per launch, and the
TBD loop's own shape of 128 sets x 256 pairs, each with the 10-iteration LM step
and without it; for context, tbdk_find_homography and
tbdk_box_propagate_ransac on the same sets; then tbdk_warp_affine_u8_dev beside
tbdk_warp_affine_u8 at 640x480.  Times are the library's per-kernel HIP events
(tbdk_timing_*), over `--reps` launches after `--warmup`; the median of
`--rounds` rounds with the range.

    python tools/probe_affine2d.py [--out profiles/affine2d_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _affine2d_cases as AC  # noqa: E402
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
    t = (args.reps, args.warmup, args.rounds)

    def emit(row, timing):
        row.update(reps=args.reps, rounds=args.rounds, **timing)
        rows.append(row)
        print(json.dumps(row), flush=True)

    shapes = [(n, out, sets) for n in (200, 1000) for out in (30, 60, 85) for sets in (1, 64, 128)] + [(256, 30, 128)]
    for n, out, nsets in shapes:
        src, dst = AC.points("plane", n, out, "similarity", 4242 + n + out)
        ds, dd = (torch.from_numpy(np.tile(a, (nsets, 1))).cuda() for a in (src, dst))
        offs = (torch.arange(nsets + 1, dtype=torch.int32) * n).cuda()
        name = f"{n} pairs, {out} % outliers"
        for model, fn_est in ((AC.FULL, klt.estimate_affine_2d), (AC.PARTIAL, klt.estimate_affine_partial_2d)):
            for method in (AC.RANSAC, AC.LMEDS):
                for refine in (10, 0):
                    r = []

                    def fn():
                        r[:] = [fn_est(ds, dd, method, 3.0, 2000, 0.99, refine, offsets=offs, ctx=ctx)]

                    row = {"input": name, "sets": nsets, "kernel": "estimate_affine2d",
                           "model": AC.MODEL_NAME[model], "method": "RANSAC" if method == AC.RANSAC else "LMEDS",
                           "refine_iters": refine}
                    timing = timed(ctx, "estimate_affine2d", fn, *t)
                    row["iters"], row["ninliers"] = int(r[0].iters[0]), int(r[0].ninliers[0])
                    emit(row, timing)
        # context: the two fits the library already has, on the same sets
        timing = timed(ctx, "find_homography",
                       lambda: klt.find_homography(ds, dd, klt.RANSAC, 3.0, 2000, 0.995, offsets=offs, ctx=ctx), *t)
        emit({"input": name, "sets": nsets, "kernel": "find_homography"}, timing)
        if n <= 1024:  # its cap
            boxes = torch.tensor([[0, 0, AC.W, AC.H]] * nsets, dtype=torch.int32).cuda()
            timing = timed(ctx, "box_propagate_ransac",
                           lambda: klt.box_propagate_ransac(ds, dd, None, offs, boxes, ctx=ctx), *t)
            emit({"input": name, "sets": nsets, "kernel": "box_propagate_ransac"}, timing)
    # the warp by a device matrix beside the warp by a host matrix
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (480, 640), dtype=np.uint8)).cuda()
    dst = torch.empty_like(img)
    M = AC.TRUTHS["shear"]
    Md = torch.from_numpy(M.reshape(6).copy()).cuda()
    for kern, m in (("warp_affine_dev", Md), ("warp_affine", M)):
        timing = timed(ctx, kern, lambda: klt.warp_affine(img, m, (640, 480), dst=dst, ctx=ctx), *t)
        emit({"input": "640x480 8UC1 LINEAR", "kernel": kern}, timing)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
