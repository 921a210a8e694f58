#!/usr/bin/env python3
"""Per-call device time of the 3x3 MORPH_OPEN and of connected_components_with_stats on 1080p MOG2-like masks
(klt.synth_render's moving objects over a static background, thresholded so that about 2 %, 20 % and 50 % of the
pixels are foreground), after `--warmup` calls: the library's HIP events around each call's launches
(tbdk_timing_*, labels "morph" and "cc"), the median over `--reps` calls; the component count and the compulsory
bytes of every connected-components phase at that size, with their time at 8 TB/s (a floor to read the numbers
against, not a bar).

    python tools/probe_blobs.py [--out profiles/blobs_probe.json]

The time of each phase comes from a kernel trace of its own (tracing slows the host, so never together with the
events above): run

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cc -- python tools/probe_blobs.py --phases D

which only repeats the connected-components call at foreground share D, and read DIR's kernel stats."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_amd import imgproc, klt  # noqa: E402

W, H = 1920, 1080
SHARES = (0.02, 0.2, 0.5)
CAP = 65536


def masks(ctx):
    """share -> 0 / 255 mask with about that share of foreground: the frame's brightest pixels"""
    frame = klt.synth_render(20261015, W, H, 128, 0, 1, ctx=ctx)[0][0]
    hist = torch.bincount(frame.reshape(-1).to(torch.int64), minlength=256).cpu().numpy()
    above = np.cumsum(hist[::-1])[::-1] / float(W * H)  # share of pixels >= level
    out = {}
    for s in SHARES:
        level = int(np.argmin(np.abs(above - s)))
        out[s] = ((frame >= level) * 255).to(torch.uint8).contiguous()
    return out


def events_us(ctx, kern, fn, reps):
    us = []
    for _ in range(reps):
        ctx.timing_enable(True)
        ctx.timing_select([kern])
        fn()
        torch.cuda.synchronize()
        n, ms = ctx.timing_query(kern)
        ctx.timing_enable(False)
        assert n == 1, (kern, n)
        us.append(1e3 * ms)
    return {"us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def phase_bytes(px, grana, cap_rows):
    """compulsory bytes per phase: what each kernel must read and write once (parents, keys and ranks are int32)"""
    keys = px // 4 if grana else px
    b = {"init": px + 4 * px + 4 * keys + (4 * px if grana else 0) + 40 * CAP,
         "merge": 3 * px,                      # the image and the row above; parents only where runs meet
         "compress": px + 8 * px,              # parent read and written
         "reduce": 4 * keys, "scan_tiles": 8 * (keys // 1024), "scan": 8 * keys,
         "relabel": 4 * px + 4 * px,           # parent read, label written (ranks at the roots only)
         "finish": 40 * cap_rows + 36 * cap_rows}
    if grana:
        b["flag"] = 4 * px
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--phases", type=float, default=None, help="only repeat the cc call at this foreground share")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    ms = masks(ctx)
    labels = torch.empty((H, W), dtype=torch.int32, device="cuda")
    stats = torch.zeros((CAP, 5), dtype=torch.int32, device="cuda")
    cent = torch.zeros((CAP, 2), dtype=torch.float64, device="cuda")
    kernel = imgproc.get_structuring_element(imgproc.MORPH_RECT, (3, 3))
    opened = torch.empty((H, W), dtype=torch.uint8, device="cuda")

    def cc(m, conn=8, t=imgproc.CCL_DEFAULT):
        return imgproc.connected_components_with_stats(m, labels, stats, cent, conn, t, CAP, ctx=ctx)

    if args.phases is not None:
        m = ms[min(SHARES, key=lambda s: abs(s - args.phases))]
        for _ in range(args.warmup + args.reps):
            cc(m)
        torch.cuda.synchronize()
        return
    rows = []
    for share, m in ms.items():
        for _ in range(args.warmup):
            imgproc.morphology_ex(m, imgproc.MORPH_OPEN, kernel, opened, ctx=ctx)
            cc(m)
            cc(m, 4, imgproc.CCL_WU)
        torch.cuda.synchronize()
        row = {"shape": f"{W}x{H}", "foreground_share": round(float((m != 0).float().mean()), 4),
               "n_labels": int(cc(m)[0].item()), "n_labels_4": int(cc(m, 4, imgproc.CCL_WU)[0].item()),
               "reps": args.reps, "warmup": args.warmup,
               "morph_open_3x3": events_us(ctx, "morph", lambda: imgproc.morphology_ex(m, imgproc.MORPH_OPEN, kernel,
                                                                                       opened, ctx=ctx), args.reps),
               "morph_compulsory_bytes": 4 * 2 * W * H,  # four passes, each reads and writes the image
               "cc_8_grana": events_us(ctx, "cc", lambda: cc(m), args.reps),
               "cc_4_wu": events_us(ctx, "cc", lambda: cc(m, 4, imgproc.CCL_WU), args.reps)}
        for name, grana in (("cc_8_grana", True), ("cc_4_wu", False)):
            b = phase_bytes(W * H, grana, min(CAP, row["n_labels"]))
            row[name + "_phase_bytes"] = b
            row[name + "_floor_us_at_8TBps"] = round(sum(b.values()) / 8e6, 2)
        row["morph_floor_us_at_8TBps"] = round(row["morph_compulsory_bytes"] / 8e6, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
