#!/usr/bin/env python3
"""What tbdk_corner_sub_pix costs, beside the GFTT launch it follows.

1080p synth_render frame, 128 ROIs (a 16 x 8 grid of 120 x 135 tiles), GFTT
(256, 0.01, 3.0): 128 rows x 256 corners with their device counts, refined with
lkdemo's criteria (COUNT|EPS, 20, 0.03) at window 5 and window 10.  Times are the
library's per-kernel HIP events ("gftt", "corner_sub_pix"), `--calls` launches
each; run the script under a kernel trace (in a run of its own) to confirm them.
`--iters` adds the mean iterations per point, counted by the numpy restatement
of tests/_subpix_oracle.py on the same corners (CPU, a few minutes).

    python tools/probe_subpix.py [--calls 20] [--iters] [--out profiles/subpix_probe.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SEED, NOBJ = 1920, 1080, 20261015, 128
ROIS = [(x * 120, y * 135, 120, 135) for y in range(8) for x in range(16)]
GFTT = (256, 0.01, 3.0)
CRITERIA = (3, 20, 0.03)


def mean_iters(frame, corners, counts, win):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    import _subpix_oracle as SO

    it = []
    for r in range(len(counts)):
        info = {}
        if counts[r] > 0:
            SO.corner_sub_pix(frame, corners[r, :counts[r]], (win, win), (-1, -1), CRITERIA, info)
            it.append(info["iters"])
    return float(np.concatenate(it).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iters", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from opencv_amd import klt

    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    frames, _ = klt.synth_render(SEED, W, H, NOBJ, 0, 1, ctx=ctx)
    frame = frames[0]
    det = klt.GoodFeaturesToTrackDetector(*GFTT)
    corners, counts = det.detect_rois(frame, ROIS)
    torch.cuda.synchronize()
    n = counts.cpu().numpy()
    row = {"width": W, "height": H, "rows": len(ROIS), "row_cap": GFTT[0], "points": int(n.clip(0).sum()),
           "criteria": CRITERIA, "calls": args.calls}
    ctx.timing_enable(True)
    ctx.timing_select(["gftt", "corner_sub_pix"])
    for _ in range(args.calls):
        det.detect_rois(frame, ROIS)
    torch.cuda.synchronize()
    cnt, ms = ctx.timing_query("gftt")
    row["gftt_us"] = round(1e3 * ms / max(cnt, 1), 2)
    for win in (5, 10):
        ctx.timing_enable(True)
        for _ in range(args.calls):
            klt.corner_sub_pix(frame, corners, (win, win), (-1, -1), CRITERIA, counts=counts, ctx=ctx)
        torch.cuda.synchronize()
        cnt, ms = ctx.timing_query("corner_sub_pix")
        assert cnt == args.calls
        row[f"corner_sub_pix_win{win}_us"] = round(1e3 * ms / cnt, 2)
        if args.iters:
            row[f"mean_iters_win{win}"] = round(mean_iters(frame.cpu().numpy(), corners.cpu().numpy(), n, win), 2)
    ctx.timing_enable(False)
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
