"""Whole-frame GFTT timing probe on the benchmark's 1080p frame: per parameter row
the mean device time of the eigenvalue stage plus LDS select (the context's "gftt"
timing record) and of the wide selection (gather, partition, walk: "gftt_wide"), from HIP
events around the launches, in blocks of launches; and, with --boxes, the existing
128-box launch pair ("gftt") alone, which a build without the wide path runs too,
so the two builds can be measured alternately.

    python tools/probe_gftt_frame.py [--tag NAME] [--blocks 5] [--launches 20] [--boxes] [--cpu] [--out FILE]

One JSON line per row.  --cpu adds the single-thread time of the CPU oracle
(oracle/gftt_oracle.c, the reference's algorithm restated) on the same call.
--out appends the rows to the JSON list in FILE (profiles/gftt_frame_probe.json
is the rows of one such sequence of runs, nothing else)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from opencv_amd import klt  # noqa: E402

ROWS = [(1000, 0.01, 0.0), (8000, 0.01, 0.0), (4000, 0.01, 10.0), (100000, 0.001, 0.0)]

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="")
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--boxes", action="store_true", help="the 128-box launch pair only")
ap.add_argument("--cpu", action="store_true", help="also time the CPU oracle on each row")
ap.add_argument("--out", default="", help="JSON file to append the rows to")
args = ap.parse_args()

ctx = klt.Context.get(0)
frames, gt = klt.synth_render(20261015, 1920, 1080, 128, 0, 1, ctx=ctx)
frame = frames[0]


def emit(row):
    print(json.dumps(row), flush=True)
    if args.out:
        rows = json.load(open(args.out)) if os.path.exists(args.out) else []
        rows.append(row)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


def measure(det, rois, names):
    for _ in range(10):  # code objects loaded, scratch grown
        c, n = det.detect_rois(frame, rois)
    torch.cuda.synchronize()
    ctx.timing_select(names)
    ctx.timing_enable(True)
    last = {k: ctx.timing_query(k) for k in names}
    means = {k: [] for k in names}
    for _ in range(args.blocks):
        for _ in range(args.launches):
            c, n = det.detect_rois(frame, rois)
        torch.cuda.synchronize()
        for k in names:
            n1, t1 = ctx.timing_query(k)
            n0, t0 = last[k]
            means[k].append(round(1e3 * (t1 - t0) / max(n1 - n0, 1), 2) if n1 > n0 else None)
            last[k] = (n1, t1)
    ctx.timing_enable(False)
    return means, n


if args.boxes:
    rois = []
    for g in gt[0].numpy():
        if not g[0]:
            continue
        x, y, w, h = (int(v) for v in g[1:])
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, 1920), min(y + h, 1080)
        if x1 - x0 >= 3 and y1 - y0 >= 3:
            rois.append((x0, y0, x1 - x0, y1 - y0))
    means, n = measure(klt.GoodFeaturesToTrackDetector(256, 0.01, 3.0), rois, ["gftt"])
    emit({"tag": args.tag, "what": "128 boxes (256, 0.01, 3.0)", "rois": len(rois),
          "launches_per_block": args.launches, "us_gftt": means["gftt"],
          "corners": int(n.clamp(min=0).sum().item())})
    sys.exit(0)

for maxc, q, md in ROWS:
    means, n = measure(klt.GoodFeaturesToTrackDetector(maxc, q, md), [(0, 0, 1920, 1080)], ["gftt", "gftt_wide"])
    row = {"tag": args.tag, "what": f"1080p frame ({maxc}, {q}, {md})", "launches_per_block": args.launches,
           "us_gftt": means["gftt"], "us_gftt_wide": means["gftt_wide"], "corners": int(n[0].item())}
    if args.cpu:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import _oracle as O

        f = frame.cpu().numpy()
        t0 = time.perf_counter()
        ref = O.gftt(f, maxc, q, md)
        row["us_cpu_oracle"] = round(1e6 * (time.perf_counter() - t0))
        assert len(ref) == row["corners"]
    emit(row)
