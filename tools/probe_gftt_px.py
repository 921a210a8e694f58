"""Standalone GFTT timing over the bench frame's boxes for each pixel type
(the 16U / 32F row): 1080p x 128 boxes, (256, .01, 3.0), HIP events
over the launch pair (the context's "gftt" timing record), blocks of launches.

    python tools/probe_gftt_px.py KIND[,KIND...] [--blocks 5] [--launches 300] [--root DIR] [--tag NAME]

KIND: u8 (the synthetic bench frame), unit (that frame plus a hashed sub-LSB
fraction, over 255, float32), u16 (the frame in the high byte, hashed noise in the
low one), u8f (the frame's integers as float32: no fresh start differs, the
price of the wider loads alone), hdr (tests/_gftt_f32_cases.hdr: every fresh start of the eigenvalue
walk differs from the running sum).  --root: the checkout whose opencv_amd
package (and built library) is measured, so that another commit's build can be
alternated with this one in one session; such a checkout needs only `u8`.
Prints one JSON line per kind: the blocks' mean microseconds per launch pair."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("kinds")
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--launches", type=int, default=300)
ap.add_argument("--root", default=ROOT)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from opencv_amd import klt  # noqa: E402

ctx = klt.Context.get(0)
frames, gt = klt.synth_render(20261015, 1920, 1080, 128, 0, 1, ctx=ctx)
rois = []
for g in gt[0].numpy():
    if not g[0]:
        continue
    x, y, w, h = (int(v) for v in g[1:])
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, 1920), min(y + h, 1080)
    if x1 - x0 >= 3 and y1 - y0 >= 3:
        rois.append((x0, y0, x1 - x0, y1 - y0))
base = frames[0].cpu().numpy()


def image(kind):
    if kind == "u8":
        return frames[0]
    import _gftt_f32_cases as FC

    H, W = base.shape
    if kind == "unit":
        frac = FC._hash16(W, H, 1).astype(np.float32) / np.float32(65536)
        a = ((base.astype(np.float32) + frac) / np.float32(255)).astype(np.float32)
    elif kind == "u16":
        a = ((base.astype(np.uint16) << 8) | (FC._hash16(W, H, 2) & 255).astype(np.uint16)).astype(np.uint16)
    elif kind == "u8f":
        a = base.astype(np.float32)
    elif kind == "hdr":
        a = FC.hdr(W, H, 3)
    else:
        raise SystemExit(f"unknown kind {kind}")
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


det = klt.GoodFeaturesToTrackDetector(256, 0.01, 3.0)
for kind in args.kinds.split(","):
    img = image(kind)
    for _ in range(50):  # code objects loaded, scratch grown
        c, n = det.detect_rois(img, rois)
    torch.cuda.synchronize()
    ctx.timing_select(["gftt"])
    ctx.timing_enable(True)
    n0, t0 = ctx.timing_query("gftt")
    means = []
    for _ in range(args.blocks):
        for _ in range(args.launches):
            c, n = det.detect_rois(img, rois)
        torch.cuda.synchronize()
        n1, t1 = ctx.timing_query("gftt")
        means.append(1e3 * (t1 - t0) / max(n1 - n0, 1))
        n0, t0 = n1, t1
    ctx.timing_enable(False)
    print(json.dumps({"tag": args.tag, "kind": kind, "rois": len(rois), "px": sum(r[2] * r[3] for r in rois),
                      "launches_per_block": args.launches, "us_per_launch_pair": [round(m, 2) for m in means],
                      "corners": int(n.clamp(min=0).sum().item())}), flush=True)
