#!/usr/bin/env python3
"""Time of tbdk_gaussian_blur_u8 on a 1920 x 1080 one-channel image: 11 x 11 at sigma 3.5, the same with the
threshold fused in (bgsegm.smooth_mask), 31 x 31 at sigma 5, 3 x 3 and 5 x 5 at sigma 0, the 11 x 11 through the
run-time-size instance (ctx option blur_generic), and the 11 x 11 on a BGR image; tbdk_threshold (BINARY and
THRESH_OTSU) on the same image.  Times are the library's HIP events (tbdk_timing_*), one window per call, the median
of `--calls` calls after `--warmup`; klt.hbm_copy of the same bytes (the image read once and written once) in the
same run is the denominator.

    python tools/probe_blur.py [--out profiles/blur_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_amd import bgsegm, imgproc, klt  # noqa: E402


def window(ctx, name, fn):
    ctx.timing_enable(True)
    ctx.timing_select([name])
    fn()
    torch.cuda.synchronize()
    n, ms = ctx.timing_query(name)
    ctx.timing_enable(False)
    assert n == 1, (name, n)
    return 1e3 * ms


def median_us(ctx, name, fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = [window(ctx, name, fn) for _ in range(calls)]
    return {"us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "n": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    w, h = 1920, 1080
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    rows = []
    for cn in (1, 3):
        shape = (h, w) if cn == 1 else (h, w, cn)
        # a foreground mask's content: 0 / 255 blobs, which saturate the row sums
        img = (torch.rand((h // 8 + 1, w // 8 + 1), device="cuda", generator=gen) < 0.3).to(torch.uint8) * 255
        img = img.repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w]
        img = img.contiguous() if cn == 1 else img[:, :, None].expand(h, w, cn).contiguous()
        dst = torch.empty(shape, dtype=torch.uint8, device="cuda")
        nbytes = img.numel()
        a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        copy = median_us(ctx, "hbm_copy", lambda: klt.hbm_copy(b, a, ctx=ctx), args.warmup, args.calls)
        jobs = {"blur 11x11 sigma 3.5": ("blur", lambda: imgproc.gaussian_blur(img, (11, 11), 3.5, dst, 3.5, ctx=ctx))}
        if cn == 1:
            jobs.update({
                "blur 11x11 sigma 3.5 + threshold 10 fused (smooth_mask)":
                    ("blur", lambda: bgsegm.smooth_mask(img, dst=dst, ctx=ctx)),
                "blur 31x31 sigma 5": ("blur", lambda: imgproc.gaussian_blur(img, (31, 31), 5.0, dst, ctx=ctx)),
                "blur 3x3 sigma 0": ("blur", lambda: imgproc.gaussian_blur(img, (3, 3), 0, dst, ctx=ctx)),
                "blur 5x5 sigma 0": ("blur", lambda: imgproc.gaussian_blur(img, (5, 5), 0, dst, ctx=ctx)),
                "blur 11x11 sigma 3.5 in place (two launches)":
                    ("blur", lambda: imgproc.gaussian_blur(dst, (11, 11), 3.5, dst, 3.5, ctx=ctx)),
                "threshold binary": ("threshold", lambda: imgproc.threshold(img, 10, 255, 0, dst, ctx=ctx)),
                "threshold otsu": ("threshold", lambda: imgproc.threshold(img, 0, 255, 8, dst, ctx=ctx)),
            })
        for what, (name, fn) in jobs.items():
            r = median_us(ctx, name, fn, args.warmup, args.calls)
            rows.append({"shape": f"{w}x{h}", "type": f"8UC{cn}", "what": what, "bytes_read_plus_written": 2 * nbytes,
                         **r, "hbm_copy_same_bytes": copy, "times_the_copy": round(r["us"] / copy["us"], 2)})
            print(json.dumps(rows[-1]), flush=True)
        if cn == 1:
            ctx.set_option("blur_generic", 1)
            r = median_us(ctx, "blur", jobs["blur 11x11 sigma 3.5"][1], args.warmup, args.calls)
            ctx.set_option("blur_generic", 0)
            rows.append({"shape": f"{w}x{h}", "type": "8UC1", "what": "blur 11x11 sigma 3.5, run-time-size instance",
                         "bytes_read_plus_written": 2 * nbytes, **r, "hbm_copy_same_bytes": copy,
                         "times_the_copy": round(r["us"] / copy["us"], 2)})
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
