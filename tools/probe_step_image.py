#!/usr/bin/env python3
"""Times the image front end and the detection-driven step.

Front end (the library's per-kernel HIP events, tbdk_timing_*, over `--reps`
launches after `--warmup`): BGR -> gray at 1080p, and 4K BGR -> gray at 1080p
(both scales exactly 2: the INTER_AREA path) and at 1600x900 (the bilinear
path), as the fused kernel and as the two calls; beside each, tbdk_hbm_copy
moving the same number of bytes (read + written), as the ceiling of a streaming
kernel.  The ratios say how far the kernels are from the copy; they are not a
pass mark.

The step (host clock around calls that end in a device synchronise): per frame
at 1080p, step_image on BGR frames next to HOG.detectMultiScale + TbdLoop.step
on the same frames converted beforehand, the two forms alternating frame by
frame on two loops; the difference is the front end plus the glue.  Rows: the
sample's HOG settings (64x128 detector, 15 levels, hit threshold 0.45) and hit
threshold -1.0 (more detections and tracks).

    python tools/probe_step_image.py [--out profiles/step_image_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_amd import hog as H  # noqa: E402
from opencv_amd import klt, tbd  # noqa: E402


def kernel_us(ctx, names, fn, warmup, reps):
    ctx.timing_enable(False)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ctx.timing_enable(True)
    ctx.timing_select(list(names))
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {}
    for k in names:
        n, ms = ctx.timing_query(k)
        out[k] = round(1e3 * ms / max(n, 1), 2)
    ctx.timing_enable(False)
    return out


def front_end(ctx, args):
    rows = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for name, (sw, sh), (dw, dh) in (("1080p_bgr_to_gray", (1920, 1080), (1920, 1080)),
                                     ("4k_bgr_to_1080p_gray_area", (3840, 2160), (1920, 1080)),
                                     ("4k_bgr_to_1600x900_gray_linear", (3840, 2160), (1600, 900))):
        src = torch.randint(0, 256, (sh, sw, 3), dtype=torch.uint8, device="cuda", generator=g)
        gray = torch.empty((sh, sw), dtype=torch.uint8, device="cuda")
        dst = torch.empty((dh, dw), dtype=torch.uint8, device="cuda")
        row = {"case": name, "src": [sw, sh], "dst": [dw, dh], "reps": args.reps}
        fused = kernel_us(ctx, ["cvt_resize_gray", "cvt_color"],
                          lambda: klt.cvt_resize_gray(src, klt.COLOR_BGR2GRAY, (dw, dh), dst=dst, ctx=ctx),
                          args.warmup, args.reps)
        row["fused_us"] = round(fused["cvt_resize_gray"] + fused["cvt_color"], 2)  # equal sizes run cvt_color alone
        row["fused_bytes"] = sw * sh * 3 + dw * dh
        if (sw, sh) != (dw, dh):
            def two():
                klt.cvt_color(src, klt.COLOR_BGR2GRAY, dst=gray, ctx=ctx)
                klt.resize_linear(gray, (dw, dh), dst=dst, ctx=ctx)

            t = kernel_us(ctx, ["cvt_color", "resize_linear"], two, args.warmup, args.reps)
            row["two_calls_us"] = round(t["cvt_color"] + t["resize_linear"], 2)
            row["two_calls_parts_us"] = t
            row["two_calls_bytes"] = sw * sh * 3 + 2 * sw * sh + dw * dh
        for key in ("fused", "two_calls"):
            if key + "_bytes" not in row:
                continue
            half = (row[key + "_bytes"] // 2 + 15) & ~15  # a copy reads and writes each byte once
            a = torch.empty(half, dtype=torch.uint8, device="cuda")
            b = torch.empty(half, dtype=torch.uint8, device="cuda")
            c = kernel_us(ctx, ["hbm_copy"], lambda: klt.hbm_copy(b, a, ctx=ctx), args.warmup, args.reps)["hbm_copy"]
            row[key + "_copy_us"] = c
            row[key + "_over_copy"] = round(row[key + "_us"] / c, 2) if c else None
            row[key + "_gbps"] = round(row[key + "_bytes"] / row[key + "_us"] / 1e3, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step(ctx, args):
    W, Hh, N, F = 1920, 1080, 32, args.frames
    frames, _ = klt.synth_render(20261015, W, Hh, N, 0, F, ctx=ctx)
    bgr = [torch.stack([f, torch.clamp(f.to(torch.int16) + 9, 0, 255).to(torch.uint8),
                        torch.clamp(f.to(torch.int16) - 7, 0, 255).to(torch.uint8)], 2).contiguous() for f in frames]
    gray = [klt.cvt_color(b, klt.COLOR_BGR2GRAY, ctx=ctx) for b in bgr]
    torch.cuda.synchronize()
    rows = []
    for name, hit in (("sample_settings_hit_0.45", 0.45), ("hit_-1.0", -1.0)):
        hg = H.HOG.create((64, 128), ctx=ctx)
        hg.setSVMDetector(hg.getDefaultPeopleDetector())
        hg.setNumLevels(15)
        hg.setHitThreshold(hit)
        cfg = tbd.default_config(W, Hh, bounds_xmax=W, bounds_ymax=Hh, track_confidence_threshold=-1.0)
        a, b = tbd.TbdLoop(cfg, ctx=ctx), tbd.TbdLoop(cfg, ctx=ctx)
        a.attach_detector(hg, confidence_mode=1)
        t_img, t_hog, t_step, ndet, ntr = [], [], [], [], []
        for f in range(F):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m, dets = a.step_image(bgr[f], f)
            t1 = time.perf_counter()
            rects, wts = hg.detectMultiScale(gray[f], confidences=True)
            t2 = time.perf_counter()
            mine = dets.copy()  # the same detections, as the caller of the two calls would build them
            t3 = time.perf_counter()
            mb = b.step(gray[f], f, mine)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            assert len(rects) == len(dets) and mb.ntracks == m.ntracks
            if f >= args.skip:
                t_img.append(1e3 * (t1 - t0))
                t_hog.append(1e3 * (t2 - t1))
                t_step.append(1e3 * (t4 - t3))
                ndet.append(len(dets))
                ntr.append(m.ntracks)
        med = statistics.median
        row = {"case": name, "size": [W, Hh], "frames_timed": len(t_img),
               "step_image_ms": round(med(t_img), 3), "hog_ms": round(med(t_hog), 3),
               "tbd_step_ms": round(med(t_step), 3),
               "front_end_plus_glue_ms": round(med(t_img) - med(t_hog) - med(t_step), 3),
               "step_image_ms_min_max": [round(min(t_img), 3), round(max(t_img), 3)],
               "detections_per_frame": round(sum(ndet) / len(ndet), 1), "tracks_per_frame": round(sum(ntr) / len(ntr), 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--skip", type=int, default=8, help="frames of the step loop left out of the medians")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    res = {"device": torch.cuda.get_device_name(0), "front_end": front_end(ctx, args), "step": step(ctx, args)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
