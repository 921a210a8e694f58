#!/usr/bin/env python3
"""Time per frame of BackgroundSubtractorKNN.apply at 1920x1080 and 1242x375, 8UC3 and 8UC1, defaults (nN 7, kNN 2,
shadows on), over `--frames` frames after `--warmup`, on three scenes: `static` (one frame repeated: every pixel
returns at the second sample), `noise` (independent uniform bytes: no pixel returns early, both passes read every
sample) and `sequence` (klt.synth_render's moving objects).  Times are the library's HIP events (tbdk_timing_*),
one window per frame: "knn_apply" (the kernel, and the clear on an initialising frame) and "knn_randu" (the fills
of the frames that have some), and "mog2_apply" on the same frames for orientation.  The bytes the kernel must
move are counted from the layout (a sample is 4 bytes for BGR, 2 for gray): worst case the whole model read once,
the frame in, the mask out, three samples written and the six plane bytes read; static case kNN samples instead
of the model and nothing written.  klt.hbm_copy's rate on the worst-case byte count, in the same run, is the
denominator of the shares.

    python tools/probe_knn.py [--out profiles/knn_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_amd import bgsegm, klt  # noqa: E402


def window(ctx, names, fn):
    """{name: (launches, ms)} of one call"""
    ctx.timing_enable(True)
    ctx.timing_select(list(names))
    fn()
    torch.cuda.synchronize()
    out = {k: ctx.timing_query(k) for k in names}
    ctx.timing_enable(False)
    return out


def stats(us):
    if not us:
        return None
    return {"us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "mean_us": round(float(np.mean(us)), 2), "n": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    rows = []
    total = args.warmup + args.frames
    for (w, h) in ((1920, 1080), (1242, 375)):
        gray, _ = klt.synth_render(20261015, w, h, 32, 0, total, ctx=ctx)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        for cn in (3, 1):
            def colour(g):
                return g if cn == 1 else torch.stack([g, torch.roll(g, 1, 1), torch.roll(g, 1, 0)], -1).contiguous()

            shape = (h, w) if cn == 1 else (h, w, 3)
            scenes = {"static": lambda t: colour(gray[0]),
                      "noise": lambda t: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen),
                      "sequence": lambda t: colour(gray[t])}
            px, word, nN, kNN = w * h, (4 if cn == 3 else 2), 7, 2
            worst = px * (3 * nN * word + cn + 1 + 3 * word + 6)
            static = px * (kNN * word + cn + 1 + 6)
            half = (worst // 2) // 16 * 16
            src = torch.empty(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            copy_us = [1e3 * window(ctx, ["hbm_copy"], lambda: klt.hbm_copy(dst, src, ctx=ctx))["hbm_copy"][1]
                       for _ in range(10)]
            copy_rate = 2 * half / float(np.median(copy_us)) / 1e3  # GB/s
            del src, dst
            for scene, frame in scenes.items():
                knn = bgsegm.createBackgroundSubtractorKNN(ctx=ctx)
                mog = bgsegm.createBackgroundSubtractorMOG2(ctx=ctx)
                mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
                for t in range(args.warmup):
                    f = frame(t)
                    knn.apply(f, mask)
                    mog.apply(f, mask)
                torch.cuda.synchronize()
                apply_us, randu_us, mog_us = [], [], []
                for t in range(args.warmup, total):
                    f = frame(t)
                    r = window(ctx, ["knn_apply", "knn_randu"], lambda: knn.apply(f, mask))
                    assert r["knn_apply"][0] == 1
                    apply_us.append(1e3 * r["knn_apply"][1])
                    if r["knn_randu"][0]:
                        randu_us.append(1e3 * r["knn_randu"][1])
                    mog_us.append(1e3 * window(ctx, ["mog2_apply"], lambda: mog.apply(f, mask))["mog2_apply"][1])
                bg_share = float((mask == 0).float().mean())
                a = stats(apply_us)
                nbytes = static if scene == "static" else worst
                row = {"shape": f"{w}x{h}", "type": f"8UC{cn}", "scene": scene, "nsamples": nN, "knn_samples": kNN,
                       "warmup_frames": args.warmup, "frames": args.frames, "knn_apply": a,
                       "knn_randu_per_frame_with_fills": stats(randu_us),
                       "knn_randu_mean_us_over_all_frames": round(float(np.sum(randu_us)) / args.frames, 2),
                       "mog2_apply": stats(mog_us), "background_share_last_mask": round(bg_share, 3),
                       "bytes_worst_case": worst, "bytes_static_case": static, "bytes_counted": nbytes,
                       "apply_GBps_of_counted": round(nbytes / a["us"] / 1e3, 1),
                       "hbm_copy_GBps": round(copy_rate, 1),
                       "share_of_copy": round((nbytes / a["us"] / 1e3) / copy_rate, 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del knn, mog
        del gray
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
