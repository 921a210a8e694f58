#!/usr/bin/env python3
"""Steady-state time of BackgroundSubtractorMOG2.apply and getBackgroundImage at 1080p and 4K, 8UC1 and 8UC3,
nmixtures 5, shadows on, after `--warmup` frames of klt.synth_render's moving-object sequence (so the pixels
hold a realistic mix of mode counts); the distribution of modes_used; the algorithmic bytes of a frame for that
distribution (read: frame, modes_used and each used mode's weight, variance and mean; written: mask, the
modes_used bytes and the model words that changed, counted by comparing the model before and after a frame); and
the time klt.hbm_copy takes to move the same number of bytes in the same run, the denominator of the roofline
share.  Times are the library's per-kernel HIP events (tbdk_timing_*): the median over `--reps` frames.

    python tools/probe_mog2.py [--out profiles/mog2_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opencv_amd import bgsegm, klt  # noqa: E402


def events_us(ctx, kern, fns):
    """per-launch times (us) of kernel `kern` over the calls fns, one timing window per call"""
    us = []
    for fn in fns:
        ctx.timing_enable(True)
        ctx.timing_select([kern])
        fn()
        torch.cuda.synchronize()
        n, ms = ctx.timing_query(kern)
        ctx.timing_enable(False)
        assert n == 1, (kern, n)
        us.append(1e3 * ms)
    return us


def stats(us):
    return {"us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def words_changed(a, b):
    return int((a.view(torch.int32) != b.view(torch.int32)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    rows = []
    for (w, h) in ((1920, 1080), (3840, 2160)):
        total = args.warmup + args.reps + 1
        gray, _ = klt.synth_render(20261015, w, h, 32, 0, total, ctx=ctx)
        for cn in (1, 3):
            def frame(t):
                g = gray[t]
                return g if cn == 1 else torch.stack([g, torch.roll(g, 1, 1), torch.roll(g, 1, 0)], -1).contiguous()

            m = bgsegm.BackgroundSubtractorMOG2.create(ctx=ctx)
            mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            for t in range(args.warmup):
                m.apply(frame(t), mask)
            torch.cuda.synchronize()
            fr = [frame(args.warmup + k) for k in range(args.reps + 1)]
            apply_us = events_us(ctx, "mog2_apply", [lambda f=f: m.apply(f, mask) for f in fr[:-1]])
            bg = m.getBackgroundImage()
            bg_us = events_us(ctx, "mog2_background", [lambda: m.getBackgroundImage(bg)] * 5)
            # one more frame between two copies of the model: the words it changes
            before = m.model()
            m.apply(fr[-1], mask)
            after = m.model()
            torch.cuda.synchronize()
            used0, used1 = before[3].to(torch.int64), after[3].to(torch.int64)
            hist = torch.bincount(used0.reshape(-1), minlength=6).cpu().tolist()
            px = w * h
            model_state = px * 5 * (2 + cn) * 4 + px
            read = px * cn + px + int(used0.sum()) * (2 + cn) * 4
            changed = sum(words_changed(a, b) for a, b in zip(before[:3], after[:3]))
            written = px + int((used0 != used1).sum()) + changed * 4
            nbytes = read + written
            half = (nbytes // 2) // 16 * 16
            src = torch.empty(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            copy_us = events_us(ctx, "hbm_copy", [lambda: klt.hbm_copy(dst, src, ctx=ctx)] * 10)
            del before, after, src, dst
            a, c = stats(apply_us), stats(copy_us)
            row = {"shape": f"{w}x{h}", "type": f"8UC{cn}", "nmixtures": 5, "detect_shadows": True,
                   "warmup_frames": args.warmup, "reps": args.reps, "apply": a, "get_background": stats(bg_us),
                   "modes_used_hist": hist, "mean_modes": round(float(used0.float().mean()), 3),
                   "model_state_bytes": model_state, "bytes_read": read, "bytes_written": written,
                   "bytes_per_frame": nbytes, "apply_GBps": round(nbytes / a["us"] / 1e3, 1),
                   "hbm_copy_same_bytes": c, "hbm_copy_GBps": round(2 * half / c["us"] / 1e3, 1),
                   "share_of_copy": round((nbytes / a["us"]) / (2 * half / c["us"]), 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del m
        del gray
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
