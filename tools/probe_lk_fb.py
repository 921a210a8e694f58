#!/usr/bin/env python3
"""What the forward-backward check costs.

1. Standalone: 1080p, ~18.6k grid points, window 21, 3 levels.  tbdk_lk_sparse_fb
   (SparsePyrLKOpticalFlow.calc_checked) next to the unfused composition it
   replaces -- two tbdk_lk_sparse calls with swapped pyramids plus the comparison
   in torch -- in alternating repetitions of `--calls` calls each, host clock
   around work that ends in a device synchronise.  The two status vectors are
   checked equal first.  The backward launch's share comes from the library's
   per-kernel HIP events ("lk_sparse", "lk_sparse_back") in a pass of its own.
2. The loop: bench.py's 1080p x 128-object configuration with ctx option
   tbd_fb_check at 1024 and at 0, alternating runs, each a fresh process
   (`bench.py --no-secondary --no-cpu-baseline --kstats lk_sparse,lk_sparse_back`).

    python tools/probe_lk_fb.py [--out profiles/lk_fb_probe.json] [--part standalone|loop|all]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "runs": [round(x, 3) for x in v]}


def standalone(args):
    import numpy as np
    import torch

    from opencv_amd import klt

    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    W, H, win, ml, thr = 1920, 1080, 21, 2, 1.0
    frames, _ = klt.synth_render(20261015, W, H, 128, 0, 2, ctx=ctx)
    ys, xs = np.mgrid[8:H - 8:10, 8:W - 8:11]
    pts = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)).cuda()
    n = pts.shape[0]
    lk = klt.SparsePyrLKOpticalFlow((win, win), ml, 30)
    Pa = klt.build_pyramid(frames[0], (win, win), ml, ctx=ctx, derivs=False)
    Pb = klt.build_pyramid(frames[1], (win, win), ml, ctx=ctx, derivs=False)
    thr_t = torch.tensor(thr, dtype=torch.float32, device="cuda")

    def fused():
        return lk.calc_checked(Pa, Pb, pts, back_threshold=thr, want_err=False).status

    def unfused():
        f = lk.calc(Pa, Pb, pts, want_err=False)
        b = lk.calc(Pb, Pa, f.next_pts, want_err=False)
        d = (pts - b.next_pts).abs().amax(1)
        return f.status & b.status & (d < thr_t).to(torch.uint8)

    for _ in range(args.warmup):
        a, b = fused(), unfused()
    torch.cuda.synchronize()
    assert torch.equal(a, b), "fused and unfused status differ"
    us = {"fused": [], "unfused": []}
    for _ in range(args.reps):
        for name, fn in (("fused", fused), ("unfused", unfused)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            us[name].append(1e6 * (time.perf_counter() - t0) / args.calls)
    kern = {}
    ctx.timing_enable(True)
    ctx.timing_select(["lk_sparse", "lk_sparse_back"])
    for _ in range(args.calls):
        fused()
    torch.cuda.synchronize()
    for k in ("lk_sparse", "lk_sparse_back"):
        cnt, ms = ctx.timing_query(k)
        kern[k + "_us"] = round(1e3 * ms / max(cnt, 1), 2)
    ctx.timing_enable(False)
    row = {"width": W, "height": H, "points": n, "win": win, "levels": ml + 1, "back_threshold": thr,
           "kept": int(a.sum().item()), "calls_per_rep": args.calls, "reps": args.reps,
           "fused_us_per_call": spread(us["fused"]), "unfused_us_per_call": spread(us["unfused"]),
           "fused_kernels": kern,
           "back_share_of_kernel_time": round(kern["lk_sparse_back_us"] /
                                              (kern["lk_sparse_us"] + kern["lk_sparse_back_us"]), 3),
           # judged against the repetitions' own spread: the fused call's slowest
           # repetition against the composition's fastest, and the medians
           "fused_not_slower": statistics.median(us["fused"]) <= statistics.median(us["unfused"]),
           "fused_max_below_unfused_min": max(us["fused"]) <= min(us["unfused"])}
    print(json.dumps(row), flush=True)
    return row


def bench_once(opt, args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", "20",
           "--no-secondary", "--no-cpu-baseline", "--kstats", "lk_sparse,lk_sparse_back,tbd_fit",
           "--ctx-option", f"tbd_fb_check={opt}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def loop(args):
    runs = {1024: [], 0: []}
    for _ in range(args.rounds):
        for opt in (1024, 0):
            d = bench_once(opt, args)
            runs[opt].append(d)
            print(json.dumps({"tbd_fb_check": opt, "frames_per_s": d["value"], "ms_per_step": d["ms_per_step"]}),
                  flush=True)
    out = {"command": "python bench.py --gpus 1 --steps %d --warmup 20 --no-secondary --no-cpu-baseline "
                      "--kstats lk_sparse,lk_sparse_back,tbd_fit --ctx-option tbd_fb_check=N" % args.steps,
           "rounds": args.rounds}
    for opt, ds in runs.items():
        last = ds[-1]
        out[f"tbd_fb_check_{opt}"] = {
            "frames_per_s": spread([d["value"] for d in ds]), "ms_per_step": spread([d["ms_per_step"] for d in ds]),
            "kernels": last.get("kernels"), "per_frame": last.get("per_frame")}
    a, b = out["tbd_fb_check_1024"]["ms_per_step"]["median"], out["tbd_fb_check_0"]["ms_per_step"]["median"]
    out["added_us_per_step"] = round(1e3 * (a - b), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["standalone", "loop", "all"], default="all")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=480)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    if args.part in ("loop", "all"):  # child processes first: this one has not opened the device yet
        res["loop"] = loop(args)
    if args.part in ("standalone", "all"):
        res["standalone"] = standalone(args)
        import torch

        res["device"] = torch.cuda.get_device_name(0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
