#!/usr/bin/env python3
"""What remap, remap_flow and warp_perspective cost at 1080p, beside tbdk_hbm_copy.

A synth_render frame as 8UC1 and three of them stacked as 8UC3; a smooth map
(a rotation by 3 degrees plus a sinusoid) and a noise map (grid + hashed noise
of +-6 px), both CV_32FC2.  Rows:

  remap            8UC1 / 8UC3, INTER_LINEAR, from the smooth and from the noise map
  remap_flow       the same noise as a flow, against `grid + flow` written by one
                   elementwise kernel (torch.add into a preallocated map) followed by
                   remap: the fused form moves 8 B/pixel fewer in each direction
  warp_perspective INTER_LINEAR and INTER_CUBIC, 8UC1, beside warp_affine with the
                   same affine part
  hbm_copy         tbdk_hbm_copy at 16 MiB (the maps' footprint, cache resident when
                   repeated) and at 512 MiB (beyond the caches)

Times are HIP events around blocks of `--calls` calls, `--reps` blocks per row, the
rows of a group alternating within a repetition; each is reported as median, min,
max and the runs.  A row's rate is its algorithmic bytes (map or flow + source +
destination) over its median time, given as a fraction of both copy rates (a
copy's bytes are read + written).

    python tools/probe_remap.py [--calls 50] [--reps 7] [--out profiles/remap_probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SEED, NOBJ = 1920, 1080, 20261015, 128


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "runs": [round(x, 3) for x in v]}


def timed(torch, fns, calls, reps):
    """us per call of every fn in fns (name -> callable), alternating within a repetition"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(1e3 * e0.elapsed_time(e1) / calls)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from opencv_amd import klt

    assert torch.cuda.is_available(), "needs a HIP device"
    ctx = klt.Context.get(0)
    frames, _ = klt.synth_render(SEED, W, H, NOBJ, 0, 3, ctx=ctx)
    g1 = frames[0].contiguous()
    g3 = frames.permute(1, 2, 0).contiguous()
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    grid = np.stack([xs, ys], -1)
    ang = np.deg2rad(3.0)
    cx, cy = W / 2, H / 2
    smooth = np.stack([cx + (xs - cx) * np.cos(ang) - (ys - cy) * np.sin(ang) + 2 * np.sin(ys / 40),
                       cy + (xs - cx) * np.sin(ang) + (ys - cy) * np.cos(ang) + 2 * np.cos(xs / 50)], -1).astype(np.float32)
    v = (np.arange(H * W * 2, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(SEED)) & np.uint64(0xFFFFFFFF)
    v = ((v ^ (v >> np.uint64(15))) * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    flow_h = (((v >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.float32) / 65536 - 0.5).reshape(H, W, 2) * 12
    flow_h = flow_h.astype(np.float32)
    t_smooth, t_flow, t_grid = (torch.from_numpy(a).cuda() for a in (smooth, flow_h, grid))
    t_noise = t_grid + t_flow
    t_map = torch.empty_like(t_grid)
    d1, d3 = torch.empty_like(g1), torch.empty_like(g3)
    px = W * H
    row = {"width": W, "height": H, "calls_per_rep": args.calls, "reps": args.reps}
    res, nbytes = {}, {}

    def add(group, bytes_of):
        us = timed(torch, group, args.calls, args.reps)
        for k, val in us.items():
            res[k] = spread(val)
            nbytes[k] = bytes_of[k]

    L, B = klt.INTER_LINEAR, klt.BORDER_REPLICATE
    add({"remap_8uc1_smooth": lambda: klt.remap(g1, t_smooth, None, L, B, dst=d1, ctx=ctx),
         "remap_8uc1_noise": lambda: klt.remap(g1, t_noise, None, L, B, dst=d1, ctx=ctx),
         "remap_8uc3_smooth": lambda: klt.remap(g3, t_smooth, None, L, B, dst=d3, ctx=ctx),
         "remap_8uc3_noise": lambda: klt.remap(g3, t_noise, None, L, B, dst=d3, ctx=ctx)},
        {"remap_8uc1_smooth": px * 10, "remap_8uc1_noise": px * 10, "remap_8uc3_smooth": px * 14,
         "remap_8uc3_noise": px * 14})

    def unfused(src, dst):
        torch.add(t_grid, t_flow, out=t_map)
        klt.remap(src, t_map, None, L, B, dst=dst, ctx=ctx)

    add({"remap_flow_8uc1": lambda: klt.remap_flow(g1, t_flow, 1, L, B, dst=d1, ctx=ctx),
         "map_then_remap_8uc1": lambda: unfused(g1, d1),
         "remap_flow_8uc3": lambda: klt.remap_flow(g3, t_flow, 1, L, B, dst=d3, ctx=ctx),
         "map_then_remap_8uc3": lambda: unfused(g3, d3),
         "map_kernel_alone": lambda: torch.add(t_grid, t_flow, out=t_map)},
        {"remap_flow_8uc1": px * 10, "map_then_remap_8uc1": px * (24 + 10), "remap_flow_8uc3": px * 14,
         "map_then_remap_8uc3": px * (24 + 14), "map_kernel_alone": px * 24})
    # fused and unfused give the same bytes
    a = klt.remap_flow(g3, t_flow, 1, L, B, ctx=ctx)
    unfused(g3, d3)
    torch.cuda.synchronize()
    assert torch.equal(a, d3), "remap_flow differs from remap of grid + flow"

    A = np.array([[np.cos(ang) * 1.02, -np.sin(ang), 11.5], [np.sin(ang), np.cos(ang) * 0.98, -7.25]])
    M = np.vstack([A, [1e-5, -2e-5, 1.0]])
    C_ = klt.INTER_CUBIC
    add({"warp_perspective_linear": lambda: klt.warp_perspective(g1, M, (W, H), L, B, dst=d1, ctx=ctx),
         "warp_affine_linear": lambda: klt.warp_affine(g1, A, (W, H), L, B, dst=d1, ctx=ctx),
         "warp_perspective_cubic": lambda: klt.warp_perspective(g1, M, (W, H), C_, B, dst=d1, ctx=ctx),
         "warp_affine_cubic": lambda: klt.warp_affine(g1, A, (W, H), C_, B, dst=d1, ctx=ctx)},
        {k: px * 2 for k in ("warp_perspective_linear", "warp_affine_linear", "warp_perspective_cubic",
                             "warp_affine_cubic")})

    small = [torch.empty(16 << 20, dtype=torch.uint8, device="cuda") for _ in range(2)]
    large = [torch.empty(512 << 20, dtype=torch.uint8, device="cuda") for _ in range(2)]
    add({"hbm_copy_16MiB": lambda: klt.hbm_copy(small[1], small[0], ctx=ctx),
         "hbm_copy_512MiB": lambda: klt.hbm_copy(large[1], large[0], ctx=ctx)},
        {"hbm_copy_16MiB": 2 * (16 << 20), "hbm_copy_512MiB": 2 * (512 << 20)})

    rate = {k: nbytes[k] / (res[k]["median"] * 1e-6) / 1e9 for k in res}  # GB/s
    row["us_per_call"] = res
    row["algorithmic_bytes"] = nbytes
    row["GB_per_s"] = {k: round(v, 1) for k, v in rate.items()}
    row["fraction_of_copy_16MiB"] = {k: round(rate[k] / rate["hbm_copy_16MiB"], 3) for k in res}
    row["fraction_of_copy_512MiB"] = {k: round(rate[k] / rate["hbm_copy_512MiB"], 3) for k in res}
    row["fused_over_unfused"] = {c: round(res[f"remap_flow_{c}"]["median"] / res[f"map_then_remap_{c}"]["median"], 3)
                                 for c in ("8uc1", "8uc3")}
    row["fused_over_unfused_bytes"] = {c: round(nbytes[f"remap_flow_{c}"] / nbytes[f"map_then_remap_{c}"], 3)
                                       for c in ("8uc1", "8uc3")}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
