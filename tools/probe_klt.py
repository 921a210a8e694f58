"""Quick kernel probe: 1080p synthetic pair, 128 boxes x 256 points, 3-level LK.

  python tools/probe_klt.py            # the report
  python tools/probe_klt.py --json     # one JSON line: per-launch median (us) of lk_sparse for each kernel

TBDK_LIB selects another build of the library, so two builds can be compared
by alternating runs of this script."""
import argparse, json, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from opencv_amd import klt

ap = argparse.ArgumentParser()
ap.add_argument("--json", action="store_true", help="print only the JSON line of per-launch medians")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
say = (lambda *a: None) if args.json else print

ctx = klt.Context.get(0)
W, H, NOBJ = 1920, 1080, 128
frames, gt = klt.synth_render(20261015, W, H, NOBJ, 0, 2, ctx=ctx)
pts = []
rng = np.random.default_rng(0)
for o in range(NOBJ):
    v, x, y, w, h = gt[0, o].tolist()
    if not v: continue
    pts.append(np.stack([rng.uniform(x, x + w, 256), rng.uniform(y, y + h, 256)], 1))
pts = torch.from_numpy(np.concatenate(pts).astype(np.float32)).cuda()
n = pts.shape[0]
P0 = klt.Pyramid(ctx, W, H, 2).build(frames[0])
P1 = klt.Pyramid(ctx, W, H, 2).build(frames[1])
lk = klt.SparsePyrLKOpticalFlow((21, 21), 2, 30)
medians = {}


def median_us(name, flow, A, B):
    """per-launch median of lk_sparse over --reps launches, each timed on its own"""
    for _ in range(3):
        res = flow.calc(A, B, pts, want_iters=True)
    torch.cuda.synchronize()
    us = []
    for _ in range(args.reps):
        ctx.timing_enable(True)
        res = flow.calc(A, B, pts, want_iters=True)
        torch.cuda.synchronize()
        c, ms = ctx.timing_query("lk_sparse")
        us.append(ms / c * 1000)
    ctx.timing_enable(False)
    medians[name] = round(float(np.median(us)), 2)
    return res


if not args.json:
    for _ in range(3):
        r = lk.calc(P0, P1, pts, want_iters=True)
    torch.cuda.synchronize()
    ctx.timing_enable(True)
    t = time.time()
    for _ in range(20):
        P1.build(frames[1])
        r = lk.calc(P0, P1, pts, want_iters=True)
    torch.cuda.synchronize()
    wall = (time.time() - t) / 20
    for k in ["pyr_build", "lk_sparse"]:
        c, ms = ctx.timing_query(k)
        print(f"{k}: {c} launches, avg {ms / c * 1000:.1f} us")
    st = r.status.cpu().numpy(); it = r.iters.cpu().numpy()
    print(f"points {n}, tracked {st.mean():.3f}, mean iters {it.mean():.2f}, wall/iter {wall*1e3:.3f} ms")
    # the fp16 pixel path on the same frames and points
    Q0 = klt.Pyramid(ctx, W, H, 2, dtype=torch.float16).build(frames[0])
    Q1 = klt.Pyramid(ctx, W, H, 2, dtype=torch.float16).build(frames[1])
    r16 = median_us("fp16", lk, Q0, Q1)
    print(f"fp16 lk_sparse: median {medians['fp16']:.1f} us; mean iters {r16.iters.float().mean().item():.2f}")
r = median_us("impl0", lk, P0, P1)
# the other kernels for comparison (impl 1 strip, 2 generic LDS, 3 multi-point)
for impl in (1, 2, 3):
    r2 = median_us(f"impl{impl}", klt.SparsePyrLKOpticalFlow((21, 21), 2, 30, impl=impl), P0, P1)
    same = torch.equal(r2.next_pts, r.next_pts) and torch.equal(r2.status, r.status) and torch.equal(r2.iters, r.iters)
    say(f"impl {impl} lk_sparse: median {medians[f'impl{impl}']:.1f} us; same result: {same}")
# the same points on 3-channel frames: u8 (lk_cn_kernel) and 16U (lk_cn_f32_kernel)
c3 = [torch.stack([f, f // 2 + 30, 255 - f], 2).contiguous() for f in frames]
c3_u16 = [torch.from_numpy((f.cpu().numpy().astype(np.uint16) * 257).view(np.int16)).cuda().view(torch.uint16) for f in c3]
for name, fr, dt in (("cn3_u8", c3, torch.uint8), ("cn3_u16", c3_u16, torch.float32)):
    C0 = klt.Pyramid(ctx, W, H, 2, dtype=dt, channels=3).build(fr[0])
    C1 = klt.Pyramid(ctx, W, H, 2, dtype=dt, channels=3).build(fr[1])
    rc = median_us(name, lk, C0, C1)
    say(f"{name} lk_sparse: median {medians[name]:.1f} us; tracked {rc.status.float().mean().item():.3f}, "
        f"mean iters {rc.iters.float().mean().item():.2f}")
if args.json:
    print(json.dumps(dict(points=n, reps=args.reps, lib=os.environ.get("TBDK_LIB", ""), lk_sparse_median_us=medians)))
