"""The case table of cv::findHomography (tests/golden/reference_homography.npz).
Shared by tools/record_reference_cases.py, tests/test_homography_oracle.py,
tests/test_homography_core_host.py and tests/test_gpu_homography.py.

Point sets come from a ground-truth homography on a 640x480 field: inliers get
uniform noise of at most 0.5 px, outliers are uniform over the field.  The
recorder stores the generated sets in the fixture and the tests read them from
there, so the fixture does not depend on the generator's stream.

A case is (label, points, n, outlier %, truth, status, method, threshold,
max_iters, confidence, seed).  `status` applies before the reference is called:
the reference sees the compacted pairs, and its mask is over those."""
import numpy as np

W, H = 640, 480
LSQ, RANSAC = 0, 8

TRUTHS = {
    "mild": np.array([[1.02, 0.03, 5.0], [-0.02, 0.98, -3.0], [4e-5, -3e-5, 1.0]]),
    "shift": np.array([[1.0, 0.0, 7.25], [0.0, 1.0, -4.5], [0.0, 0.0, 1.0]]),
    # w = 1 + 1.5e-3 x - 1e-3 y: between 0.52 and 1.96 on the field
    "strong": np.array([[0.9, -0.2, 40.0], [0.25, 1.1, -20.0], [1.5e-3, -1e-3, 1.0]]),
}


def _apply(T, p):
    w = T[2, 0] * p[:, 0] + T[2, 1] * p[:, 1] + T[2, 2]
    return np.stack([(T[0, 0] * p[:, 0] + T[0, 1] * p[:, 1] + T[0, 2]) / w,
                     (T[1, 0] * p[:, 0] + T[1, 1] * p[:, 1] + T[1, 2]) / w], 1)


def _plane(rng, n, outliers, truth):
    src = rng.uniform([0, 0], [W, H], (n, 2))
    dst = _apply(TRUTHS[truth], src) + rng.uniform(-0.5, 0.5, (n, 2))
    out = rng.permutation(n)[:int(round(n * outliers / 100.0))]
    dst[out] = rng.uniform([0, 0], [W, H], (len(out), 2))
    return src, dst


def points(kind, n, outliers, truth, seed):
    """(src, dst) float32 [n, 2]"""
    rng = np.random.default_rng(seed)
    if kind == "plane":
        src, dst = _plane(rng, n, outliers, truth)
    elif kind == "collinear":  # every point on one line: no subset passes
        t = 2.0 * rng.permutation(200)[:n]  # integers: the cross products are exactly zero in float
        src = np.stack([20 + t, 30 + 0.5 * t], 1)
        dst = src + [3.0, 1.0]
    elif kind == "coincident":
        src = np.tile([[100.0, 120.0]], (n, 1))
        dst = np.tile([[104.0, 118.0]], (n, 1))
    elif kind == "line4":  # n points of which n - 1 are collinear (5: four on a line)
        t = np.linspace(0, 300, n - 1)
        src = np.concatenate([np.stack([50 + t, 60 + 0.25 * t], 1), [[200.0, 400.0]]])
        dst = _apply(TRUTHS["mild"], src)
    elif kind == "planes2":  # two interleaved planes of near-equal size
        src = rng.uniform([0, 0], [W, H], (n, 2))
        dst = _apply(TRUTHS["mild"], src)
        dst[1::2] = _apply(TRUTHS["strong"], src[1::2])
        dst += rng.uniform(-0.5, 0.5, (n, 2))
    elif kind == "dup":  # every pair twice
        s, d = _plane(rng, n // 2, outliers, truth)
        src, dst = np.repeat(s, 2, 0), np.repeat(d, 2, 0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(src, np.float32).reshape(n, 2), np.ascontiguousarray(dst, np.float32).reshape(n, 2)


def status(kind, n):
    if kind is None:
        return None
    if kind == "ones":
        return np.ones(n, np.uint8)
    if kind == "alt":
        return (np.arange(n) % 2 == 0).astype(np.uint8)
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "few":  # three ones among many
        s = np.zeros(n, np.uint8)
        s[[1, n // 2, n - 2]] = 1
        return s
    raise ValueError(kind)


def _c(label, kind="plane", n=200, out=30, truth="mild", st=None, method=RANSAC, thr=3.0, iters=2000, conf=0.995,
       seed=0):
    return (label, kind, n, out, truth, st, method, thr, iters, conf, seed)


def cases():
    c = []
    # sizes (1000 is the sample's maxCorners); 30 % outliers stop inside the first batch of 64
    for n in (0, 3, 4, 5, 8, 63, 64, 65, 200, 1000):
        c.append(_c(f"size {n}", n=n, seed=100 + n))
    # outlier shares: 0 % stops in iteration 0, 60 % several batches in
    for out in (0, 60, 85):  # 85 %: eight batches, no early stop (500 keeps the restatement quick)
        c.append(_c(f"outliers {out}", out=out, iters=500 if out == 85 else 2000, seed=200 + out))
    for thr in (1.0, 10.0, 0.0, -2.0):
        c.append(_c(f"threshold {thr}", thr=thr, seed=300))
    # 85 % outliers at threshold 1: niters stays at max_iters (no consensus at 300), so the loop ends at
    # iteration 0, inside the first batch, at the batch boundary and one either side of it, batches in
    for it in (1, 7, 63, 64, 65, 300):
        c.append(_c(f"max_iters {it}", n=65, out=85, thr=1.0, iters=it, seed=400))
    c.append(_c("max_iters 300 of 200", out=60, iters=300, seed=401))
    for conf in (0.9, 0.9999):
        c.append(_c(f"confidence {conf}", out=60, conf=conf, seed=500))
    for truth in ("shift", "strong"):
        c.append(_c(f"truth {truth}", truth=truth, seed=600))
    c.append(_c("collinear", kind="collinear", n=20, seed=700))
    c.append(_c("coincident", kind="coincident", n=10, seed=701))
    c.append(_c("5 points, 4 collinear", kind="line4", n=5, seed=702))
    c.append(_c("two planes", kind="planes2", n=200, seed=703))
    c.append(_c("inliers on a line but one", kind="line4", n=12, seed=704))
    c.append(_c("duplicated pairs", kind="dup", n=64, out=25, seed=705))
    for st, n in (("ones", 200), ("alt", 200), ("zero", 200), ("few", 50)):
        c.append(_c(f"status {st}", n=n, st=st, seed=800))
    for n in (4, 5, 64, 1000):
        c.append(_c(f"method 0 size {n}", n=n, out=0, method=LSQ, seed=900 + n))
    return c


NCASES = 42


def label(i):
    return cases()[i][0]


def inputs(i):
    """(src, dst, status or None, method, threshold, max_iters, confidence) of case i"""
    _, kind, n, out, truth, st, method, thr, iters, conf, seed = cases()[i]
    src, dst = points(kind, n, out, truth, seed)
    return src, dst, status(st, n), method, thr, iters, conf


def compact(src, dst, st):
    """what the reference sees: the status != 0 pairs, in order"""
    if st is None:
        return src, dst
    k = st != 0
    return np.ascontiguousarray(src[k]), np.ascontiguousarray(dst[k])


def fixture_inputs(fx, i):
    """case i as recorded: (src, dst, status or None, method, threshold, max_iters, confidence), the points from the
    fixture"""
    _, _, _, _, _, _, method, thr, iters, conf, _ = cases()[i]
    st = fx[f"status_{i}"] if f"status_{i}" in fx.files else None
    return fx[f"src_{i}"], fx[f"dst_{i}"], st, method, thr, iters, conf


def fixture_outputs(fx, i, n):
    """(valid, ninliers, mask [n], H noavx2 [3, 3], H default [3, 3]) of case i over its n compacted pairs"""
    valid, nin = (int(v) for v in fx[f"{i}_valid"])
    mask = np.unpackbits(fx[f"{i}_mask"])[:n]
    h = fx[f"{i}_H"]
    other = fx[f"other_{i}_H"] if f"other_{i}_H" in fx.files else h
    return valid, nin, mask, h, other
