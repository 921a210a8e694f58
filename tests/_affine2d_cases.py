"""The case table of cv::estimateAffine2D / cv::estimateAffinePartial2D
(tests/golden/reference_affine2d.npz).  Shared by tools/record_reference_cases.py,
tests/test_affine2d_oracle.py, tests/test_affine2d_core_host.py and
tests/test_gpu_affine2d.py.

Point sets come from a ground-truth 2x3 matrix on a 640x480 field: inliers get
uniform noise of at most 0.5 px, outliers are uniform over the field.  The
recorder stores the generated sets in the fixture and the tests read them from
there, so the fixture does not depend on the generator's stream.  A set is
shared by every case with the same (kind, n, outlier %, truth, seed): the two
models and the two methods mostly run on the same sets.

A case is (label, points, n, outlier %, truth, status, model, method,
threshold, max_iters, confidence, seed).  `status` applies before the reference
is called: the reference sees the compacted pairs, and its mask is over those."""
import numpy as np

W, H = 640, 480
FULL, PARTIAL = 0, 1
RANSAC, LMEDS = 8, 4
MODEL_NAME = {FULL: "full", PARTIAL: "partial"}

_a = np.deg2rad(3.0)
TRUTHS = {
    "similarity": np.array([[1.05 * np.cos(_a), -1.05 * np.sin(_a), 6.0], [1.05 * np.sin(_a), 1.05 * np.cos(_a), -4.0]]),
    "shear": np.array([[1.03, 0.12, 5.0], [-0.04, 0.95, -3.0]]),
    "shift": np.array([[1.0, 0.0, 7.25], [0.0, 1.0, -4.5]]),
    "reflection": np.array([[-1.0, 0.0, 630.0], [0.0, 1.0, 3.0]]),  # the partial model cannot represent it
}


def _apply(T, p):
    return np.stack([T[0, 0] * p[:, 0] + T[0, 1] * p[:, 1] + T[0, 2], T[1, 0] * p[:, 0] + T[1, 1] * p[:, 1] + T[1, 2]], 1)


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
    elif kind == "collinear":  # every point on one line: no 3-point subset passes, every 2-point one does
        t = 2.0 * rng.permutation(200)[:n]  # integers: the cross products are exactly zero in float
        src = np.stack([20 + t, 30 + 0.5 * t], 1)
        dst = src + [3.0, 1.0]
    elif kind == "coincident":
        src = np.tile([[100.0, 120.0]], (n, 1))
        dst = np.tile([[104.0, 118.0]], (n, 1))
    elif kind == "line":  # n points of which n - 1 are collinear
        t = np.linspace(0, 300, n - 1)
        src = np.concatenate([np.stack([50 + t, 60 + 0.25 * t], 1), [[200.0, 400.0]]])
        dst = _apply(TRUTHS[truth], src)
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


SIZES = (0, 1, 2, 3, 4, 5, 8, 63, 64, 65, 200, 1000)


def _model_cases(model):
    name = MODEL_NAME[model]

    def c(label, kind="plane", n=200, out=30, truth="similarity", st=None, method=RANSAC, thr=3.0, iters=2000,
          conf=0.99, seed=0):
        return (f"{name} {label}", kind, n, out, truth, st, model, method, thr, iters, conf, seed)

    r = []
    # sizes straddle modelPoints and the batch of 64
    for n in SIZES:
        r.append(c(f"size {n}", n=n, seed=100 + n))
    for out in (0, 60, 85):  # 85 %: many batches (500 keeps the restatement quick)
        r.append(c(f"outliers {out}", out=out, iters=500 if out == 85 else 2000, seed=200 + out))
    for thr in (1.0, 10.0, 0.0, -2.0):  # 0 and -2: the threshold is not defaulted
        r.append(c(f"threshold {thr}", thr=thr, seed=300))
    # 85 % outliers at threshold 1: the loop ends at iteration 0, inside the first batch, at its boundary and one
    # either side of it, batches in
    for it in (1, 7, 63, 64, 65, 300):
        r.append(c(f"max_iters {it}", n=65, out=85, thr=1.0, iters=it, seed=400))
    for conf in (0.9, 0.9999):
        r.append(c(f"confidence {conf}", out=60, conf=conf, seed=260))
    for truth in ("shear", "shift", "reflection"):
        r.append(c(f"truth {truth}", truth=truth, seed=600))
    r.append(c("collinear", kind="collinear", n=20, seed=700))
    r.append(c("coincident", kind="coincident", n=10, seed=701))
    r.append(c("all but one collinear", kind="line", n=12, seed=704))
    r.append(c("duplicated pairs", kind="dup", n=64, out=25, seed=705))
    for st, n in (("ones", 200), ("alt", 200), ("zero", 200), ("few", 50)):
        r.append(c(f"status {st}", n=n, st=st, seed=800))
    # LMEDS: even and odd counts (the rank count/2), 30 % outliers
    for n in SIZES:
        r.append(c(f"lmeds size {n}", n=n, method=LMEDS, seed=100 + n))
    r.append(c("lmeds outliers 60", out=60, method=LMEDS, seed=260))  # beyond its breakdown point: a poor model
    r.append(c("lmeds confidence 0.3", method=LMEDS, conf=0.3, seed=300))  # MAX(niters, 3) applies
    r.append(c("lmeds max_iters 5", method=LMEDS, iters=5, seed=300))  # below the computed niters
    r.append(c("lmeds collinear", kind="collinear", n=20, method=LMEDS, seed=700))  # getSubset's 1000 attempts
    r.append(c("lmeds truth reflection", truth="reflection", method=LMEDS, seed=600))
    return r


def cases():
    return _model_cases(FULL) + _model_cases(PARTIAL)


NCASES = 110


def label(i):
    return cases()[i][0]


def _set_key(case):
    _, kind, n, out, truth, _, _, _, _, _, _, seed = case
    return (kind, n, out, truth, seed)


def set_ids():
    """per case, the index of its point set among the distinct sets in order of first use; and the distinct keys"""
    keys, ids = [], []
    for c in cases():
        k = _set_key(c)
        if k not in keys:
            keys.append(k)
        ids.append(keys.index(k))
    return ids, keys


def inputs(i):
    """(src, dst, status or None, model, method, threshold, max_iters, confidence) of case i"""
    _, kind, n, out, truth, st, model, method, thr, iters, conf, seed = cases()[i]
    src, dst = points(kind, n, out, truth, seed)
    return src, dst, status(st, n), model, method, thr, iters, conf


def compact(src, dst, st):
    """what the reference sees: the status != 0 pairs, in order"""
    if st is None:
        return src, dst
    k = st != 0
    return np.ascontiguousarray(src[k]), np.ascontiguousarray(dst[k])


_IDS = None


def fixture_inputs(fx, i):
    """case i as recorded: (src, dst, status or None, model, method, threshold, max_iters, confidence), the points
    from the fixture"""
    global _IDS
    if _IDS is None:
        _IDS = set_ids()[0]
    _, _, n, _, _, st, model, method, thr, iters, conf, _ = cases()[i]
    k = _IDS[i]
    return fx[f"set_{k}_src"], fx[f"set_{k}_dst"], status(st, n), model, method, thr, iters, conf


def fixture_outputs(fx, i, n, refine_iters):
    """(valid, mask [n], M [2, 3] as recorded in the stored state, M in the other state) of case i over its n
    compacted pairs, for refineIters 0 or 10"""
    r = f"{i}_r{refine_iters}"
    valid = int(fx[f"{r}_valid"][0])
    mask = np.unpackbits(fx[f"{r}_mask"])[:n]
    m = fx[f"{r}_M"]
    other = fx[f"other_{r}_M"] if f"other_{r}_M" in fx.files else m
    return valid, mask, m, other
