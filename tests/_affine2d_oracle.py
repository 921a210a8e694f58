"""cv::estimateAffine2D and cv::estimateAffinePartial2D (RANSAC and LMEDS)
restated operation by operation: calib3d/src/ptsetreg.cpp:53-371 (the two
registrators), :520-680 (the estimator callbacks), :683-795 (the refine
callbacks), :821-980 (the two entry points), precomp.hpp:136-157
(haveCollinearPoints), calib3d/src/levmarq.cpp:89-196 (the LM step) with
core/src/lapack.cpp's Jacobi from tests/_homography_oracle.py.

Python floats are IEEE doubles and every operation below is one correctly
rounded operation; the float parts (the collinearity differences, the error) use
numpy float32.  No numpy.linalg.  The LM step's sums are plain in-order sums: it
is compared by what it does to points, not bit for bit (DESIGN.md §5
"estimateAffine2D").

`estimate` returns a Result; `Result.margins` holds, for every
RANSACUpdateNumIters call that rounded, the distance of num/denom from the
nearest k + 0.5 (contract B)."""
import math

import numpy as np

from _homography_oracle import DBL_EPSILON, DBL_MIN, FLT_EPSILON, MAX_REDRAWS, Rng, Result, _div, jacobi

F32 = np.float32
FULL, PARTIAL = 0, 1
RANSAC, LMEDS = 8, 4
DBL_MAX = 1.7976931348623157e308
IDENTITY = [1., 0., 0., 0., 1., 0.]


def model_points(model):
    return 2 if model == PARTIAL else 3


def have_collinear3(p):
    """precomp.hpp:136-157 with count 3: one test, points 1 and 0 against point 2"""
    dx1, dy1 = float(p[1, 0] - p[2, 0]), float(p[1, 1] - p[2, 1])
    dx2, dy2 = float(p[0, 0] - p[2, 0]), float(p[0, 1] - p[2, 1])
    return abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2))


def get_subset(src, dst, rng, count, mp, max_attempts):
    """getSubset: mp indices, or None.  checkSubset never fires for two points."""
    for _ in range(max_attempts):
        idx = []
        for i in range(mp):
            for _r in range(MAX_REDRAWS):
                v = rng.draw(count)
                if v not in idx:
                    break
            else:
                break
            idx.append(v)
        if len(idx) != mp:
            continue
        if mp == 3 and (have_collinear3(src[idx]) or have_collinear3(dst[idx])):
            continue
        return idx
    return None


def _mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def solve_full(f, t):
    """Affine2DEstimatorCallback::runKernel on float32 [3, 2] arrays: six doubles"""
    (x1, y1), (x2, y2), (x3, y3) = f.tolist()
    (X1, Y1), (X2, Y2), (X3, Y3) = t.tolist()
    d = _div(1., x1 * (y2 - y3) + x2 * (y3 - y1) + x3 * (y1 - y2))
    return [_mul(d, X1 * (y2 - y3) + X2 * (y3 - y1) + X3 * (y1 - y2)),
            _mul(d, X1 * (x3 - x2) + X2 * (x1 - x3) + X3 * (x2 - x1)),
            _mul(d, X1 * (x2 * y3 - x3 * y2) + X2 * (x3 * y1 - x1 * y3) + X3 * (x1 * y2 - x2 * y1)),
            _mul(d, Y1 * (y2 - y3) + Y2 * (y3 - y1) + Y3 * (y1 - y2)),
            _mul(d, Y1 * (x3 - x2) + Y2 * (x1 - x3) + Y3 * (x2 - x1)),
            _mul(d, Y1 * (x2 * y3 - x3 * y2) + Y2 * (x3 * y1 - x1 * y3) + Y3 * (x1 * y2 - x2 * y1))]


def solve_partial(f, t):
    """AffinePartial2DEstimatorCallback::runKernel on float32 [2, 2] arrays"""
    (x1, y1), (x2, y2) = f.tolist()[:2]
    (X1, Y1), (X2, Y2) = t.tolist()[:2]
    d = _div(1., (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2))
    S0 = _mul(d, (X1 - X2) * (x1 - x2) + (Y1 - Y2) * (y1 - y2))
    S1 = _mul(d, (Y1 - Y2) * (x1 - x2) - (X1 - X2) * (y1 - y2))
    S2 = _mul(d, (Y1 - Y2) * (x1 * y2 - x2 * y1) - (X1 * y2 - X2 * y1) * (y1 - y2) - (X1 * x2 - X2 * x1) * (x1 - x2))
    S3 = _mul(d, -(X1 - X2) * (x1 * y2 - x2 * y1) - (Y1 * x2 - Y2 * x1) * (x1 - x2) - (Y1 * y2 - Y2 * y1) * (y1 - y2))
    return [S0, -S1, S2, S1, S0, S3]


def run_kernel(f, t, mp):
    return solve_full(f, t) if mp == 3 else solve_partial(f, t)


def errors(src, dst, M):
    """computeError: float32 [n], the model converted to float first"""
    with np.errstate(all="ignore"):
        F = np.array(M, np.float64).astype(F32)
        a = F[0] * src[:, 0] + F[1] * src[:, 1] + F[2] - dst[:, 0]
        b = F[3] * src[:, 0] + F[4] * src[:, 1] + F[5] - dst[:, 1]
        return a * a + b * b


def update_niters(p, ep, mp, niters, margins):
    """RANSACUpdateNumIters(p, ep, mp, niters)"""
    p = min(max(p, 0.), 1.)
    ep = min(max(ep, 0.), 1.)
    num = max(1. - p, DBL_MIN)
    denom = 1. - math.pow(1. - ep, mp)
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= niters * (-denom):
        return niters
    q = num / denom
    margins.append(abs(q - math.floor(q) - 0.5))
    return int(round(q))  # cvRound: ties to even


def rank_element(err, k):
    """what std::nth_element leaves at position k when it orders the errors as ints (ptsetreg.cpp:340)"""
    return np.sort(err.view(np.int32))[k:k + 1].view(F32)[0]


# ---- the LM step ----

def lm_compute(M, m, h, jac, n):
    r, J = [], []
    for (Mx, My), (mx, my) in zip(M, m):
        if n == 6:
            xi = h[0] * Mx + h[1] * My + h[2]
            yi = h[3] * Mx + h[4] * My + h[5]
        else:
            xi = h[0] * Mx - h[1] * My + h[2]
            yi = h[1] * Mx + h[0] * My + h[3]
        r.append(xi - mx)
        r.append(yi - my)
        if jac:
            if n == 6:
                J.append([Mx, My, 1., 0., 0., 0.])
                J.append([0., 0., 0., Mx, My, 1.])
            else:
                J.append([Mx, -My, 1., 0.])
                J.append([My, Mx, 0., 1.])
    return r, J


def _normal(J, r, n):
    A = [[0.0] * n for _ in range(n)]
    v = [0.0] * n
    for row, ri in zip(J, r):
        for a in range(n):
            if row[a] == 0.0:
                continue
            v[a] += row[a] * ri
            for b in range(a, n):
                A[a][b] += row[a] * row[b]
    for a in range(n):
        for b in range(a):
            A[a][b] = A[b][a]
    return A, v


def _eig(A, n):
    W, V = jacobi([row[:] for row in A], n)
    thr = 0.0
    for w in W:
        thr += w
    return W, V, thr * DBL_EPSILON * 2


def _eig_solve(A, b, n):
    W, V, thr = _eig(A, n)
    x = [0.0] * n
    for i in range(n):
        if abs(W[i]) <= thr:
            continue
        s = 0.0
        for j in range(n):
            s += V[i][j] * b[j]
        s *= 1 / W[i]
        for j in range(n):
            x[j] = x[j] + s * V[i][j]
    return x


def _eig_inv_diag_max(A, n):
    W, V, thr = _eig(A, n)
    mx = DBL_EPSILON
    for j in range(n):
        d = 0.0
        for i in range(n):
            if abs(W[i]) <= thr:
                continue
            d += V[i][j] * (V[i][j] * (1 / W[i]))
        mx = max(mx, abs(d))
    return mx


def lm_refine(M, m, x, max_iters):
    """createLMSolver(cb, max_iters)->run(x), x of 6 or 4 parameters"""
    n = len(x)
    Ml, ml = M.tolist(), m.tolist()
    x = list(x)
    r, J = lm_compute(Ml, ml, x, True, n)
    S = sum(v * v for v in r)
    A, v = _normal(J, r, n)
    D = [A[i][i] for i in range(n)]
    lam, lc, it = 1.0, 0.75, 0
    while True:
        Ap = [row[:] for row in A]
        for i in range(n):
            Ap[i][i] += lam * D[i]
        d = _eig_solve(Ap, v, n)
        xd = [x[i] - d[i] for i in range(n)]
        rd, _ = lm_compute(Ml, ml, xd, False, n)
        Sd = sum(q * q for q in rd)
        temp = [-sum(A[i][j] * d[j] for j in range(n)) + 2 * v[i] for i in range(n)]
        dS = sum(d[i] * temp[i] for i in range(n))
        R = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1)
        if R > 0.75:
            lam *= 0.5
            if lam < lc:
                lam = 0
        elif R < 0.25:
            t = sum(d[i] * v[i] for i in range(n))
            nu = (Sd - S) / (t if abs(t) > DBL_EPSILON else 1) + 2
            nu = min(max(nu, 2.), 10.)
            if lam == 0:
                lam = lc = 1. / _eig_inv_diag_max(A, n)
                nu *= 0.5
            lam *= nu
        if Sd < S:
            S, x = Sd, xd
            r, J = lm_compute(Ml, ml, x, True, n)
            A, v = _normal(J, r, n)
        it += 1
        if not (it < max_iters and max(abs(q) for q in d) >= FLT_EPSILON and max(abs(q) for q in r) >= FLT_EPSILON):
            break
    return x


def estimate(src, dst, model=FULL, method=RANSAC, thr=3.0, max_iters=2000, confidence=0.99, refine_iters=10):
    """src, dst: float32 [n, 2], the status != 0 pairs.  Result: valid, M (6 doubles, the identity when not valid),
    M0 (M before the LM step), mask (uint8 [n]), ninliers, iters, subsets (the accepted subsets of the iterations the
    loop ran), hyps (their M), margins."""
    res = Result()
    n, mp = len(src), model_points(model)
    res.valid, res.mask, res.ninliers, res.iters = 0, np.zeros(n, np.uint8), 0, 0
    res.subsets, res.hyps, res.margins = [], [], []
    res.M = res.M0 = list(IDENTITY)
    if n < mp:
        return res
    if n == mp:
        M = run_kernel(src, dst, mp)
        mask = np.ones(n, np.uint8)
    elif method == RANSAC:
        rng = Rng()
        niters, it, max_good, best_mask, M = max(max_iters, 1), 0, 0, None, None
        t = F32(thr * thr)
        while it < niters:
            idx = get_subset(src, dst, rng, n, mp, 10000)
            if idx is None:
                break
            res.subsets.append(idx)
            model_i = run_kernel(src[idx], dst[idx], mp)
            res.hyps.append(model_i)
            with np.errstate(invalid="ignore"):
                good_mask = errors(src, dst, model_i) <= t
            good = int(good_mask.sum())
            if good > max(max_good, mp - 1):
                best_mask, M, max_good = good_mask, model_i, good
                niters = update_niters(confidence, (n - good) / n, mp, niters, res.margins)
            it += 1
        res.iters = it
        if max_good == 0:
            return res
        mask = best_mask.astype(np.uint8)
    else:
        rng = Rng()
        niters = max(update_niters(confidence, 0.45, mp, max_iters, res.margins), 3)
        min_median, M, it = DBL_MAX, None, 0
        while it < niters:
            idx = get_subset(src, dst, rng, n, mp, 1000)
            if idx is None:
                break
            res.subsets.append(idx)
            model_i = run_kernel(src[idx], dst[idx], mp)
            res.hyps.append(model_i)
            median = float(rank_element(errors(src, dst, model_i), n // 2))
            if median < min_median:
                min_median, M = median, model_i
            it += 1
        res.iters = it
        if not min_median < DBL_MAX:
            return res
        sigma = max(2.5 * 1.4826 * (1 + 5. / (n - mp)) * math.sqrt(min_median), 0.001)
        with np.errstate(invalid="ignore"):
            mask = (errors(src, dst, M) <= F32(sigma * sigma)).astype(np.uint8)
        if int(mask.sum()) < mp:
            return res
    M0 = M
    if n > mp and refine_iters:
        k = mask != 0
        s, d = np.ascontiguousarray(src[k]), np.ascontiguousarray(dst[k])
        if len(s) > 0:
            if mp == 3:
                M = lm_refine(s, d, M, refine_iters)
            else:
                h = lm_refine(s, d, [M[0], M[3], M[2], M[5]], refine_iters)
                M = [h[0], -h[1], h[2], h[1], h[0], h[3]]
    res.valid, res.mask, res.ninliers, res.M, res.M0 = 1, mask, int(mask.sum()), M, M0
    return res


def transfer(M, pts):
    """the images of float32 [n, 2] points under the 2x3 M, in double"""
    M = np.asarray(M, np.float64).reshape(2, 3)
    p = pts.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([M[0, 0] * p[:, 0] + M[0, 1] * p[:, 1] + M[0, 2],
                         M[1, 0] * p[:, 0] + M[1, 1] * p[:, 1] + M[1, 2]], 1)


def distance(M1, M2, pts):
    """contract C: the largest displacement, in pixels, between the images of `pts` under the two matrices"""
    if len(pts) == 0:
        return 0.0
    d = transfer(M1, pts) - transfer(M2, pts)
    return float(np.sqrt((d * d).sum(1)).max())


def same_bits(a, b):
    """two matrices equal word for word, any NaN equal to any NaN (its sign differs between platforms)"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))


FIXTURE = None
_TABLE = {}


def fixture():
    """tests/golden/reference_affine2d.npz, loaded once"""
    global FIXTURE
    if FIXTURE is None:
        import os

        FIXTURE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_affine2d.npz"))
    return FIXTURE


def table_result(i, refine_iters=10):
    """estimate on case i of tests/_affine2d_cases.py (the fixture's points, status applied), computed once per
    process and shared by the tests: the result must not be changed"""
    import _affine2d_cases as AC

    if (i, refine_iters) not in _TABLE:
        src, dst, st, model, method, thr, iters, conf = AC.fixture_inputs(fixture(), i)
        s, d = AC.compact(src, dst, st)
        _TABLE[(i, refine_iters)] = estimate(s, d, model, method, thr, iters, conf, refine_iters)
    return _TABLE[(i, refine_iters)]


def hyps_hash(hyps):
    """FNV-1a 64 over the bits of every hypothesis' M, NaN entries as the word 0x7ff8000000000000
    (affine2d_core_check.cpp)"""
    h = 14695981039346656037
    for m in hyps:
        a = np.array(m, np.float64)
        w = a.view(np.uint64).copy()
        w[np.isnan(a)] = 0x7ff8000000000000
        for b in w.tobytes():
            h = ((h ^ b) * 1099511628211) & ((1 << 64) - 1)
    return h
