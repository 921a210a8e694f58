"""cv::findHomography (method 0 and RANSAC) restated operation by operation:
calib3d/src/fundam.cpp:62-433 (the estimator callback, the refine callback and
the dispatch), calib3d/src/ptsetreg.cpp:53-252 (RANSAC), core/src/lapack.cpp:96-260
(the Jacobi eigen solver), core/src/matmul.simd.hpp's 3x3 branch, unfused (the
noavx2 dispatch state), calib3d/src/levmarq.cpp:89-196 (the LM step).

Python floats are IEEE doubles and every operation below is one correctly
rounded operation, so the doubles round as the reference's do; the float parts
(the collinearity differences, the reprojection error) use numpy float32.  No
numpy.linalg.  The LM step's sums are plain in-order sums: it is compared by
what it does to points, not bit for bit (DESIGN.md §5 "findHomography").

`find_homography` returns a Result; `Result.margins` holds, for every niters
update, the distance of num/denom from the nearest k + 0.5 (contract B)."""
import math

import numpy as np

F32 = np.float32
FLT_EPSILON = 1.1920928955078125e-07
DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
LSQ, RANSAC = 0, 8
MAX_ATTEMPTS = 10000
MAX_REDRAWS = 256  # the library's bound on redraws of one slot (never reached: DESIGN.md)


class Rng:
    """cv::RNG((uint64)-1); uniform(0, n) = (unsigned)next() % n (core/operations.hpp:383-393)"""

    def __init__(self):
        self.state = (1 << 64) - 1

    def draw(self, n):
        s = self.state
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) & ((1 << 64) - 1)
        self.state = s
        return (s & 0xFFFFFFFF) % n


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def have_collinear(p):
    """precomp.hpp:136-157 on four float32 points [4, 2]: the differences are float, the rest double"""
    i = 3
    for j in range(i):
        dx1, dy1 = float(p[j, 0] - p[i, 0]), float(p[j, 1] - p[i, 1])
        for k in range(j):
            dx2, dy2 = float(p[k, 0] - p[i, 0]), float(p[k, 1] - p[i, 1])
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def _det3(p, t):
    a = [[float(p[k, 0]), float(p[k, 1]), 1.0] for k in t]
    return (a[0][0] * (a[1][1] * a[2][2] - a[2][1] * a[1][2]) - a[0][1] * (a[1][0] * a[2][2] - a[2][0] * a[1][2])
            + a[0][2] * (a[1][0] * a[2][1] - a[2][0] * a[1][1]))


def check_subset(s, d):
    if have_collinear(s) or have_collinear(d):
        return False
    negative = 0
    for t in ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)):
        negative += _det3(s, t) * _det3(d, t) < 0
    return negative in (0, 4)


def _hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b /= a
        return a * math.sqrt(1 + b * b)
    if b > 0:
        a /= b
        return b * math.sqrt(1 + a * a)
    return 0.0


def jacobi(A, n):
    """JacobiImpl_<double>: A is n x n (lists; the upper triangle is read and changed).  Returns (W, V), the
    eigenvalues in descending order and the eigenvectors as rows."""
    eps = DBL_EPSILON
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    W = [0.0] * n
    indR, indC = [0] * n, [0] * n
    for k in range(n):
        W[k] = A[k][k]
        if k < n - 1:
            m, mv = k + 1, abs(A[k][k + 1])
            for i in range(k + 2, n):
                val = abs(A[k][i])
                if mv < val:
                    mv, m = val, i
            indR[k] = m
        if k > 0:
            m, mv = 0, abs(A[0][k])
            for i in range(1, k):
                val = abs(A[i][k])
                if mv < val:
                    mv, m = val, i
            indC[k] = m
    if n > 1:
        for _ in range(n * n * 30):
            k, mv = 0, abs(A[0][indR[0]])
            for i in range(1, n - 1):
                val = abs(A[i][indR[i]])
                if mv < val:
                    mv, k = val, i
            l = indR[k]
            for i in range(1, n):
                val = abs(A[indC[i]][i])
                if mv < val:
                    mv, k, l = val, indC[i], i
            p = A[k][l]
            if abs(p) <= eps:
                break
            y = (W[l] - W[k]) * 0.5
            t = abs(y) + _hypot(p, y)
            s = _hypot(p, t)
            c = _div(t, s)
            s = _div(p, s)
            t = _div(p, t) * p
            if y < 0:
                s, t = -s, -t
            A[k][l] = 0.0
            W[k] -= t
            W[l] += t
            for i in range(k):
                a0, b0 = A[i][k], A[i][l]
                A[i][k], A[i][l] = a0 * c - b0 * s, a0 * s + b0 * c
            for i in range(k + 1, l):
                a0, b0 = A[k][i], A[i][l]
                A[k][i], A[i][l] = a0 * c - b0 * s, a0 * s + b0 * c
            for i in range(l + 1, n):
                a0, b0 = A[k][i], A[l][i]
                A[k][i], A[l][i] = a0 * c - b0 * s, a0 * s + b0 * c
            Vk, Vl = V[k], V[l]
            for i in range(n):
                a0, b0 = Vk[i], Vl[i]
                Vk[i], Vl[i] = a0 * c - b0 * s, a0 * s + b0 * c
            for idx in (k, l):
                if idx < n - 1:
                    m, mv = idx + 1, abs(A[idx][idx + 1])
                    for i in range(idx + 2, n):
                        val = abs(A[idx][i])
                        if mv < val:
                            mv, m = val, i
                    indR[idx] = m
                if idx > 0:
                    m, mv = 0, abs(A[0][idx])
                    for i in range(1, idx):
                        val = abs(A[i][idx])
                        if mv < val:
                            mv, m = val, i
                    indC[idx] = m
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return W, V


def _mul3(a, b):
    """gemm's 3x3 branch, alpha 1, beta 0 on a zero C: (a0*b0 + a1*b1 + a2*b2)*1 + 0*0, unfused"""
    d = [0.0] * 9
    for i in range(3):
        for j in range(3):
            t = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j]
            d[3 * i + j] = t * 1.0 + 0.0 * 0.0
    return d


def run_kernel(M, m):
    """HomographyEstimatorCallback::runKernel on float32 [n, 2] arrays: H as 9 doubles, or None (it returned 0)"""
    count = len(M)
    Ml, ml = M.tolist(), m.tolist()  # float32 -> double, exact
    cmx = cmy = cMx = cMy = 0.0
    for i in range(count):
        cmx += ml[i][0]
        cmy += ml[i][1]
        cMx += Ml[i][0]
        cMy += Ml[i][1]
    cmx /= count
    cmy /= count
    cMx /= count
    cMy /= count
    smx = smy = sMx = sMy = 0.0
    for i in range(count):
        smx += abs(ml[i][0] - cmx)
        smy += abs(ml[i][1] - cmy)
        sMx += abs(Ml[i][0] - cMx)
        sMy += abs(Ml[i][1] - cMy)
    if abs(smx) < DBL_EPSILON or abs(smy) < DBL_EPSILON or abs(sMx) < DBL_EPSILON or abs(sMy) < DBL_EPSILON:
        return None
    smx, smy, sMx, sMy = count / smx, count / smy, count / sMx, count / sMy
    inv_hnorm = [1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1]
    hnorm2 = [sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1]
    L = [[0.0] * 9 for _ in range(9)]
    for i in range(count):
        x, y = (ml[i][0] - cmx) * smx, (ml[i][1] - cmy) * smy
        X, Y = (Ml[i][0] - cMx) * sMx, (Ml[i][1] - cMy) * sMy
        Lx = [X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x]
        Ly = [0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y]
        for j in range(9):
            Lj = L[j]
            for k in range(j, 9):
                Lj[k] += Lx[j] * Lx[k] + Ly[j] * Ly[k]
    _, V = jacobi(L, 9)
    h0 = _mul3(_mul3(inv_hnorm, V[8]), hnorm2)
    s = _div(1.0, h0[8])
    with np.errstate(all="ignore"):
        return [float(np.float64(v) * np.float64(s) + 0.0) for v in h0]


def errors(M, m, H):
    """computeError: float32 [n]"""
    with np.errstate(all="ignore"):
        Hf = np.array(H[:8], np.float64).astype(F32)
        Mx, My = M[:, 0], M[:, 1]
        ww = F32(1) / (Hf[6] * Mx + Hf[7] * My + F32(1))
        dx = (Hf[0] * Mx + Hf[1] * My + Hf[2]) * ww - m[:, 0]
        dy = (Hf[3] * Mx + Hf[4] * My + Hf[5]) * ww - m[:, 1]
        return dx * dx + dy * dy


def update_niters(p, ep, niters, margins):
    """RANSACUpdateNumIters(p, ep, 4, niters)"""
    p = min(max(p, 0.), 1.)
    ep = min(max(ep, 0.), 1.)
    num = max(1. - p, DBL_MIN)
    denom = 1. - math.pow(1. - ep, 4)
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= niters * (-denom):
        return niters
    q = num / denom
    margins.append(abs(q - math.floor(q) - 0.5))
    return int(round(q))  # cvRound: ties to even


class Result:
    pass


def get_subset(M, m, rng, count):
    """getSubset(..., maxAttempts = 10000): four indices, or None"""
    for _ in range(MAX_ATTEMPTS):
        idx = []
        for i in range(4):
            for _r in range(MAX_REDRAWS):
                v = rng.draw(count)
                if v not in idx:
                    break
            else:
                break
            idx.append(v)
        if len(idx) == 4 and check_subset(M[idx], m[idx]):
            return idx
    return None


def lm_compute(M, m, h, jac):
    """HomographyRefineCallback::compute: r [2n] and J [2n][8] as lists"""
    r, J = [], []
    for (Mx, My), (mx, my) in zip(M, m):
        ww = h[6] * Mx + h[7] * My + 1.
        ww = 1. / ww if abs(ww) > DBL_EPSILON else 0.
        xi = (h[0] * Mx + h[1] * My + h[2]) * ww
        yi = (h[3] * Mx + h[4] * My + h[5]) * ww
        r.append(xi - mx)
        r.append(yi - my)
        if jac:
            J.append([Mx * ww, My * ww, ww, 0., 0., 0., -Mx * ww * xi, -My * ww * xi])
            J.append([0., 0., 0., Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi])
    return r, J


def _normal(J, r):
    A = [[0.0] * 8 for _ in range(8)]
    v = [0.0] * 8
    for row, ri in zip(J, r):
        for a in range(8):
            if row[a] == 0.0:
                continue
            v[a] += row[a] * ri
            for b in range(a, 8):
                A[a][b] += row[a] * row[b]
    for a in range(8):
        for b in range(a):
            A[a][b] = A[b][a]
    return A, v


def _eig_solve(A, b):
    """solve(A, b, DECOMP_EIG): Jacobi, then SVBkSb with eps = 2 DBL_EPSILON"""
    W, V = jacobi([row[:] for row in A], 8)
    thr = 0.0
    for w in W:
        thr += w
    thr *= DBL_EPSILON * 2
    x = [0.0] * 8
    for i in range(8):
        if abs(W[i]) <= thr:
            continue
        s = 0.0
        for j in range(8):
            s += V[i][j] * b[j]
        s *= 1 / W[i]
        for j in range(8):
            x[j] = x[j] + s * V[i][j]
    return x


def _eig_inv_diag_max(A):
    """max(DBL_EPSILON, max |diag(invert(A, DECOMP_EIG))|)"""
    W, V = jacobi([row[:] for row in A], 8)
    thr = 0.0
    for w in W:
        thr += w
    thr *= DBL_EPSILON * 2
    mx = DBL_EPSILON
    for j in range(8):
        d = 0.0
        for i in range(8):
            if abs(W[i]) <= thr:
                continue
            d += V[i][j] * (V[i][j] * (1 / W[i]))
        mx = max(mx, abs(d))
    return mx


def lm_refine(M, m, H):
    """createLMSolver(cb, 10)->run(H8): the first eight entries refined, H[8] kept"""
    Ml, ml = M.tolist(), m.tolist()
    x = list(H[:8])
    r, J = lm_compute(Ml, ml, x, True)
    S = sum(v * v for v in r)
    A, v = _normal(J, r)
    D = [A[i][i] for i in range(8)]
    lam, lc, it = 1.0, 0.75, 0
    while True:
        Ap = [row[:] for row in A]
        for i in range(8):
            Ap[i][i] += lam * D[i]
        d = _eig_solve(Ap, v)
        xd = [x[i] - d[i] for i in range(8)]
        rd, _ = lm_compute(Ml, ml, xd, False)
        Sd = sum(q * q for q in rd)
        temp = [-sum(A[i][j] * d[j] for j in range(8)) + 2 * v[i] for i in range(8)]
        dS = sum(d[i] * temp[i] for i in range(8))
        R = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1)
        if R > 0.75:
            lam *= 0.5
            if lam < lc:
                lam = 0
        elif R < 0.25:
            t = sum(d[i] * v[i] for i in range(8))
            nu = (Sd - S) / (t if abs(t) > DBL_EPSILON else 1) + 2
            nu = min(max(nu, 2.), 10.)
            if lam == 0:
                lam = lc = 1. / _eig_inv_diag_max(A)
                nu *= 0.5
            lam *= nu
        if Sd < S:
            S, x = Sd, xd
            r, J = lm_compute(Ml, ml, x, True)
            A, v = _normal(J, r)
        it += 1
        if not (it < 10 and max(abs(q) for q in d) >= FLT_EPSILON and max(abs(q) for q in r) >= FLT_EPSILON):
            break
    return x + [H[8]]


def find_homography(src, dst, method=RANSAC, thr=3.0, max_iters=2000, confidence=0.995, refine=True):
    """src, dst: float32 [n, 2], the status != 0 pairs.  Result: valid, H (9 doubles, the identity when not valid),
    H0 (H before the LM step), mask (uint8 [n]), ninliers, iters, subsets (the accepted 4-point subsets of the
    iterations the loop ran), hyps (their H, None where runKernel returned 0), margins."""
    res = Result()
    n = len(src)
    res.valid, res.mask, res.ninliers, res.iters = 0, np.zeros(n, np.uint8), 0, 0
    res.subsets, res.hyps, res.margins = [], [], []
    res.H = res.H0 = [1., 0., 0., 0., 1., 0., 0., 0., 1.]
    if thr <= 0:
        thr = 3.0
    H = None
    if n < 4:  # the library's rule for method 0 too (the reference returns a meaningless matrix there)
        return res
    if method == LSQ or n == 4:
        H = run_kernel(src, dst)
        if H is None:
            return res
        mask = np.ones(n, np.uint8)
    else:
        rng = Rng()
        niters, it, max_good, best_mask = max(max_iters, 1), 0, 0, None
        t = F32(thr * thr)
        while it < niters:
            idx = get_subset(src, dst, rng, n)
            if idx is None:
                if it == 0:
                    return res
                break
            res.subsets.append(idx)
            model = run_kernel(src[idx], dst[idx])
            res.hyps.append(model)
            if model is not None:
                good_mask = errors(src, dst, model) <= t
                good = int(good_mask.sum())
                if good > max(max_good, 3):
                    best_mask, H, max_good = good_mask, model, good
                    niters = update_niters(confidence, (n - good) / n, niters, res.margins)
            it += 1
        res.iters = it
        if max_good == 0:
            return res
        mask = best_mask.astype(np.uint8)
    H0 = H
    if n > 4:
        k = mask != 0
        s, d = np.ascontiguousarray(src[k]), np.ascontiguousarray(dst[k])
        if len(s) > 0:
            if method == RANSAC:
                H1 = run_kernel(s, d)
                if H1 is not None:
                    H = H1
            H0 = H
            if refine:
                H = lm_refine(s, d, H)
    res.valid, res.mask, res.ninliers, res.H, res.H0 = 1, mask, int(mask.sum()), H, H0
    return res


def transfer(H, pts):
    """the images of float32 [n, 2] points under H, in double"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = pts.astype(np.float64)
    with np.errstate(all="ignore"):
        w = H[2, 0] * p[:, 0] + H[2, 1] * p[:, 1] + H[2, 2]
        return np.stack([(H[0, 0] * p[:, 0] + H[0, 1] * p[:, 1] + H[0, 2]) / w,
                         (H[1, 0] * p[:, 0] + H[1, 1] * p[:, 1] + H[1, 2]) / w], 1)


def distance(H1, H2, pts):
    """contract C: the largest displacement, in pixels, between the images of `pts` under the two matrices"""
    if len(pts) == 0:
        return 0.0
    d = transfer(H1, pts) - transfer(H2, pts)
    return float(np.sqrt((d * d).sum(1)).max())


FIXTURE = None
_TABLE = {}


def fixture():
    """tests/golden/reference_homography.npz, loaded once"""
    global FIXTURE
    if FIXTURE is None:
        import os

        FIXTURE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_homography.npz"))
    return FIXTURE


def table_result(i, refine=True):
    """find_homography on case i of tests/_homography_cases.py (the fixture's points, status applied), computed once
    per process and shared by the tests: the result must not be changed"""
    import _homography_cases as HC

    if (i, refine) not in _TABLE:
        src, dst, st, method, thr, iters, conf = HC.fixture_inputs(fixture(), i)
        s, d = HC.compact(src, dst, st)
        _TABLE[(i, refine)] = find_homography(s, d, method, thr, iters, conf, refine)
    return _TABLE[(i, refine)]


def hyps_hash(hyps):
    """FNV-1a 64 over the bits of every hypothesis' H, a zero word for a failed one (homography_core_check.cpp)"""
    h = 14695981039346656037
    for m in hyps:
        for b in (np.asarray(m, np.float64).tobytes() if m is not None else bytes(8)):
            h = ((h ^ b) * 1099511628211) & ((1 << 64) - 1)
    return h
