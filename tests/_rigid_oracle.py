"""_rigid_oracle.py — restatement of the point-set branch of
cv::estimateRigidTransform(A, B, fullAffine=false, ransacMaxIters,
ransacGoodRatio, ransacSize0=3) (modules/video/src/lkpyramid.cpp:1479-1693).
TEST INFRASTRUCTURE ONLY.

The RANSAC is deterministic: cv::RNG is constructed with state (uint64)-1 on
every call (core/operations.hpp:383-393).  The draws, the redraw rules, the
abandon rule, the inlier threshold from boundingRect(pB)
(imgproc/src/shapedescr.cpp:898-907) and the inlier test's operation order are
the reference's; getRTMatrix is oracle/box_fit_oracle.py's (numpy eigen solve,
equal to the reference's Jacobi solve to double rounding).

Besides the result, estimate() reports how far the decisions were from their
thresholds, so a test can assert that a comparison against another
implementation of the same arithmetic is well posed:
  resid_margin  : min over every evaluated hypothesis and point of
                  |residual - thr| (px)
  collin_margin : min over every evaluated collinearity comparison of
                  |lhs - rhs| / max(lhs, rhs)"""
import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import box_fit_oracle as BF  # noqa: E402

FLT_EPSILON = np.float32(1.1920929e-07)
_f32 = np.float32


class RNG:
    """cv::RNG (multiply-with-carry), core/operations.hpp:383-393"""

    def __init__(self, state: int = 0xFFFFFFFFFFFFFFFF):
        self.state = state

    def next(self) -> int:
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a: int, b: int) -> int:
        return a if a == b else self.next() % (b - a) + a


@dataclass
class Rigid:
    M: np.ndarray | None          # 2x3, None: no transform
    k: int                        # round that reached consensus, -1: none
    inliers: np.ndarray           # bool per point (all False without a transform)
    resid_margin: float
    collin_margin: float
    rounds: int                   # hypotheses evaluated

    @property
    def found(self) -> bool:
        return self.M is not None


def closed_form(a, b) -> np.ndarray:
    """getRTMatrix with the normal system solved in closed form (the kernel's
    box_fit.hpp::solve) instead of the eigen solve"""
    sa, sb = BF.rt_sums(a, b)
    s00, s02, s03, n = sa[0, 0], sa[0, 2], sa[0, 3], sa[2, 2]
    den = s00 - (s02 * s02 + s03 * s03) / n
    if not den > 1e-9:
        return np.array([[1.0, -0.0, 0.0], [0.0, 1.0, 0.0]])
    p = (sb[0] - (s02 * sb[2] + s03 * sb[3]) / n) / den
    q = (sb[1] + (s03 * sb[2] - s02 * sb[3]) / n) / den
    tx = (sb[2] - s02 * p + s03 * q) / n
    ty = (sb[3] - s03 * p - s02 * q) / n
    return np.array([[p, -q, tx], [q, p, ty]])


def _close(P, i, j) -> bool:
    # fabs(float) + fabs(float) < FLT_EPSILON in float (:1618-1623); the double
    # difference of two floats is exact, so rounding it once is the float result
    dx = _f32(abs(P[i][0] - P[j][0]))
    dy = _f32(abs(P[i][1] - P[j][1]))
    return bool(_f32(dx + dy) < FLT_EPSILON)


def _collinear(p0, p1, p2):
    """:1640-1648 for one point set -> (rejected, relative margin)"""
    dx1, dy1 = p1[0] - p0[0], p1[1] - p0[1]   # float differences promoted to double; exact in double
    dx2, dy2 = p2[0] - p0[0], p2[1] - p0[1]
    dx1, dy1, dx2, dy2 = (float(_f32(v)) for v in (dx1, dy1, dx2, dy2))
    lhs = abs(dx1 * dy2 - dy1 * dx2)
    rhs = 0.01 * np.sqrt(dx1 * dx1 + dy1 * dy1) * np.sqrt(dx2 * dx2 + dy2 * dy2)
    big = max(lhs, rhs)
    return lhs < rhs, (abs(lhs - rhs) / big if big > 0 else np.inf)


def bounding_rect(b: np.ndarray):
    lo = np.floor(b.min(0)).astype(np.int64)
    hi = np.floor(b.max(0)).astype(np.int64)
    return int(lo[0]), int(lo[1]), int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)


def estimate(a, b, max_iters: int = 500, good_ratio: float = 0.5, solve=BF.get_rt_matrix) -> Rigid:
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(b, np.float32).reshape(-1, 2)
    count = len(a)
    none = Rigid(None, -1, np.zeros(count, bool), np.inf, np.inf, 0)
    if count < 3:  # count == 0 throws in the reference (checkVector): recorded as no transform
        return none
    _, _, bw, bh = bounding_rect(b)
    thr = max(bw, bh) * 0.05
    A = a.astype(np.float64).tolist()  # exact values of the floats, as Python floats
    B = b.astype(np.float64).tolist()
    ax, ay = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)
    bx, by = b[:, 0].astype(np.float64), b[:, 1].astype(np.float64)
    rng = RNG()
    resid_margin = collin_margin = np.inf
    rounds = 0
    for k in range(max_iters):
        idx = [0, 0, 0]
        i = 0
        while i < 3:
            k1 = 0
            while k1 < max_iters:
                idx[i] = rng.uniform(0, count)
                rejected = False
                for j in range(i):
                    if idx[j] == idx[i] or _close(A, idx[i], idx[j]) or _close(B, idx[i], idx[j]):
                        rejected = True
                        break
                if not rejected and i == 2:
                    rej, mg = _collinear(A[idx[0]], A[idx[1]], A[idx[2]])
                    collin_margin = min(collin_margin, mg)
                    if not rej:  # || short-circuits: the second set is compared only now
                        rej, mg = _collinear(B[idx[0]], B[idx[1]], B[idx[2]])
                        collin_margin = min(collin_margin, mg)
                    rejected = rej
                if not rejected:
                    break
                k1 += 1
            if k1 >= max_iters:
                break
            i += 1
        if i < 3:
            continue
        m = solve(a[idx], b[idx])
        # :1666-1667, in double, one rounding per operation
        res = np.abs(m[0, 0] * ax + m[0, 1] * ay + m[0, 2] - bx) + np.abs(m[1, 0] * ax + m[1, 1] * ay + m[1, 2] - by)
        good = res < thr
        rounds += 1
        resid_margin = min(resid_margin, float(np.abs(res - thr).min()))
        if good.sum() >= count * good_ratio:
            return Rigid(BF.get_rt_matrix(a[good], b[good]) if solve is BF.get_rt_matrix else solve(a[good], b[good]),
                         k, good, resid_margin, collin_margin, rounds)
    none.resid_margin, none.collin_margin, none.rounds = resid_margin, collin_margin, rounds
    return none


def tolerance(a, b, M) -> np.ndarray:
    """the project's fit tolerance (tests/test_gpu_box_fit.py): 64 eps cond(A) max(1, |M|)"""
    sa, _ = BF.rt_sums(a, b)
    return 64 * np.finfo(np.float64).eps * np.linalg.cond(sa) * np.maximum(1.0, np.abs(M))
