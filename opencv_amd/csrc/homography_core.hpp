// homography_core.hpp — the arithmetic of cv::findHomography (method 0 and
// RANSAC), as __host__ __device__ functions: the subset check
// (calib3d/src/fundam.cpp:65-100, precomp.hpp:136-157), the normalised DLT
// (runKernel, :116-181) with the Jacobi eigen solver it calls
// (core/src/lapack.cpp:96-260) and the two 3x3 products in gemm's order, the
// float reprojection error (:191-210), RANSACUpdateNumIters
// (ptsetreg.cpp:53-73) and the LM refinement (fundam.cpp:223-266,
// levmarq.cpp:89-196).  homography.hip's kernels call them; so does the
// stand-alone host check (tests/cpp/homography_core_check.cpp), which is why
// this file includes nothing of HIP and compiles with a plain C++ compiler.
//
// Every double operation is written once, in the reference's order, and the
// build does not contract (-ffp-contract=off), so the host and the device round
// alike.  Storage is reached through small accessors: a solver's matrices live
// wherever the caller puts them (an array on the host, a lane's column of LDS
// on the device), and nothing here indexes a local array with a run-time index.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ransac_rng.hpp"

namespace tbdk {
namespace homography_core {

struct Pt {
    float x, y;
};

constexpr int kMaxAttempts = 10000;  // getSubset's maxAttempts as RANSAC calls it
constexpr int kMaxRedraws = 256;     // redraws of one slot; the reference has no bound
constexpr int kLmIters = 10;

// ---- a solver's workspace: the upper triangle of A (n(n+1)/2 <= 45), V (n*n <= 81), W (n <= 9) ----
constexpr int kWsV = 45, kWsW = 126, kWsDoubles = 135;

struct Ws {
    double* base;
    int stride;
    TBDK_HD double& at(int i) const { return base[i * stride]; }
    TBDK_HD double& A(int i, int j, int n) const { return at(i * n - ((i * (i - 1)) >> 1) + (j - i)); }  // i <= j
    TBDK_HD double& V(int i, int j, int n) const { return at(kWsV + i * n + j); }
    TBDK_HD double& W(int i) const { return at(kWsW + i); }
};

// nine 4-bit indices in a register (indR / indC of the Jacobi)
TBDK_HD int nib_get(unsigned long long v, int i) { return (int)((v >> (4 * i)) & 15u); }
TBDK_HD unsigned long long nib_set(unsigned long long v, int i, int x)
{
    return (v & ~(15ull << (4 * i))) | ((unsigned long long)x << (4 * i));
}

// core/src/lapack.cpp:96-111
TBDK_HD double cv_hypot(double a, double b)
{
    a = fabs(a);
    b = fabs(b);
    if (a > b) {
        b /= a;
        return a * sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * sqrt(1 + a * a);
    }
    return 0;
}

// The Jacobi's loops have data-dependent bounds (the pivot's row and column).
// On the device every iteration of such a loop would wait for its own LDS
// load, so each loop is written over the fixed range [0, N) instead: all loads
// first, from an index that is always valid, then the reference's comparisons
// or rotations in the reference's order under the loop's own condition.  The
// operations and their order per element are the reference's.

// indR[k]: the column of the largest |A(k, i)|, i > k (the first on a tie)
template <int N>
TBDK_HD int jacobi_row_max(const Ws& ws, int k)
{
    double val[N];
#pragma unroll
    for (int i = 1; i < N; i++) val[i] = fabs(ws.A(k, i > k ? i : k + 1, N));
    int m = k + 1;
    double mv = fabs(ws.A(k, k + 1, N));
#pragma unroll
    for (int i = 2; i < N; i++)
        if (i >= k + 2 && mv < val[i]) mv = val[i], m = i;
    return m;
}

// indC[k]: the row of the largest |A(i, k)|, i < k (the first on a tie)
template <int N>
TBDK_HD int jacobi_col_max(const Ws& ws, int k)
{
    double val[N];
#pragma unroll
    for (int i = 0; i < N - 1; i++) val[i] = fabs(ws.A(i < k ? i : 0, k, N));
    int m = 0;
    double mv = val[0];
#pragma unroll
    for (int i = 1; i < N - 1; i++)
        if (i < k && mv < val[i]) mv = val[i], m = i;
    return m;
}

// JacobiImpl_<double> on the upper triangle ws.A: eigenvalues into ws.W in
// descending order, eigenvectors into the rows of ws.V.  At most N*N*30
// rotations, so it ends on any input; every index it forms is inside [0, N).
template <int N>
TBDK_HD void jacobi(const Ws& ws)
{
    for (int i = 0; i < N; i++) {
        for (int j = 0; j < N; j++) ws.V(i, j, N) = 0;
        ws.V(i, i, N) = 1;
    }
    unsigned long long indR = 0, indC = 0;
    for (int k = 0; k < N; k++) {
        ws.W(k) = ws.A(k, k, N);
        if (k < N - 1) indR = nib_set(indR, k, jacobi_row_max<N>(ws, k));
        if (k > 0) indC = nib_set(indC, k, jacobi_col_max<N>(ws, k));
    }
    const int max_iters = N * N * 30;
    if (N > 1)
        for (int iters = 0; iters < max_iters; iters++) {
            // the pivot: the largest of the row maxima, then of the column maxima
            double rv[N], cv[N];
#pragma unroll
            for (int i = 0; i < N - 1; i++) rv[i] = fabs(ws.A(i, nib_get(indR, i), N));
#pragma unroll
            for (int i = 1; i < N; i++) cv[i] = fabs(ws.A(nib_get(indC, i), i, N));
            int k = 0;
            double mv = rv[0];
#pragma unroll
            for (int i = 1; i < N - 1; i++)
                if (mv < rv[i]) mv = rv[i], k = i;
            int l = nib_get(indR, k);
#pragma unroll
            for (int i = 1; i < N; i++)
                if (mv < cv[i]) mv = cv[i], k = nib_get(indC, i), l = i;
            const double p = ws.A(k, l, N);
            if (fabs(p) <= DBL_EPSILON) break;
            const double y = (ws.W(l) - ws.W(k)) * 0.5;
            double t = fabs(y) + cv_hypot(p, y);
            double s = cv_hypot(p, t);
            const double c = t / s;
            s = p / s;
            t = (p / t) * p;
            if (y < 0) s = -s, t = -t;
            ws.A(k, l, N) = 0;
            ws.W(k) -= t;
            ws.W(l) += t;
            // rotate rows and columns k and l: for every i but k and l, the element of line i in
            // row / column k with the one in row / column l (the reference's three loops)
            double a0[N], b0[N];
#pragma unroll
            for (int i = 0; i < N; i++) {
                a0[i] = ws.A(i < k ? i : k, i < k ? k : i, N);
                b0[i] = ws.A(i < l ? i : l, i < l ? l : i, N);
            }
#pragma unroll
            for (int i = 0; i < N; i++)
                if (i != k && i != l) {
                    ws.A(i < k ? i : k, i < k ? k : i, N) = a0[i] * c - b0[i] * s;
                    ws.A(i < l ? i : l, i < l ? l : i, N) = a0[i] * s + b0[i] * c;
                }
            // rotate eigenvectors
#pragma unroll
            for (int i = 0; i < N; i++) {
                a0[i] = ws.V(k, i, N);
                b0[i] = ws.V(l, i, N);
            }
#pragma unroll
            for (int i = 0; i < N; i++) {
                ws.V(k, i, N) = a0[i] * c - b0[i] * s;
                ws.V(l, i, N) = a0[i] * s + b0[i] * c;
            }
            for (int j = 0; j < 2; j++) {
                const int idx = j == 0 ? k : l;
                if (idx < N - 1) indR = nib_set(indR, idx, jacobi_row_max<N>(ws, idx));
                if (idx > 0) indC = nib_set(indC, idx, jacobi_col_max<N>(ws, idx));
            }
        }
    for (int k = 0; k < N - 1; k++) {
        int m = k;
        for (int i = k + 1; i < N; i++)
            if (ws.W(m) < ws.W(i)) m = i;
        if (k != m) {
            double tmp = ws.W(m);
            ws.W(m) = ws.W(k);
            ws.W(k) = tmp;
            for (int i = 0; i < N; i++) {
                tmp = ws.V(m, i, N);
                ws.V(m, i, N) = ws.V(k, i, N);
                ws.V(k, i, N) = tmp;
            }
        }
    }
}

// ---- checkSubset on four pairs ----

// haveCollinearPoints(ms, 4): the differences are float (Point2f - Point2f), the rest double
TBDK_HD bool have_collinear4(const Pt* p)
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double dx1 = p[j].x - p[3].x, dy1 = p[j].y - p[3].y;
#pragma unroll
        for (int k = 0; k < j; k++) {
            const double dx2 = p[k].x - p[3].x, dy2 = p[k].y - p[3].y;
            if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}

// determinant(Matx33d(p.x, p.y, 1; q.x, q.y, 1; r.x, r.y, 1)) (core/matx.hpp: Matx_DetOp<_Tp, 3>)
TBDK_HD double det_rows(Pt p, Pt q, Pt r)
{
    const double a00 = p.x, a01 = p.y, a10 = q.x, a11 = q.y, a20 = r.x, a21 = r.y;
    return a00 * (a11 * 1. - a21 * 1.) - a01 * (a10 * 1. - a20 * 1.) + 1. * (a10 * a21 - a20 * a11);
}

TBDK_HD bool check_subset4(const Pt* s, const Pt* d)
{
    if (have_collinear4(s) || have_collinear4(d)) return false;
    int negative = 0;
    negative += det_rows(s[0], s[1], s[2]) * det_rows(d[0], d[1], d[2]) < 0;
    negative += det_rows(s[1], s[2], s[3]) * det_rows(d[1], d[2], d[3]) < 0;
    negative += det_rows(s[0], s[2], s[3]) * det_rows(d[0], d[2], d[3]) < 0;
    negative += det_rows(s[0], s[1], s[3]) * det_rows(d[0], d[1], d[3]) < 0;
    return negative == 0 || negative == 4;
}

// getSubset: the next accepted subset of `count` (> 4) pairs, or false after
// kMaxAttempts.  `pairs` gives M(i) and m(i), the source and destination points.
template <class Pairs>
TBDK_HD bool get_subset(const Pairs& pairs, int count, RansacRng& rng, int* i0, int* i1, int* i2, int* i3)
{
    for (int attempt = 0; attempt < kMaxAttempts; ++attempt) {
        int a = 0, b = 0, c = 0, d = 0, r;
        bool got = true;
        a = rng.draw(count);
        for (r = 0; r < kMaxRedraws; ++r) {
            b = rng.draw(count);
            if (b != a) break;
        }
        got = got && r < kMaxRedraws;
        if (got) {
            for (r = 0; r < kMaxRedraws; ++r) {
                c = rng.draw(count);
                if (c != a && c != b) break;
            }
            got = r < kMaxRedraws;
        }
        if (got) {
            for (r = 0; r < kMaxRedraws; ++r) {
                d = rng.draw(count);
                if (d != a && d != b && d != c) break;
            }
            got = r < kMaxRedraws;
        }
        if (!got) continue;
        const Pt s[4] = {pairs.M(a), pairs.M(b), pairs.M(c), pairs.M(d)};
        const Pt t[4] = {pairs.m(a), pairs.m(b), pairs.m(c), pairs.m(d)};
        if (check_subset4(s, t)) {
            *i0 = a, *i1 = b, *i2 = c, *i3 = d;
            return true;
        }
    }
    return false;
}

// ---- runKernel ----

struct Norm {
    double cmx, cmy, cMx, cMy;  // centroids of the destination (m) and source (M) points
    double smx, smy, sMx, sMy;  // count / sum of absolute deviations
};

// the centroid and deviation sums in point order; false where runKernel returns 0
template <class Pairs>
TBDK_HD bool normalize(const Pairs& pairs, int count, Norm* nm)
{
    double cmx = 0, cmy = 0, cMx = 0, cMy = 0;
    for (int i = 0; i < count; i++) {
        const Pt M = pairs.M(i), m = pairs.m(i);
        cmx += m.x;
        cmy += m.y;
        cMx += M.x;
        cMy += M.y;
    }
    cmx /= count;
    cmy /= count;
    cMx /= count;
    cMy /= count;
    double smx = 0, smy = 0, sMx = 0, sMy = 0;
    for (int i = 0; i < count; i++) {
        const Pt M = pairs.M(i), m = pairs.m(i);
        smx += fabs(m.x - cmx);
        smy += fabs(m.y - cmy);
        sMx += fabs(M.x - cMx);
        sMy += fabs(M.y - cMy);
    }
    nm->cmx = cmx, nm->cmy = cmy, nm->cMx = cMx, nm->cMy = cMy;
    nm->smx = nm->smy = nm->sMx = nm->sMy = 0;
    // a NaN sum passes, as it does in the reference: the fit goes on with NaN
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON)
        return false;
    nm->smx = count / smx, nm->smy = count / smy, nm->sMx = count / sMx, nm->sMy = count / sMy;
    return true;
}

// Lx[j] and Ly[j] of one pair (fundam.cpp:166-167)
TBDK_HD double ltl_lx(int j, double X, double Y, double x)
{
    switch (j) {
    case 0: return X;
    case 1: return Y;
    case 2: return 1;
    case 6: return -x * X;
    case 7: return -x * Y;
    case 8: return -x;
    default: return 0;
    }
}

TBDK_HD double ltl_ly(int j, double X, double Y, double y)
{
    switch (j) {
    case 3: return X;
    case 4: return Y;
    case 5: return 1;
    case 6: return -y * X;
    case 7: return -y * Y;
    case 8: return -y;
    default: return 0;
    }
}

// what pair (M, m) adds to LtL[j][k]
TBDK_HD double ltl_term(int j, int k, const Norm& nm, Pt M, Pt m)
{
    const double x = (m.x - nm.cmx) * nm.smx, y = (m.y - nm.cmy) * nm.smy;
    const double X = (M.x - nm.cMx) * nm.sMx, Y = (M.y - nm.cMy) * nm.sMy;
    return ltl_lx(j, X, Y, x) * ltl_lx(k, X, Y, x) + ltl_ly(j, X, Y, y) * ltl_ly(k, X, Y, y);
}

// all 45 entries of LtL, each summed in point order
template <class Pairs>
TBDK_HD void ltl_accumulate(const Pairs& pairs, int count, const Norm& nm, const Ws& ws)
{
    for (int e = 0; e < 45; ++e) ws.at(e) = 0;
    for (int i = 0; i < count; i++) {
        const Pt M = pairs.M(i), m = pairs.m(i);
#pragma unroll
        for (int j = 0; j < 9; j++)
#pragma unroll
            for (int k = j; k < 9; k++) ws.A(j, k, 9) += ltl_term(j, k, nm, M, m);
    }
}

// gemm's 3x3 branch (core/src/matmul.simd.hpp), alpha 1 and beta 0 on a zero C, unfused
TBDK_HD void mul3(const double* a, const double* b, double* d)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double t = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
            d[3 * i + j] = t * 1. + 0. * 0.;
        }
}

// eigen(LtL), the last eigenvector as H0, invHnorm * H0 * Hnorm2, scaled by 1 / H(2, 2)
TBDK_HD void solve_ltl(const Ws& ws, const Norm& nm, double* H)
{
    jacobi<9>(ws);
    double h0[9], ht[9];
#pragma unroll
    for (int i = 0; i < 9; i++) h0[i] = ws.V(8, i, 9);
    const double inv_hnorm[9] = {1. / nm.smx, 0, nm.cmx, 0, 1. / nm.smy, nm.cmy, 0, 0, 1};
    const double hnorm2[9] = {nm.sMx, 0, -nm.cMx * nm.sMx, 0, nm.sMy, -nm.cMy * nm.sMy, 0, 0, 1};
    mul3(inv_hnorm, h0, ht);
    mul3(ht, hnorm2, h0);
    const double s = 1. / h0[8];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = h0[i] * s + 0.;
}

// runKernel, sequential: false where it returns 0 (H untouched)
template <class Pairs>
TBDK_HD bool run_kernel(const Pairs& pairs, int count, const Ws& ws, double* H)
{
    Norm nm;
    if (!normalize(pairs, count, &nm)) return false;
    ltl_accumulate(pairs, count, nm, ws);
    solve_ltl(ws, nm, H);
    return true;
}

// ---- computeError / findInliers ----

struct ModelF {
    float h[8];
};

TBDK_HD ModelF model_f(const double* H)
{
    ModelF f;
#pragma unroll
    for (int i = 0; i < 8; i++) f.h[i] = (float)H[i];
    return f;
}

TBDK_HD float reproj_error(const ModelF& f, Pt M, Pt m)
{
    const float ww = 1.f / (f.h[6] * M.x + f.h[7] * M.y + 1.f);
    const float dx = (f.h[0] * M.x + f.h[1] * M.y + f.h[2]) * ww - m.x;
    const float dy = (f.h[3] * M.x + f.h[4] * M.y + f.h[5]) * ww - m.y;
    return dx * dx + dy * dy;
}

TBDK_HD float inlier_bound(double thr) { return (float)(thr * thr); }
TBDK_HD bool is_inlier(const ModelF& f, float t, Pt M, Pt m) { return reproj_error(f, M, m) <= t; }

// RANSACUpdateNumIters(p, ep, 4, max_iters).  log and pow are the platform's:
// the result can differ between platforms only where num / denom is within
// their error of k + 0.5, and *margin reports that distance (1 where no
// rounding took place).
TBDK_HD int update_num_iters(double p, double ep, int max_iters, double* margin)
{
    if (margin) *margin = 1.;
    p = p > 0. ? p : 0.;
    p = p < 1. ? p : 1.;
    ep = ep > 0. ? ep : 0.;
    ep = ep < 1. ? ep : 1.;
    double num = 1. - p > DBL_MIN ? 1. - p : DBL_MIN;
    double denom = 1. - pow(1. - ep, 4);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    if (denom >= 0 || -num >= max_iters * (-denom)) return max_iters;
    const double q = num / denom;
    if (margin) *margin = fabs(q - floor(q) - 0.5);
    return (int)rint(q);  // cvRound
}

// ---- the LM refinement ----

struct LmSums {
    double A[36];  // upper triangle of JtJ, row-major
    double v[8];   // Jt r
    double S;      // |r|^2
    double rinf;   // |r|_inf
};

TBDK_HD constexpr int lm_idx(int a, int b) { return a * 8 - ((a * (a - 1)) >> 1) + (b - a); }  // a <= b

TBDK_HD void lm_zero(LmSums* s)
{
#pragma unroll
    for (int i = 0; i < 36; i++) s->A[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s->v[i] = 0;
    s->S = 0;
    s->rinf = 0;
}

// HomographyRefineCallback::compute for one pair, added to the sums
TBDK_HD void lm_point(const double* h, Pt Mp, Pt mp, bool jac, LmSums* s)
{
    const double Mx = Mp.x, My = Mp.y;
    double ww = h[6] * Mx + h[7] * My + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
    const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
    const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
    const double r0 = xi - mp.x, r1 = yi - mp.y;
    s->S += r0 * r0;
    s->S += r1 * r1;
    if (!jac) return;
    s->rinf = fmax(s->rinf, fmax(fabs(r0), fabs(r1)));
    const double j0[8] = {Mx * ww, My * ww, ww, 0., 0., 0., -Mx * ww * xi, -My * ww * xi};
    const double j1[8] = {0., 0., 0., Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
#pragma unroll
    for (int a = 0; a < 8; a++) {
        s->v[a] += j0[a] * r0 + j1[a] * r1;
#pragma unroll
        for (int b = a; b < 8; b++) s->A[lm_idx(a, b)] += j0[a] * j0[b] + j1[a] * j1[b];
    }
}

// ws.A (n = 8) = A + lambda * diag(D)
TBDK_HD void lm_load(const Ws& ws, const double* A, const double* D, double lambda)
{
#pragma unroll
    for (int a = 0; a < 8; a++)
#pragma unroll
        for (int b = a; b < 8; b++) ws.A(a, b, 8) = A[lm_idx(a, b)] + (a == b ? lambda * D[a] : 0.);
}

// the sum of the eigenvalues times 2 DBL_EPSILON (SVBkSb's threshold)
TBDK_HD double lm_eig_threshold(const Ws& ws)
{
    double thr = 0;
    for (int i = 0; i < 8; i++) thr += ws.W(i);
    return thr * (DBL_EPSILON * 2);
}

// solve(ws.A, b, x, DECOMP_EIG): Jacobi, then SVBkSb
TBDK_HD void lm_eig_solve(const Ws& ws, const double* b, double* x)
{
    jacobi<8>(ws);
    const double thr = lm_eig_threshold(ws);
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = 0;
    for (int i = 0; i < 8; i++) {
        double wi = ws.W(i);
        if (fabs(wi) <= thr) continue;
        wi = 1 / wi;
        double s = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) s += ws.V(i, j, 8) * b[j];
        s *= wi;
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = x[j] + s * ws.V(i, j, 8);
    }
}

// max(DBL_EPSILON, max |diag(invert(ws.A, DECOMP_EIG))|)
TBDK_HD double lm_eig_inv_diag_max(const Ws& ws)
{
    jacobi<8>(ws);
    const double thr = lm_eig_threshold(ws);
    double maxval = DBL_EPSILON;
    for (int j = 0; j < 8; j++) {
        double d = 0;
        for (int i = 0; i < 8; i++) {
            const double wi = ws.W(i);
            if (fabs(wi) <= thr) continue;
            d += ws.V(i, j, 8) * (ws.V(i, j, 8) * (1 / wi));
        }
        maxval = fmax(maxval, fabs(d));
    }
    return maxval;
}

// LMSolverImpl::run with maxIters 10 on H[0..7].  sums(h, jac, cur) returns
// |r|^2 over the inliers at parameters h and, with jac, fills *cur (the host
// walks the inliers in order; the device reduces across a wave).  *cur is the
// caller's storage: a local on the host, LDS on the device, where every lane
// holds the same values and registers are better spent elsewhere.
template <class Sums>
TBDK_HD void lm_refine(const Sums& sums, const Ws& ws, LmSums* cur, double* H)
{
    const double Rlo = 0.25, Rhi = 0.75;
    double x[8], xd[8], d[8], D[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = H[i];
    double S = sums(x, true, cur);
#pragma unroll
    for (int i = 0; i < 8; i++) D[i] = cur->A[lm_idx(i, i)];
    double lambda = 1, lc = 0.75;
    for (int iter = 0;;) {
        lm_load(ws, cur->A, D, lambda);
        lm_eig_solve(ws, cur->v, d);
#pragma unroll
        for (int i = 0; i < 8; i++) xd[i] = x[i] - d[i];
        const double Sd = sums(xd, false, cur);
        // temp_d = -A d + 2 v; dS = d . temp_d
        double dS = 0, dv = 0, dinf = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            double ad = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) ad += cur->A[i <= j ? lm_idx(i, j) : lm_idx(j, i)] * d[j];
            dS += d[i] * (ad * -1. + cur->v[i] * 2.);
            dv += d[i] * cur->v[i];
            dinf = fmax(dinf, fabs(d[i]));
        }
        const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            double nu = (Sd - S) / (fabs(dv) > DBL_EPSILON ? dv : 1) + 2;
            nu = fmin(fmax(nu, 2.), 10.);
            if (lambda == 0) {
                lm_load(ws, cur->A, D, 0.);
                lambda = lc = 1. / lm_eig_inv_diag_max(ws);
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            S = Sd;
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = xd[i];
            (void)sums(x, true, cur);
        }
        iter++;
        const bool proceed = iter < kLmIters && dinf >= FLT_EPSILON && cur->rinf >= FLT_EPSILON;
        if (!proceed) break;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) H[i] = x[i];
}

}  // namespace homography_core
}  // namespace tbdk
