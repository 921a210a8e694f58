// affine2d_core.hpp — the arithmetic of cv::estimateAffine2D and
// cv::estimateAffinePartial2D (calib3d/src/ptsetreg.cpp:53-371, :520-980), as
// __host__ __device__ functions: getSubset for 3 and 2 model points with
// checkSubset (precomp.hpp:136-157), the two closed-form minimal solvers, the
// float error and findInliers, RANSACUpdateNumIters with modelPoints as a
// parameter, LMEDS's rank selection and sigma, and LMSolverImpl::run
// (levmarq.cpp:89-196) for 6 and 4 parameters.  affine2d.hip's kernel calls
// them; so does the stand-alone host check (tests/cpp/affine2d_core_check.cpp),
// which is why this file includes nothing of HIP and compiles with a plain C++
// compiler.
//
// Written as homography_core.hpp is: every double operation once, in the
// reference's order, no contraction (-ffp-contract=off), storage through small
// accessors.  The Jacobi solver, the point type and the solver workspace are
// homography_core.hpp's; nothing there changes.
#pragma once

#include "homography_core.hpp"

namespace tbdk {
namespace affine2d_core {

using homography_core::Pt;
using homography_core::Ws;

constexpr int kFull = 0, kPartial = 1;     // TBDK_AFFINE2D_FULL / _PARTIAL
constexpr int kRansac = 8, kLmeds = 4;     // TBDK_AFFINE2D_RANSAC / _LMEDS
constexpr int kMaxAttemptsRansac = 10000;  // getSubset's maxAttempts as RANSAC calls it (ptsetreg.cpp:206)
constexpr int kMaxAttemptsLmeds = 1000;    // its default, which LMEDS takes (:315)
constexpr int kMaxRedraws = homography_core::kMaxRedraws;
constexpr double kLmedsOutlierRatio = 0.45;

TBDK_HD constexpr int model_points(int model) { return model == kPartial ? 2 : 3; }

// haveCollinearPoints(ms, 3): one test, of point 1 and point 0 against point 2; the differences are float
TBDK_HD bool have_collinear3(Pt p0, Pt p1, Pt p2)
{
    const double dx1 = p1.x - p2.x, dy1 = p1.y - p2.y;
    const double dx2 = p0.x - p2.x, dy2 = p0.y - p2.y;
    return fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
}

// getSubset for MP model points: the next accepted subset of `count` (> MP)
// pairs, or false after max_attempts.  With two points checkSubset never fires
// (haveCollinearPoints(ms, 2) has no pair to test): two coincident points pass.
template <int MP, class Pairs>
TBDK_HD bool get_subset(const Pairs& pairs, int count, RansacRng& rng, int max_attempts, int* idx)
{
    for (int attempt = 0; attempt < max_attempts; ++attempt) {
        int a = 0, b = 0, c = 0, r;
        a = rng.draw(count);
        for (r = 0; r < kMaxRedraws; ++r) {
            b = rng.draw(count);
            if (b != a) break;
        }
        bool got = r < kMaxRedraws;
        if (MP == 3 && got) {
            for (r = 0; r < kMaxRedraws; ++r) {
                c = rng.draw(count);
                if (c != a && c != b) break;
            }
            got = r < kMaxRedraws;
        }
        if (!got) continue;
        if (MP == 3 && (have_collinear3(pairs.M(a), pairs.M(b), pairs.M(c)) ||
                        have_collinear3(pairs.m(a), pairs.m(b), pairs.m(c))))
            continue;
        idx[0] = a, idx[1] = b;
        if (MP == 3) idx[2] = c;
        return true;
    }
    return false;
}

// Affine2DEstimatorCallback::runKernel (:571-579): f = from, t = to
TBDK_HD void solve_full(Pt f1, Pt f2, Pt f3, Pt t1, Pt t2, Pt t3, double* M)
{
    const double x1 = f1.x, y1 = f1.y, x2 = f2.x, y2 = f2.y, x3 = f3.x, y3 = f3.y;
    const double X1 = t1.x, Y1 = t1.y, X2 = t2.x, Y2 = t2.y, X3 = t3.x, Y3 = t3.y;
    const double d = 1. / (x1 * (y2 - y3) + x2 * (y3 - y1) + x3 * (y1 - y2));
    M[0] = d * (X1 * (y2 - y3) + X2 * (y3 - y1) + X3 * (y1 - y2));
    M[1] = d * (X1 * (x3 - x2) + X2 * (x1 - x3) + X3 * (x2 - x1));
    M[2] = d * (X1 * (x2 * y3 - x3 * y2) + X2 * (x3 * y1 - x1 * y3) + X3 * (x1 * y2 - x2 * y1));
    M[3] = d * (Y1 * (y2 - y3) + Y2 * (y3 - y1) + Y3 * (y1 - y2));
    M[4] = d * (Y1 * (x3 - x2) + Y2 * (x1 - x3) + Y3 * (x2 - x1));
    M[5] = d * (Y1 * (x2 * y3 - x3 * y2) + Y2 * (x3 * y1 - x1 * y3) + Y3 * (x1 * y2 - x2 * y1));
}

// AffinePartial2DEstimatorCallback::runKernel (:665-678); coincident points give d = 1/0 and a NaN model
TBDK_HD void solve_partial(Pt f1, Pt f2, Pt t1, Pt t2, double* M)
{
    const double x1 = f1.x, y1 = f1.y, x2 = f2.x, y2 = f2.y;
    const double X1 = t1.x, Y1 = t1.y, X2 = t2.x, Y2 = t2.y;
    const double d = 1. / ((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2));
    const double S0 = d * ((X1 - X2) * (x1 - x2) + (Y1 - Y2) * (y1 - y2));
    const double S1 = d * ((Y1 - Y2) * (x1 - x2) - (X1 - X2) * (y1 - y2));
    const double S2 = d * ((Y1 - Y2) * (x1 * y2 - x2 * y1) - (X1 * y2 - X2 * y1) * (y1 - y2) - (X1 * x2 - X2 * x1) * (x1 - x2));
    const double S3 = d * (-(X1 - X2) * (x1 * y2 - x2 * y1) - (Y1 * x2 - Y2 * x1) * (x1 - x2) - (Y1 * y2 - Y2 * y1) * (y1 - y2));
    M[0] = M[4] = S0;
    M[1] = -S1;
    M[2] = S2;
    M[3] = S1;
    M[5] = S3;
}

// runKernel on the subset idx of `pairs`
template <int MP, class Pairs>
TBDK_HD void run_kernel(const Pairs& pairs, const int* idx, double* M)
{
    if (MP == 3)
        solve_full(pairs.M(idx[0]), pairs.M(idx[1]), pairs.M(idx[2]), pairs.m(idx[0]), pairs.m(idx[1]), pairs.m(idx[2]), M);
    else
        solve_partial(pairs.M(idx[0]), pairs.M(idx[1]), pairs.m(idx[0]), pairs.m(idx[1]), M);
}

// ---- computeError / findInliers (:597-608, :83-100) ----

struct ModelF {
    float f[6];
};

TBDK_HD ModelF model_f(const double* M)
{
    ModelF r;
#pragma unroll
    for (int i = 0; i < 6; i++) r.f[i] = (float)M[i];
    return r;
}

TBDK_HD float reproj_error(const ModelF& F, Pt f, Pt t)
{
    const float a = F.f[0] * f.x + F.f[1] * f.y + F.f[2] - t.x;
    const float b = F.f[3] * f.x + F.f[4] * f.y + F.f[5] - t.y;
    return a * a + b * b;
}

// the threshold is taken as given: estimateAffine2D does not default one <= 0
TBDK_HD float inlier_bound(double thr) { return (float)(thr * thr); }
TBDK_HD bool is_inlier(const ModelF& F, float t, Pt f, Pt p) { return reproj_error(F, f, p) <= t; }

// RANSACUpdateNumIters(p, ep, model_points, max_iters) (:53-73).  log and pow
// are the platform's; *margin reports the distance of num / denom from k + 0.5
// (1 where no rounding took place), as homography_core::update_num_iters does.
TBDK_HD int update_num_iters(double p, double ep, int model_points, int max_iters, double* margin)
{
    if (margin) *margin = 1.;
    p = p > 0. ? p : 0.;
    p = p < 1. ? p : 1.;
    ep = ep > 0. ? ep : 0.;
    ep = ep < 1. ? ep : 1.;
    double num = 1. - p > DBL_MIN ? 1. - p : DBL_MIN;
    double denom = 1. - pow(1. - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    if (denom >= 0 || -num >= max_iters * (-denom)) return max_iters;
    const double q = num / denom;
    if (margin) *margin = fabs(q - floor(q) - 0.5);
    return (int)rint(q);  // cvRound
}

// LMEDS's iteration count (:307-308)
TBDK_HD int lmeds_num_iters(double confidence, int model_points, int max_iters, double* margin)
{
    const int n = update_num_iters(confidence, kLmedsOutlierRatio, model_points, max_iters, margin);
    return n > 3 ? n : 3;
}

// The bits of the element of rank k (0-based) among n floats ordered by their
// bit patterns, which is the value std::nth_element leaves at position k
// (:340 orders the errors as ints; they are >= +0 or NaN, so the unsigned order
// is the same).  A radix select from the top bit down: `count(mask, want)`
// returns how many elements e have (bits(e) & mask) == want.
template <class Count>
TBDK_HD unsigned rank_select(const Count& count, int k)
{
    unsigned prefix = 0, mask = 0;
    for (int b = 31; b >= 0; --b) {
        const unsigned bit = 1u << b;
        const int zeros = count(mask | bit, prefix);  // matching the prefix, bit b clear
        if (k >= zeros) {
            k -= zeros;
            prefix |= bit;
        }
        mask |= bit;
    }
    return prefix;
}

// the inlier threshold LMEDS derives from the least median (:353-354)
TBDK_HD double lmeds_sigma(double min_median, int count, int model_points)
{
    const double sigma = 2.5 * 1.4826 * (1 + 5. / (count - model_points)) * sqrt(min_median);
    return sigma > 0.001 ? sigma : 0.001;
}

// ---- the LM refinement, N parameters (6: the matrix row-major; 4: a, b, tx, ty) ----

template <int N>
struct LmSums {
    double A[N * (N + 1) / 2];  // upper triangle of JtJ, row-major
    double v[N];                // Jt r
    double S;                   // |r|^2
    double rinf;                // |r|_inf
};

template <int N>
TBDK_HD constexpr int lm_idx(int a, int b)
{
    return a * N - ((a * (a - 1)) >> 1) + (b - a);  // a <= b
}

template <int N>
TBDK_HD void lm_zero(LmSums<N>* s)
{
#pragma unroll
    for (int i = 0; i < N * (N + 1) / 2; i++) s->A[i] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) s->v[i] = 0;
    s->S = 0;
    s->rinf = 0;
}

// (a, b, tx, ty) <-> [a -b tx; b a ty] (:951-965)
TBDK_HD void partial_pack(const double* M, double* h) { h[0] = M[0], h[1] = M[3], h[2] = M[2], h[3] = M[5]; }
TBDK_HD void partial_unpack(const double* h, double* M)
{
    M[0] = M[4] = h[0];
    M[1] = -h[1];
    M[2] = h[2];
    M[3] = h[1];
    M[5] = h[3];
}

// Affine2DRefineCallback::compute (N = 6) / AffinePartial2DRefineCallback::compute (N = 4) for one pair
template <int N>
TBDK_HD void lm_point(const double* h, Pt Mp, Pt mp, bool jac, LmSums<N>* s)
{
    const double Mx = Mp.x, My = Mp.y;
    double xi, yi;
    if (N == 6) {
        xi = h[0] * Mx + h[1] * My + h[2];
        yi = h[3] * Mx + h[4] * My + h[5];
    } else {
        xi = h[0] * Mx - h[1] * My + h[2];
        yi = h[1] * Mx + h[0] * My + h[3];
    }
    const double r0 = xi - mp.x, r1 = yi - mp.y;
    s->S += r0 * r0;
    s->S += r1 * r1;
    if (!jac) return;
    s->rinf = fmax(s->rinf, fmax(fabs(r0), fabs(r1)));
    double j0[6] = {Mx, My, 1., 0., 0., 0.}, j1[6] = {0., 0., 0., Mx, My, 1.};
    if (N == 4) {
        j0[1] = -My, j0[3] = 0.;
        j1[0] = My, j1[1] = Mx, j1[2] = 0., j1[3] = 1.;
    }
#pragma unroll
    for (int a = 0; a < N; a++) {
        s->v[a] += j0[a] * r0 + j1[a] * r1;
#pragma unroll
        for (int b = a; b < N; b++) s->A[lm_idx<N>(a, b)] += j0[a] * j0[b] + j1[a] * j1[b];
    }
}

// ws.A (n = N) = A + lambda * diag(D)
template <int N>
TBDK_HD void lm_load(const Ws& ws, const double* A, const double* D, double lambda)
{
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
        for (int b = a; b < N; b++) ws.A(a, b, N) = A[lm_idx<N>(a, b)] + (a == b ? lambda * D[a] : 0.);
}

template <int N>
TBDK_HD double lm_eig_threshold(const Ws& ws)
{
    double thr = 0;
    for (int i = 0; i < N; i++) thr += ws.W(i);
    return thr * (DBL_EPSILON * 2);
}

// solve(A + lambda diag(D), v, d, DECOMP_EIG): Jacobi, then SVBkSb
template <int N>
TBDK_HD void lm_solve(const Ws& ws, const LmSums<N>* cur, const double* D, double lambda, double* x)
{
    lm_load<N>(ws, cur->A, D, lambda);
    homography_core::jacobi<N>(ws);
    const double thr = lm_eig_threshold<N>(ws);
#pragma unroll
    for (int j = 0; j < N; j++) x[j] = 0;
    for (int i = 0; i < N; i++) {
        double wi = ws.W(i);
        if (fabs(wi) <= thr) continue;
        wi = 1 / wi;
        double s = 0;
#pragma unroll
        for (int j = 0; j < N; j++) s += ws.V(i, j, N) * cur->v[j];
        s *= wi;
#pragma unroll
        for (int j = 0; j < N; j++) x[j] = x[j] + s * ws.V(i, j, N);
    }
}

// max(DBL_EPSILON, max |diag(invert(A, DECOMP_EIG))|)
template <int N>
TBDK_HD double lm_inv_diag_max(const Ws& ws, const LmSums<N>* cur, const double* D)
{
    lm_load<N>(ws, cur->A, D, 0.);
    homography_core::jacobi<N>(ws);
    const double thr = lm_eig_threshold<N>(ws);
    double maxval = DBL_EPSILON;
    for (int j = 0; j < N; j++) {
        double d = 0;
        for (int i = 0; i < N; i++) {
            const double wi = ws.W(i);
            if (fabs(wi) <= thr) continue;
            d += ws.V(i, j, N) * (ws.V(i, j, N) * (1 / wi));
        }
        maxval = fmax(maxval, fabs(d));
    }
    return maxval;
}

// LMSolverImpl::run with maxIters = max_iters (>= 1) on x[0..N).  `step`
// supplies what the caller spreads over its threads:
//   step.sums(x, jac, cur)          |r|^2 over the inliers at x; with jac it fills *cur
//   step.solve(cur, D, lambda, d)   lm_solve
//   step.inv_diag_max(cur, D)       lm_inv_diag_max
// *cur is the caller's storage (a local on the host, LDS on the device).
template <int N, class Step>
TBDK_HD void lm_refine(const Step& step, LmSums<N>* cur, int max_iters, double* x)
{
    const double Rlo = 0.25, Rhi = 0.75;
    double xd[N], d[N], D[N];
    double S = step.sums(x, true, cur);
#pragma unroll
    for (int i = 0; i < N; i++) D[i] = cur->A[lm_idx<N>(i, i)];
    double lambda = 1, lc = 0.75;
    for (int iter = 0;;) {
        step.solve(cur, D, lambda, d);
#pragma unroll
        for (int i = 0; i < N; i++) xd[i] = x[i] - d[i];
        const double Sd = step.sums(xd, false, cur);
        // temp_d = -A d + 2 v; dS = d . temp_d
        double dS = 0, dv = 0, dinf = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            double ad = 0;
#pragma unroll
            for (int j = 0; j < N; j++) ad += cur->A[i <= j ? lm_idx<N>(i, j) : lm_idx<N>(j, i)] * d[j];
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
                lambda = lc = 1. / step.inv_diag_max(cur, D);
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            S = Sd;
#pragma unroll
            for (int i = 0; i < N; i++) x[i] = xd[i];
            (void)step.sums(x, true, cur);
        }
        iter++;
        const bool proceed = iter < max_iters && dinf >= FLT_EPSILON && cur->rinf >= FLT_EPSILON;
        if (!proceed) break;
    }
}

}  // namespace affine2d_core
}  // namespace tbdk
