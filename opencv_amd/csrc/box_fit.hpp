// box_fit.hpp — 4-DOF similarity fit of point correspondences, the non-full-
// affine branch of getRTMatrix (video/src/lkpyramid.cpp:1398-1470), used by
// the KLT box propagation.  The sums follow the reference exactly (float
// products of Point2f, accumulated in double, in point order); the 4x4 normal
// system is solved in closed form (the reference calls cv::solve(DECOMP_EIG):
// the two agree to double rounding, see tests/test_gpu_box_fit.py).
#pragma once

#include <hip/hip_runtime.h>

#include "ransac_rng.hpp"
#include "tbdk_internal.hpp"

namespace tbdk {

struct SimilarityFit {
    double p, q, tx, ty;  // M = [p -q tx; q p ty]
    int ok;               // normal matrix not singular
};

struct SimilaritySums {
    double s00 = 0, s02 = 0, s03 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    int m = 0;

    // a[i] -> b[i], i in [0, k), appended in order (lkpyramid.cpp:1445-1454)
    template <class P>
    __host__ __device__ void add(P a, P b, int k)
    {
        for (int i = 0; i < k; ++i) {
            const float ax = a[i].x, ay = a[i].y, bx = b[i].x, by = b[i].y;
            s00 += ax * ax + ay * ay;
            s02 += ax;
            s03 += ay;
            b0 += ax * bx + ay * by;
            b1 += ax * by - ay * bx;
            b2 += bx;
            b3 += by;
        }
        m += k;
    }

    // [s00 0 s02 s03; 0 s00 -s03 s02; s02 -s03 n 0; s03 s02 0 n] [p q tx ty]^T = [b0 b1 b2 b3]^T
    __host__ __device__ SimilarityFit solve() const
    {
        SimilarityFit f{1.0, 0.0, 0.0, 0.0, 0};
        if (m <= 0) return f;
        const double n = (double)m;
        const double den = s00 - (s02 * s02 + s03 * s03) / n;
        if (!(den > 1e-9)) return f;
        f.p = (b0 - (s02 * b2 + s03 * b3) / n) / den;
        f.q = (b1 + (s03 * b2 - s02 * b3) / n) / den;
        f.tx = (b2 - s02 * f.p + s03 * f.q) / n;
        f.ty = (b3 - s03 * f.p - s02 * f.q) / n;
        f.ok = 1;
        return f;
    }
};

#if defined(__HIPCC__)
// Wave-parallel form: lane l sums pairs l, l+64, ... in order, then a fixed
// xor-butterfly combines the 64 partial sums (deterministic; differs from the
// sequential order only by double rounding, like the reference's own solve).
__device__ inline SimilarityFit wave_fit_similarity(const float2* a, const float2* b, int m, int lane)
{
    SimilaritySums p;
    for (int i = lane; i < m; i += 64) p.add(a + i, b + i, 1);
    SimilaritySums s;
    s.s00 = wave_sum_f64(p.s00);
    s.s02 = wave_sum_f64(p.s02);
    s.s03 = wave_sum_f64(p.s03);
    s.b0 = wave_sum_f64(p.b0);
    s.b1 = wave_sum_f64(p.b1);
    s.b2 = wave_sum_f64(p.b2);
    s.b3 = wave_sum_f64(p.b3);
    s.m = m;
    return s.solve();
}

// ---- RANSAC consensus of cv::estimateRigidTransform's point-set branch -------
// (video/src/lkpyramid.cpp:1591-1688, fullAffine = false, ransacSize0 = 3).
// The sample sequence is the reference's: cv::RNG seeded with (uint64)-1 per
// call, one draw per attempt, the redraw rules and the abandon rule of
// :1603-1658.  Everything the sampling touches is wave-uniform and is kept in
// scalar registers (the LDS reads of the drawn pairs go through readfirstlane);
// only the inlier test runs lanes-over-points.

// RansacRng: ransac_rng.hpp

struct RansacFit {
    SimilarityFit fit;  // over the consensus set; ok = 0 without consensus
    SimilarityFit hyp;  // the 3-point hypothesis that reached consensus
    double thr;         // inlier threshold: max(brect.width, brect.height) * 0.05
    int k;              // round at which consensus was reached, -1: none
    int good;           // consensus size
};

__device__ __forceinline__ float2 uniform_pair(const float2* p, int i)
{
    const float2 v = p[i];
    return make_float2(__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v.x))),
                       __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v.y))));
}

// :1618-1623, in float as the reference's fabs(float) overloads
__device__ __forceinline__ bool ransac_close(float2 u, float2 v)
{
    return fabsf(u.x - v.x) + fabsf(u.y - v.y) < 1.1920929e-07f;
}

// :1640-1648 for one point set
__device__ __forceinline__ bool ransac_collinear(float2 p0, float2 p1, float2 p2)
{
    const double dx1 = p1.x - p0.x, dy1 = p1.y - p0.y;
    const double dx2 = p2.x - p0.x, dy2 = p2.y - p0.y;
    return fabs(dx1 * dy2 - dy1 * dx2) < 0.01 * sqrt(dx1 * dx1 + dy1 * dy1) * sqrt(dx2 * dx2 + dy2 * dy2);
}

// :1666-1667, m = [p -q tx; q p ty]
__device__ __forceinline__ bool ransac_inlier(const SimilarityFit& h, double thr, float2 a, float2 b)
{
    const double m1 = -h.q;
    return fabs(h.p * a.x + m1 * a.y + h.tx - b.x) + fabs(h.q * a.x + h.p * a.y + h.ty - b.y) < thr;
}

// One wave, m compacted pairs a[i] -> b[i] in LDS (read only).  The outcome is
// the sequential reference's: the first round k < max_iters whose 3-point
// hypothesis has good >= m * good_ratio inliers, then getRTMatrix over those
// inliers (lane l sums inliers l, l + 64, ... in order, fixed butterfly).
__device__ inline RansacFit wave_fit_ransac(const float2* a, const float2* b, int m, int lane, int max_iters,
                                            double good_ratio)
{
    RansacFit r;
    r.fit = SimilarityFit{1.0, 0.0, 0.0, 0.0, 0};
    r.hyp = r.fit;
    r.thr = 0.0;
    r.k = -1;
    r.good = 0;
    if (m < 3) return r;
    // boundingRect(pB) of float points: floor(min), floor(max) - floor(min) + 1 (shapedescr.cpp:898-907)
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -0x7fffffff, y1 = -0x7fffffff;
    for (int i = lane; i < m; i += 64) {
        const int fx = (int)floorf(b[i].x), fy = (int)floorf(b[i].y);
        x0 = min(x0, fx);
        x1 = max(x1, fx);
        y0 = min(y0, fy);
        y1 = max(y1, fy);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64));
        y0 = min(y0, __shfl_xor(y0, o, 64));
        y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    r.thr = max(x1 - x0 + 1, y1 - y0 + 1) * 0.05;
    const double need = m * good_ratio;
    RansacRng rng;
    for (int k = 0; k < max_iters; ++k) {
        // slot 0: any index; slots 1, 2: up to max_iters draws each, a slot that
        // runs out abandons the round
        const int i0 = rng.draw(m);
        const float2 a0 = uniform_pair(a, i0), b0 = uniform_pair(b, i0);
        int i1 = 0;
        float2 a1 = a0, b1 = b0;
        bool got = false;
        for (int k1 = 0; k1 < max_iters && !got; ++k1) {
            i1 = rng.draw(m);
            if (i1 == i0) continue;
            a1 = uniform_pair(a, i1);
            b1 = uniform_pair(b, i1);
            got = !(ransac_close(a1, a0) || ransac_close(b1, b0));
        }
        if (!got) continue;
        float2 a2 = a0, b2 = b0;
        got = false;
        for (int k1 = 0; k1 < max_iters && !got; ++k1) {
            const int i2 = rng.draw(m);
            if (i2 == i0 || i2 == i1) continue;
            a2 = uniform_pair(a, i2);
            b2 = uniform_pair(b, i2);
            if (ransac_close(a2, a0) || ransac_close(b2, b0) || ransac_close(a2, a1) || ransac_close(b2, b1)) continue;
            got = !(ransac_collinear(a0, a1, a2) || ransac_collinear(b0, b1, b2));
        }
        if (!got) continue;
        SimilaritySums s3;
        s3.add(&a0, &b0, 1);
        s3.add(&a1, &b1, 1);
        s3.add(&a2, &b2, 1);
        const SimilarityFit h = s3.solve();
        int good = 0;
        for (int i0_ = 0; i0_ < m; i0_ += 64) {
            const int i = i0_ + lane;
            good += __popcll(__ballot(i < m && ransac_inlier(h, r.thr, a[i], b[i])));
        }
        if (good >= need) {
            r.k = k;
            r.good = good;
            r.hyp = h;
            break;
        }
    }
    if (r.k < 0) return r;
    SimilaritySums p;
    for (int i = lane; i < m; i += 64)
        if (ransac_inlier(r.hyp, r.thr, a[i], b[i])) p.add(a + i, b + i, 1);
    SimilaritySums s;
    s.s00 = wave_sum_f64(p.s00);
    s.s02 = wave_sum_f64(p.s02);
    s.s03 = wave_sum_f64(p.s03);
    s.b0 = wave_sum_f64(p.b0);
    s.b1 = wave_sum_f64(p.b1);
    s.b2 = wave_sum_f64(p.b2);
    s.b3 = wave_sum_f64(p.b3);
    s.m = r.good;
    r.fit = s.solve();
    return r;
}
#endif

template <class P>
__host__ __device__ inline SimilarityFit fit_similarity(P a, P b, int m)
{
    SimilaritySums s;
    s.add(a, b, m);
    return s.solve();
}

}  // namespace tbdk
