// lk_walk.hpp — the level walk of the one-point-per-wave PyrLK kernels
// (lk_sparse_kernel, lk_sparse_back_kernel, lk_strip_kernel, lk_cn_kernel,
// lk_cn_f32_kernel): LKTrackerInvoker's control rules (video/src/lkpyramid.cpp:
// 178-695), written once.  All control flow is wave-uniform.
//
// What differs between the kernels is a window policy `Win`:
//   win_w(), win_h()      the window size (compile-time for the strip kernel)
//   gate(fx, fy, ix, iy, L)
//                         true when the window origin (ix, iy) = floor(fx, fy)
//                         is outside level L (the fp32 path also names NaN)
//   setup(L, ipx, ipy, fa, fb, A11, A12, A22)
//                         stages the window of I and its derivatives at origin
//                         (ipx, ipy), fractions (fa, fb); returns the G sums
//                         scaled by FLT_SCALE
//   step(L, inx, iny, fa, fb, b1, b2)
//                         one Newton step's b sums against J at (inx, iny),
//                         scaled as the pixel path scales them
//   error(L, inx, iny, fa, fb)
//                         the level-0 L1 error, normalised
//   release()             the barrier an LDS policy needs before the next
//                         level's setup rewrites its arrays
// Built with -ffp-contract=off: every float / double expression below is
// evaluated as written, which is as the reference writes it.
//
// The several-points-per-wave kernels (klt_lk_multi_body.inc, klt_f16.hip) run
// the same rules per point under lane masks and keep their own text.
#pragma once
#include "lk_device.hpp"

namespace tbdk {

struct LkWalkOut {
    float x, y;  // the tracked point
    float err;   // the level-0 error, or minEig under GET_MIN_EIGENVALS
    int status;
    int nit;  // Newton steps taken over all levels
};

// p0: the point in the first image; init: the start in the second image, read
// only under USE_INITIAL_FLOW; want_err: run the level-0 error pass
template <class Win>
__device__ __forceinline__ void lk_walk(const LkArgs& a, int flags, bool want_err, float p0x, float p0y,
                                        float init_x, float init_y, Win& win, LkWalkOut& out)
{
    const int winW = win.win_w(), winH = win.win_h();
    const float halfx = (winW - 1) * 0.5f, halfy = (winH - 1) * 0.5f;
    float outx = init_x, outy = init_y;
    int status = 1, nit = 0;
    float errv = 0.f;

    for (int level = a.max_level; level >= 0; --level) {
        const LkLevel L = a.lv[level];
        const float sc = (float)(1. / (1 << level));
        float prevx = p0x * sc, prevy = p0y * sc;
        float nextx, nexty;
        if (level == a.max_level) {
            if (flags & TBDK_OPTFLOW_USE_INITIAL_FLOW) {
                nextx = outx * sc;
                nexty = outy * sc;
            } else {
                nextx = prevx;
                nexty = prevy;
            }
        } else {
            nextx = outx * 2.f;
            nexty = outy * 2.f;
        }
        outx = nextx;
        outy = nexty;

        prevx -= halfx;
        prevy -= halfy;
        const int ipx = (int)floorf(prevx), ipy = (int)floorf(prevy);
        if (win.gate(prevx, prevy, ipx, ipy, L)) {
            if (level == 0) {
                status = 0;
                errv = 0.f;
            }
            continue;
        }
        // A = float(sum) * 2^-20   (lkpyramid.cpp:438-440)
        float A11, A12, A22;
        win.setup(L, ipx, ipy, prevx - ipx, prevy - ipy, A11, A12, A22);

        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                             (float)(2 * winW * winH);
        if (flags & TBDK_OPTFLOW_LK_GET_MIN_EIGENVALS) errv = minEig;
        if (minEig < a.min_eig || D < 1.19209290e-07F /*FLT_EPSILON*/) {
            if (level == 0) status = 0;
            win.release();
            continue;
        }
        D = 1.f / D;

        nextx -= halfx;
        nexty -= halfy;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_count; ++j) {
            const int inx = (int)floorf(nextx), iny = (int)floorf(nexty);
            if (win.gate(nextx, nexty, inx, iny, L)) {
                if (level == 0) status = 0;
                break;
            }
            nit++;
            float b1, b2;
            win.step(L, inx, iny, nextx - inx, nexty - iny, b1, b2);
            const float ddx = (A12 * b2 - A22 * b1) * D;
            const float ddy = (A12 * b1 - A11 * b2) * D;
            nextx += ddx;
            nexty += ddy;
            outx = nextx + halfx;
            outy = nexty + halfy;
            if ((double)ddx * ddx + (double)ddy * ddy <= a.eps2) break;
            if (j > 0 && (double)fabsf(ddx + pdx) < 0.01 && (double)fabsf(ddy + pdy) < 0.01) {
                outx -= ddx * 0.5f;
                outy -= ddy * 0.5f;
                break;
            }
            pdx = ddx;
            pdy = ddy;
        }

        if (level == 0 && status && want_err && (flags & TBDK_OPTFLOW_LK_GET_MIN_EIGENVALS) == 0) {
            const float npx = outx - halfx, npy = outy - halfy;
            const int inx = (int)floorf(npx), iny = (int)floorf(npy);
            if (win.gate(npx, npy, inx, iny, L)) status = 0;
            else errv = win.error(L, inx, iny, npx - inx, npy - iny);
        }
        win.release();
    }
    out.x = outx;
    out.y = outy;
    out.err = errv;
    out.status = status;
    out.nit = nit;
}

// the forward kernels' prologue and epilogue: point i of the launch, started at
// next_pts under USE_INITIAL_FLOW; lane 0 stores the result
template <class Win>
__device__ __forceinline__ void lk_walk_point(const LkArgs& a, int i, bool lane0, Win& win)
{
    const float p0x = a.prev_pts[2 * i], p0y = a.prev_pts[2 * i + 1];
    float init_x = 0.f, init_y = 0.f;
    if (a.flags & TBDK_OPTFLOW_USE_INITIAL_FLOW) {
        init_x = a.next_pts[2 * i];
        init_y = a.next_pts[2 * i + 1];
    }
    LkWalkOut o;
    lk_walk(a, a.flags, a.err != nullptr, p0x, p0y, init_x, init_y, win, o);
    if (lane0) {
        a.next_pts[2 * i] = o.x;
        a.next_pts[2 * i + 1] = o.y;
        a.status[i] = (uint8_t)o.status;
        if (a.err) a.err[i] = o.err;
        if (a.iters) a.iters[i] = o.nit;
    }
}

}  // namespace tbdk
