// remap_core.hpp — the address computation of cv::remap / cv::warpPerspective:
// map decoding (RemapInvoker, imgproc/src/imgwarp.cpp:1105-1280), the
// projective map (WarpPerspectiveInvoker, :2706-2797), cv::borderInterpolate and
// the tap indices of remapNearest / remapBilinear / remapBicubic, as
// __host__ __device__ functions.  remap.hip's kernels call them; so does the
// host bounds walk (tests/cpp/remap_bounds_check.cpp), which is why this file
// includes nothing of HIP and compiles with a plain C++ compiler.
//
// The one property everything here serves: whatever a map holds (NaN, +-inf,
// 1e30, any short), make_taps returns either no load at all or indices inside
// the source.
#pragma once

#include <limits.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TBDK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TBDK_HD inline
#endif

namespace tbdk {
namespace remap_core {

// the reference's values (tbdk.h: TBDK_INTER_*, TBDK_BORDER_*; remap.hip asserts the equality)
enum { kNearest = 0, kLinear = 1, kCubic = 2 };
enum { kConstant = 0, kReplicate = 1, kReflect = 2, kWrap = 3, kReflect101 = 4, kTransparent = 5 };
// what a destination pixel does
enum { kSample = 0, kFill = 1, kKeep = 2 };  // gather taps / write the border value / leave untouched

struct Coord {
    int sx, sy;  // integer source position (a short's range)
    int ax, ay;  // 5-bit sub-pixel fractions (0 under NEAREST)
};

// cv::invert, 3x3 CV_64F (core/src/lapack.cpp: det3, d = 1./d), double
// arithmetic; a singular matrix gives the zero matrix, as cv::invert leaves it
TBDK_HD void invert_3x3(const double* m, double* out)
{
    const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                     m[2] * (m[3] * m[7] - m[4] * m[6]);
    double t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (d != 0.) {
        const double r = 1. / d;
        t[0] = (m[4] * m[8] - m[5] * m[7]) * r;
        t[1] = (m[2] * m[7] - m[1] * m[8]) * r;
        t[2] = (m[1] * m[5] - m[2] * m[4]) * r;
        t[3] = (m[5] * m[6] - m[3] * m[8]) * r;
        t[4] = (m[0] * m[8] - m[2] * m[6]) * r;
        t[5] = (m[2] * m[3] - m[0] * m[5]) * r;
        t[6] = (m[3] * m[7] - m[4] * m[6]) * r;
        t[7] = (m[1] * m[6] - m[0] * m[7]) * r;
        t[8] = (m[0] * m[4] - m[1] * m[3]) * r;
    }
    for (int i = 0; i < 9; ++i) out[i] = t[i];
}

TBDK_HD int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// cvRound(float) as cvtss2si: ties to even; 0x80000000 for NaN and values outside int
TBDK_HD int cv_round_f(float v)
{
    const float r = rintf(v);
    return (r >= -2147483648.f && r < 2147483648.f) ? (int)r : INT_MIN;
}

// CV_32FC2 and CV_32FC1 + CV_32FC1 maps (:1134-1168 NEAREST, :1197-1274 otherwise)
TBDK_HD Coord decode_float(float mx, float my, bool nearest)
{
    Coord c;
    if (nearest) {
        c.sx = sat16(cv_round_f(mx));
        c.sy = sat16(cv_round_f(my));
        c.ax = c.ay = 0;
        return c;
    }
    const int X = cv_round_f(mx * 32.f), Y = cv_round_f(my * 32.f);
    c.sx = sat16(X >> 5);
    c.sy = sat16(Y >> 5);
    c.ax = X & 31;
    c.ay = Y & 31;
    return c;
}

// CV_16SC2 with or without its CV_16UC1 fraction plane.  Under NEAREST the
// fraction moves the position by NNDeltaTab_i (:1118-1132), which initInterTab2D
// fills with `j < INTER_TAB_SIZE/2` (:237-238): plus one where the fraction is
// BELOW one half, and the sum is stored into a short, so it wraps.  (The table
// is filled by a process's first interpolating call and is all zero before it;
// this is the state after it.)
TBDK_HD Coord decode_fixed(int x, int y, bool has_frac, unsigned frac, bool nearest)
{
    Coord c;
    const int a = (int)(frac & 1023u);
    c.sx = x;
    c.sy = y;
    c.ax = c.ay = 0;
    if (!has_frac) return c;
    if (nearest) {
        c.sx = (int)(int16_t)(uint16_t)(x + ((a & 31) < 16));
        c.sy = (int)(int16_t)(uint16_t)(y + ((a >> 5) < 16));
        return c;
    }
    c.ax = a & 31;
    c.ay = a >> 5;
    return c;
}

// the map of remap_flow, never stored: one float32 addition per coordinate
TBDK_HD Coord decode_flow(int x, int y, float fx, float fy, float sign, bool nearest)
{
    return decode_float((float)x + sign * fx, (float)y + sign * fy, nearest);
}

// WarpPerspectiveInvoker's block width: bh0 = min(16, rows), bw0 = min(1024 / bh0, cols)
TBDK_HD int perspective_block_width(int dw, int dh)
{
    const int bh0 = dh < 16 ? dh : 16, bw = 1024 / bh0;
    return bw < dw ? bw : dw;
}

// max(INT_MIN, min(INT_MAX, f)) then saturate_cast<int>.  The reference's two
// bodies disagree on a NaN (0 * inf, where W is subnormal): the SSE4.1 body
// (_mm_min_pd / _mm_max_pd / cvtpd2dq) gives INT_MIN, the scalar body
// (std::min / std::max return their first argument) INT_MAX.
TBDK_HD int persp_to_int(double f, bool vec)
{
    if (f != f) return vec ? INT_MIN : INT_MAX;
    f = f < 2147483647.0 ? f : 2147483647.0;
    f = f > -2147483648.0 ? f : -2147483648.0;
    return (int)rint(f);
}

// m maps dst -> src.  The block's origin column xb enters the rounding; the
// first bw & ~15 pixels of a block row are the SSE4.1 body's, the rest the
// scalar body's (imgwarp.sse4_1.cpp:219-494).
TBDK_HD Coord decode_perspective(const double* m, int bw0, int dw, int x, int y, bool nearest)
{
    const int xb = x / bw0 * bw0, x1 = x - xb;
    const int bw = bw0 < dw - xb ? bw0 : dw - xb;
    const bool vec = x1 < (bw & ~15);
    const double X0 = (m[0] * xb + m[1] * y) + m[2];
    const double Y0 = (m[3] * xb + m[4] * y) + m[5];
    const double W0 = (m[6] * xb + m[7] * y) + m[8];
    double W = W0 + m[6] * x1;
    W = W != 0 ? (nearest ? 1. : 32.) / W : 0;
    const int X = persp_to_int((X0 + m[0] * x1) * W, vec), Y = persp_to_int((Y0 + m[3] * x1) * W, vec);
    Coord c;
    if (nearest) {
        c.sx = sat16(X);
        c.sy = sat16(Y);
        c.ax = c.ay = 0;
    } else {
        c.sx = sat16(X >> 5);
        c.sy = sat16(Y >> 5);
        c.ax = X & 31;
        c.ay = Y & 31;
    }
    return c;
}

// cv::borderInterpolate (core/src/copy.cpp) in closed form; -1 under
// BORDER_CONSTANT.  The reference reflects in a loop, one period per turn (up
// to 16 K turns for a 2-pixel source and a hostile map); the reflections have
// period 2 len (REFLECT) and 2 len - 2 (REFLECT_101), so one remainder does it.
// |p| <= 32771 and len < 32767 here: no product or sum leaves int.
TBDK_HD int border_interp(int p, int len, int border)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (border == kReplicate) return p < 0 ? 0 : len - 1;
    if (border == kReflect || border == kReflect101) {
        if (len == 1) return 0;
        const int delta = border == kReflect101;
        const int period = 2 * len - 2 * delta;
        int q = p % period;
        if (q < 0) q += period;
        return q < len ? q : period - 1 + delta - q;
    }
    if (border == kWrap) {
        int q = p % len;
        if (q < 0) q += len;
        return q;
    }
    return -1;
}

template <int INTER>
struct TapCount {
    static constexpr int value = INTER == kNearest ? 1 : (INTER == kLinear ? 2 : 4);
};

// The columns xs[] and rows ys[] of the N x N taps of one destination pixel
// (N = 1, 2, 4), each inside the source or -1 (BORDER_CONSTANT: the border
// value stands in).  Returns kSample, kFill or kKeep; xs / ys are written only
// with kSample.
//
// One form serves the reference's inlier and border paths: with every tap inside,
// its border formulas give what its inlier formulas give (the bilinear sum is
// the same expression; the bicubic cval*ONE + sum (S - cval)*w equals sum S*w,
// the 16 weights adding up to ONE), so the inlier test only decides the
// BORDER_TRANSPARENT skip.  The reference skips whole non-inlier runs for
// cn != 3 (:760-765) and single pixels for cn == 3 (:834-837); per pixel that is
// one condition, tested here per pixel.  (Its 8UC3 inlier window is one column
// narrower under SIMD, :669-672; the pixels that leaves to the border path are
// sampled there with the same result, and are not skipped.)
template <int INTER>
TBDK_HD int make_taps(int sx, int sy, int sw, int sh, int border, int* xs, int* ys)
{
    if (INTER == kNearest) {  // remapNearest :330-428
        if ((unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh) {
            xs[0] = sx;
            ys[0] = sy;
            return kSample;
        }
        if (border == kTransparent) return kKeep;
        if (border == kConstant) return kFill;
        xs[0] = border_interp(sx, sw, border);
        ys[0] = border_interp(sy, sh, border);
        return kSample;
    }
    if (INTER == kLinear) {  // remapBilinear :649-856
        const bool inlier = (unsigned)sx < (unsigned)(sw - 1 > 0 ? sw - 1 : 0) &&
                            (unsigned)sy < (unsigned)(sh - 1 > 0 ? sh - 1 : 0);
        if (!inlier) {
            if (border == kTransparent) return kKeep;
            if (border == kConstant && (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0)) return kFill;
        }
        for (int q = 0; q < 2; ++q) {
            xs[q] = border_interp(sx + q, sw, border);
            ys[q] = border_interp(sy + q, sh, border);
        }
        return kSample;
    }
    // remapBicubic :860-958; its window starts one pixel up and left
    const int bx = sx - 1, by = sy - 1;
    const bool inlier = (unsigned)bx < (unsigned)(sw - 3 > 0 ? sw - 3 : 0) &&
                        (unsigned)by < (unsigned)(sh - 3 > 0 ? sh - 3 : 0);
    int b1 = border;
    if (!inlier) {
        if (border == kTransparent) {
            if ((unsigned)(bx + 1) >= (unsigned)sw || (unsigned)(by + 1) >= (unsigned)sh) return kKeep;
            b1 = kReflect101;
        }
        if (b1 == kConstant && (bx >= sw || bx + 4 <= 0 || by >= sh || by + 4 <= 0)) return kFill;
    }
    for (int q = 0; q < 4; ++q) {
        xs[q] = border_interp(bx + q, sw, b1);
        ys[q] = border_interp(by + q, sh, b1);
    }
    return kSample;
}

}  // namespace remap_core
}  // namespace tbdk
