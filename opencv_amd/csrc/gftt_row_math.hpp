// gftt_row_math.hpp — the per-pixel float arithmetic of the GFTT eigenvalue walk
// (klt_gftt.hip), host and device: the Sobel row terms, the gradient pair, the
// min eigenvalue of a box-summed covariance and the order-preserving float key.
// Each term that the walk spells shorter than the reference's filter engine does
// stands here next to its literal form, with the argument that the two agree bit
// for bit; tests/cpp/gftt_row_check.cpp runs both forms on the host.
// Every expression rounds as written: build with -ffp-contract=off.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBDK_ROW_HD __host__ __device__ __forceinline__
#else
#define TBDK_ROW_HD inline
#endif

namespace tbdk {

// Sobel rows of one image row at columns (x-1, x, x+1) in the reference's
// filter-engine order (see oracle/gftt_oracle.c): rx = [-1 0 1], ry = [k 2k k]
struct SobelRow {
    float rx, ry;
};

// the literal form: every tap a multiply and an add, the zero tap included
TBDK_ROW_HD SobelRow sobel_row_lit(float s0, float s1, float s2, float k, float k2)
{
    float t = -1.f * s0;
    t = t + 0.f * s1;
    t = t + 1.f * s2;
    float u = k * s0;
    u = u + k2 * s1;
    u = u + k * s2;
    return SobelRow{t, u};
}

// ... of an 8-bit image, whose pixels are the integers 0..255: rx as s2 - s0.
// -1*s0 is -s0 and 1*s2 is s2 exactly; 0*s1 is +0 since s1 >= 0 is finite, and
// (-s0) + (+0) is -s0 for s0 > 0 and +0 for s0 == 0 (round to nearest gives +0
// for (-0) + (+0)).  What remains is (-s0) + s2 against s2 - s0: the same real
// number rounded once, and when it is zero both are +0 (x - x and (-x) + x are
// +0 in round to nearest), so neither form can yield -0.  ry is unchanged.
TBDK_ROW_HD SobelRow sobel_row(float s0, float s1, float s2, float k, float k2)
{
    float u = k * s0;
    u = u + k2 * s1;
    u = u + k * s2;
    return SobelRow{s2 - s0, u};
}

// ... of a 32F image (TBDK_PIX_F32; a 16U image is one converted in the load):
// the reference's float row filter for ksize 3, SymmRowSmallFilter<float, float>
// (filter.simd.hpp:1708-1743, 2425-2469) in its unfused form: rx = S[x+1] - S[x-1],
// ry = S[x]*k0 + (S[x-1] + S[x+1])*k1
TBDK_ROW_HD SobelRow sobel_row_f32(float s0, float s1, float s2, float k, float k2)
{
    return SobelRow{s2 - s0, s1 * k2 + (s0 + s2) * k};
}

// The gradient pair of a pixel from the Sobel rows of the image rows above (p),
// at (c) and below (n) it: the column filters [k 2k k] on rx and [-1 0 1] on ry,
// each ending in the filter engine's "+ delta" with delta = 0.
struct Grad {
    float dx, dy;
};
TBDK_ROW_HD Grad grad_lit(const SobelRow& p, const SobelRow& c, const SobelRow& n, float k, float k2)
{
    return Grad{(p.rx + n.rx) * k + (c.rx * k2 + 0.f), (n.ry - p.ry) + 0.f};
}
// ... of an 8-bit or 16-bit image (non-negative integer pixels): without the
// "+ 0.f".  x + 0.f differs from x only for x == -0, and no operand can be -0:
//  - c.rx is s2 - s0 of integers: a non-zero integer or +0 (above); times
//    k2 > 0 that is a non-zero number of magnitude >= k2 (no underflow: k2 is
//    1/1530 for 8 bits, 1/6 for 16) or +0;
//  - every ry is a sum of products of non-negative numbers, so >= +0, and
//    n.ry - p.ry is -0 only for (-0) - (+0).
// dx itself then cannot be -0 either (a sum is -0 only when both terms are).
TBDK_ROW_HD Grad grad_int(const SobelRow& p, const SobelRow& c, const SobelRow& n, float k, float k2)
{
    return Grad{(p.rx + n.rx) * k + c.rx * k2, n.ry - p.ry};
}

// min eigenvalue of the 2x2 matrix [[a, b], [b, c]] from the box sums (a, b, c)
// of (dx*dx, dx*dy, dy*dy), as calcMinEigenVal writes it (corner.cpp:52-101).
// On integer pixels every box sum of squares is >= +0, so aa + cc >= +0, the
// square root is finite and >= +0, and e is finite and never -0: x - y is -0
// only for (-0) - (+0), and aa + cc is never -0.
TBDK_ROW_HD float min_eig(float a, float b, float c)
{
    const float aa = a * 0.5f, bb = b, cc = c * 0.5f;
    const float t = aa - cc;
    return (aa + cc) - sqrtf(bb * bb + t * t);
}

// float bits -> int key of the same order (for integer maxima over floats of
// either sign).  Monotonic over every non-NaN float with -0 just below +0, so
// over values that are never NaN and never -0 (min_eig on integer pixels)
// key(max(a, b)) == max(key(a), key(b)): a float maximum may run through the
// rows and its key be taken once at the end.
TBDK_ROW_HD int fkey_bits(int i) { return i >= 0 ? i : i ^ 0x7FFFFFFF; }

}  // namespace tbdk
