// blur_host.hpp — the host side of cv::GaussianBlur on 8-bit images and of
// cv::threshold: the 8.8 fixed-point Gaussian coefficients
// (getFixedpointGaussianKernel<ufixedpoint16>, imgproc/src/smooth.dispatch.cpp:124-169),
// the kernel-size rules of createGaussianKernels and GaussianBlur (:175-199,
// :490-503) and cv::threshold's 8-bit parameter rules (imgproc/src/thresh.cpp:1556-1585),
// restated.  blur.hip plans its launches with it; tests/cpp/blur_host_check.cpp
// runs the same text under the sanitizers, which is why this file includes
// nothing of HIP.
//
// The reference evaluates the coefficients in softdouble.  Its +, -, * and / are
// IEEE-754 double operations rounded to nearest, so plain double gives the same
// bits provided nothing is contracted into an FMA (-ffp-contract=off, as the
// whole library is built) and the one mulAdd the reference does ask for is a
// real fused one.  Its exp is its own table-and-polynomial routine
// (core/src/softfloat.cpp: f64_exp), whose operation sequence sd_exp repeats;
// libm's exp differs from it in the last bits, and a coefficient within an ulp of
// a rounding boundary would flip.
#pragma once

#include <stdint.h>
#include <string.h>

namespace tbdk {
namespace blur_host {

constexpr int kMaxK = 31;  // taps a side, as tbdk_morph_u8's element

enum { kConstant = 0, kReplicate = 1, kReflect = 2, kWrap = 3, kReflect101 = 4 };  // cv::BorderTypes
enum { kBinary = 0, kBinaryInv = 1, kTrunc = 2, kToZero = 3, kToZeroInv = 4, kTypeMask = 7, kOtsu = 8, kTriangle = 16 };

inline double from_bits(uint64_t u)
{
    double d;
    memcpy(&d, &u, sizeof d);
    return d;
}

// round to the nearest integer, ties to even, for |v| < 2^51 in the default
// rounding mode (what f64_roundToInt(round_near_even) and cvRound(softdouble) do)
inline double round_even(double v)
{
    const double magic = 6755399441055744.0;  // 1.5 * 2^52
    volatile double t = v + magic;            // volatile: the sum is rounded to double before the subtraction
    return t - magic;
}

// 2^(k/64), k = 0..63, as doubles (the table f64_exp scales its polynomial with)
inline double exp2_64th(int k)
{
    static const uint64_t tab[64] = {
        0x3ff0000000000000ull, 0x3ff02c9a3e778061ull, 0x3ff059b0d3158574ull, 0x3ff0874518759bc8ull,
        0x3ff0b5586cf9890full, 0x3ff0e3ec32d3d1a2ull, 0x3ff11301d0125b51ull, 0x3ff1429aaea92de0ull,
        0x3ff172b83c7d517bull, 0x3ff1a35beb6fcb75ull, 0x3ff1d4873168b9aaull, 0x3ff2063b88628cd6ull,
        0x3ff2387a6e756238ull, 0x3ff26b4565e27cddull, 0x3ff29e9df51fdee1ull, 0x3ff2d285a6e4030bull,
        0x3ff306fe0a31b715ull, 0x3ff33c08b26416ffull, 0x3ff371a7373aa9cbull, 0x3ff3a7db34e59ff7ull,
        0x3ff3dea64c123422ull, 0x3ff4160a21f72e2aull, 0x3ff44e086061892dull, 0x3ff486a2b5c13cd0ull,
        0x3ff4bfdad5362a27ull, 0x3ff4f9b2769d2ca7ull, 0x3ff5342b569d4f82ull, 0x3ff56f4736b527daull,
        0x3ff5ab07dd485429ull, 0x3ff5e76f15ad2148ull, 0x3ff6247eb03a5585ull, 0x3ff6623882552225ull,
        0x3ff6a09e667f3bcdull, 0x3ff6dfb23c651a2full, 0x3ff71f75e8ec5f74ull, 0x3ff75feb564267c9ull,
        0x3ff7a11473eb0187ull, 0x3ff7e2f336cf4e62ull, 0x3ff82589994cce13ull, 0x3ff868d99b4492edull,
        0x3ff8ace5422aa0dbull, 0x3ff8f1ae99157736ull, 0x3ff93737b0cdc5e5ull, 0x3ff97d829fde4e50ull,
        0x3ff9c49182a3f090ull, 0x3ffa0c667b5de565ull, 0x3ffa5503b23e255dull, 0x3ffa9e6b5579fdbfull,
        0x3ffae89f995ad3adull, 0x3ffb33a2b84f15fbull, 0x3ffb7f76f2fb5e47ull, 0x3ffbcc1e904bc1d2ull,
        0x3ffc199bdd85529cull, 0x3ffc67f12e57d14bull, 0x3ffcb720dcef9069ull, 0x3ffd072d4a07897cull,
        0x3ffd5818dcfba487ull, 0x3ffda9e603db3285ull, 0x3ffdfc97337b9b5full, 0x3ffe502ee78b3ff6ull,
        0x3ffea4afa2a490daull, 0x3ffefa1bee615a27ull, 0x3fff50765b6e4540ull, 0x3fffa7c1819e90d8ull};
    return from_bits(tab[k & 63]);
}

// exp(x) for finite x, the reference's way: x * 64 / ln 2 split into an integer
// (its low six bits pick the table entry, the rest is the power of two) and a
// remainder in [-1/2, 1/2] / 64 that goes through a degree-5 polynomial.
inline double sd_exp(double x)
{
    const double c0 = from_bits(0x3f83ce0f3e46f431ull);  // every polynomial coefficient is stored over c0
    const double a5 = 1.0 / c0;
    const double a4 = from_bits(0x3fe62e42fefa39f1ull) / c0;
    const double a3 = from_bits(0x3fcebfbdff82a45aull) / c0;
    const double a2 = from_bits(0x3fac6b08d81fec75ull) / c0;
    const double a1 = from_bits(0x3f83b2a72b4f3cd3ull) / c0;
    const double a0 = from_bits(0x3f55e7aa1566c2a4ull) / c0;
    const double prescale = from_bits(0x3ff71547652b82feull) * 64.0;  // 64 / ln 2
    const double max_val = 3000.0 * 64.0;
    double x0;
    if (x >= 2048.0 || x <= -2048.0)  // a biased exponent above 1023 + 10
        x0 = x < 0 ? -max_val : max_val;
    else
        x0 = x * prescale;
    const double r = round_even(x0);
    const int val0 = (int)r;
    int t = (val0 >> 6) + 1023;  // arithmetic shift: floor
    t = t < 0 ? 0 : (t > 2047 ? 2047 : t);
    const double buf = from_bits((uint64_t)t << 52);
    x0 = (x0 - r) * (1.0 / 64.0);
    return buf * c0 * exp2_64th(val0 & 63) * (((((a0 * x0 + a1) * x0 + a2) * x0 + a3) * x0 + a4) * x0 + a5);
}

// getFixedpointGaussianKernel<ufixedpoint16>(n, sigma): out gets n coefficients in
// 1/256 units.  false: n below 1 (any n above: the 31 limit is the kernels').
inline bool gaussian_kernel_u8(int n, double sigma, uint16_t* out)
{
    if (!out || n < 1) return false;
    if (sigma <= 0 && (n == 1 || n == 3 || n == 5 || n == 7)) {
        static const uint16_t small[4][7] = {{256}, {64, 128, 64}, {16, 64, 96, 64, 16}, {8, 28, 56, 72, 56, 28, 8}};
        for (int i = 0; i < n; ++i) out[i] = small[n >> 1][i];
        return true;
    }
    // mulAdd(n, 0.15, 0.35): one rounding
    const double sg = sigma > 0 ? sigma : __builtin_fma((double)n, 0.15, 0.35);
    const double scale = (-0.5 * 0.25) / (sg * sg);
    double sum = 0;
    // the reference keeps its values in a std::vector; n is unbounded here, so they are computed twice
    for (int i = 0, x = 1 - n; i < n; ++i, x += 2) sum += sd_exp((double)(x * x) * scale);
    sum = 1.0 / sum;
    for (int i = 0, x = 1 - n; i < n; ++i, x += 2) {
        const double v = sd_exp((double)(x * x) * scale) * sum;
        // ufixedpoint16(softdouble): 0 for a negative value, else cvRound(v * 256) cut to 16 bits
        out[i] = v < 0 ? 0 : (uint16_t)(int)round_even(v * 256.0);
    }
    return true;
}

// cvRound(double): ties to even
inline int cv_round(double v) { return (int)round_even(v); }
inline int cv_floor(double v)
{
    const int i = (int)v;
    return i - (i > v);
}

// One GaussianBlur call on an isolated 8-bit image as the kernel runs it.
struct BlurPlan {
    bool copy;  // both kernels collapsed to one tap: dst = src
    int kw, kh;
    uint16_t kx[kMaxK], ky[kMaxK];
};

// createGaussianKernels and GaussianBlur's size rules.  false (the caller returns
// TBDK_EINVAL): an even or negative size, a size of 0 without a positive sigma, a
// size above kMaxK, a sigma that is NaN or too large for the automatic size.
inline bool make_plan(int width, int height, int kw, int kh, double sigma_x, double sigma_y, int border, BlurPlan* p)
{
    memset(p, 0, sizeof(*p));
    if (!(sigma_x == sigma_x) || !(sigma_y == sigma_y)) return false;
    if (sigma_x > 1e6 || sigma_y > 1e6) return false;
    // GaussianBlur: one row or one column under a border that reads the image back
    if (border != kConstant) {
        if (height == 1) kh = 1;
        if (width == 1) kw = 1;
    }
    if (kw == 1 && kh == 1) {
        p->copy = true;
        p->kw = p->kh = 1;
        p->kx[0] = p->ky[0] = 256;
        return true;
    }
    if (sigma_y <= 0) sigma_y = sigma_x;
    if (kw <= 0 && sigma_x > 0) kw = cv_round(sigma_x * 3 * 2 + 1) | 1;
    if (kh <= 0 && sigma_y > 0) kh = cv_round(sigma_y * 3 * 2 + 1) | 1;
    if (kw <= 0 || kh <= 0 || kw % 2 != 1 || kh % 2 != 1 || kw > kMaxK || kh > kMaxK) return false;
    if (sigma_x < 0) sigma_x = 0;
    if (sigma_y < 0) sigma_y = 0;
    p->kw = kw;
    p->kh = kh;
    gaussian_kernel_u8(kw, sigma_x, p->kx);
    gaussian_kernel_u8(kh, sigma_y, p->ky);
    return true;
}

// cv::threshold on 8-bit pixels, as one rule per pixel: dst = v > ithresh ? hi(v) : lo(v),
// each of hi / lo either a constant or v itself.
struct ThreshPlan {
    int ithresh;   // the value the reference returns
    int hi_const;  // -1: v
    int lo_const;  // -1: v
};

// type: one of the five, no flag bits.  false: another type.
inline bool thresh_plan_u8(double thresh, double maxval, int type, ThreshPlan* p)
{
    if (type < kBinary || type > kToZeroInv) return false;
    if (!(thresh == thresh) || !(maxval == maxval)) return false;
    const double tc = thresh < -1e9 ? -1e9 : (thresh > 1e9 ? 1e9 : thresh);
    const double mc = maxval < -1e9 ? -1e9 : (maxval > 1e9 ? 1e9 : maxval);
    const int ithresh = cv_floor(tc);
    int imaxval = cv_round(mc);
    if (type == kTrunc) imaxval = ithresh;
    imaxval = imaxval < 0 ? 0 : (imaxval > 255 ? 255 : imaxval);
    p->ithresh = ithresh;
    // the rule below gives the reference's constant fills and copies for ithresh < 0
    // (every pixel is above) and ithresh >= 255 (none is) as well: see thresh_special
    switch (type) {
    case kBinary: p->hi_const = imaxval; p->lo_const = 0; break;
    case kBinaryInv: p->hi_const = 0; p->lo_const = imaxval; break;
    case kTrunc: p->hi_const = imaxval; p->lo_const = -1; break;
    case kToZero: p->hi_const = -1; p->lo_const = 0; break;
    default: p->hi_const = 0; p->lo_const = -1; break;
    }
    // TRUNC below zero: the reference fills with 0, and saturate_cast<uchar>(ithresh) is 0
    return true;
}

// the reference's own early exits, for the tests' branch counts: 0 none, 1 a constant fill, 2 a copy
inline int thresh_special(int ithresh, int type)
{
    if (ithresh >= 0 && ithresh < 255) return 0;
    if (type == kBinary || type == kBinaryInv || ((type == kTrunc || type == kToZeroInv) && ithresh < 0) ||
        (type == kToZero && ithresh >= 255))
        return 1;
    return 2;
}

}  // namespace blur_host
}  // namespace tbdk
