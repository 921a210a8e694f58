// lk_stop.hpp — the Newton step's stopping tests of the several-points-per-wave
// PyrLK kernels (klt_lk_multi_body.inc) in single precision, with the same
// truth values as the reference's double expressions (LKTrackerInvoker,
// video/src/lkpyramid.cpp:684-693).  Host and device: tests/cpp/lk_stop_check.cpp
// runs this text against the double expressions on the CPU.  Compiled without
// floating-point contraction (q below is two products and a sum, each rounded).
#pragma once

#if defined(__HIPCC__)
#define TBDK_LK_HD __host__ __device__ inline
#else
#define TBDK_LK_HD inline
#endif

namespace tbdk {
namespace lkstop {

// The reference's tests, as the kernels had them.
TBDK_LK_HD bool eps_exact(float ddx, float ddy, double eps2) { return (double)ddx * ddx + (double)ddy * ddy <= eps2; }
TBDK_LK_HD bool osc_exact(float s) { return (double)__builtin_fabsf(s) < 0.01; }

// (double)|s| < 0.01: 0.01f = 0x3C23D70A is 0.00999999977648... < 0.01 and
// the next float up, 0x3C23D70B, is 0.01000000070780... > 0.01, so no float
// lies in (0.01f, 0.01) and the double test is |s| <= 0.01f (NaN: false in both).
TBDK_LK_HD bool osc_small(float s) { return __builtin_fabsf(s) <= 0.01f; }

// Single-precision bounds of the epsilon test  E = ddx^2 + ddy^2 <= eps2.
//
// The double expression: both products are exact (24 x 24 bits), their sum
// rounds once, e64 = E (1 + d), |d| <= 2^-53.  The float expression
// q = fl(fl(ddx ddx) + fl(ddy ddy)) has three roundings of 2^-24 each, and a
// product below the smallest normal (2^-126) may lose up to 2^-126 of absolute
// value (all of it where subnormals are flushed):
//     q = E (1 + t) + u,   |t| <= 2^-22,   |u| <= 2^-125.
// For 2^-100 <= eps2 <= 2^100 take lo = fl(eps2 (1 - 2^-19)), hi = fl(eps2 (1 + 2^-19));
// the float rounding of each moves it by at most 2^-24 relative, so
// lo <= eps2 (1 - 2^-20) and hi >= eps2 (1 + 2^-20), and u <= 2^-25 eps2.  Then
//     q < lo  =>  E < (lo + 2^-125) / (1 - 2^-22) <= eps2 (1 - 2^-20 + 2^-25)(1 + 2^-21) < eps2 (1 - 2^-53)
//             =>  e64 <= eps2:  the test is true;
//     q > hi  =>  E > (hi - 2^-125) / (1 + 2^-22) >= eps2 (1 + 2^-20 - 2^-25)(1 - 2^-22) > eps2 (1 + 2^-53)
//             =>  e64 > eps2:   the test is false
// (q = +Inf from an overflowing product or sum needs E > 2^127 > eps2, false as
// well).  In between, or with q NaN, the caller evaluates eps_exact.  An eps2
// outside [2^-100, 2^100] (0, tiny, huge, Inf, NaN) gets lo = -Inf, hi = +Inf:
// no q is below lo or above hi, every step takes the double expression.
struct EpsBounds {
    float lo, hi;
};

TBDK_LK_HD EpsBounds eps_bounds(double eps2)
{
    EpsBounds b;
    b.lo = -__builtin_inff();
    b.hi = __builtin_inff();
    if (eps2 >= 0x1p-100 && eps2 <= 0x1p100) {
        b.lo = (float)(eps2 * (1.0 - 0x1p-19));
        b.hi = (float)(eps2 * (1.0 + 0x1p-19));
    }
    return b;
}

TBDK_LK_HD float eps_q(float ddx, float ddy) { return ddx * ddx + ddy * ddy; }
// the test is true / false whatever q's roundings were; neither: ambiguous
TBDK_LK_HD bool eps_below(float q, EpsBounds b) { return q < b.lo; }
TBDK_LK_HD bool eps_above(float q, EpsBounds b) { return q > b.hi; }
TBDK_LK_HD bool eps_ambiguous(float q, EpsBounds b) { return !eps_below(q, b) && !eps_above(q, b); }

// the whole test for one point (the kernels branch on eps_ambiguous per wave)
TBDK_LK_HD bool eps_reached(float ddx, float ddy, double eps2, EpsBounds b)
{
    const float q = eps_q(ddx, ddy);
    return eps_ambiguous(q, b) ? eps_exact(ddx, ddy, eps2) : eps_below(q, b);
}

}  // namespace lkstop
}  // namespace tbdk
