// lk_stop_check.cpp — the single-precision stopping tests of the PyrLK Newton
// step (opencv_amd/csrc/lk_stop.hpp, the text the kernels compile) against the
// reference's double expressions, on the CPU.  Built by
// tests/test_lk_stop_predicate.py with -ffp-contract=off and ASan + UBSan.
//   * |s| <= 0.01f  vs  (double)|s| < 0.01: every float within 64 ulp of +-0.01,
//     and zeros, infinities, NaN;
//   * the epsilon test per eps2 in {0, 1e-40, 1e-12, 1e-4, 0.25, 1e30, inf}:
//     10^7 random (ddx, ddy) (half of them any bit pattern, half on a ring of
//     relative width 2^-18 around sqrt(eps2)), and the pairs (d, 0), (0, d) with
//     d the floats around sqrt(eps2), so that d^2 is at, just below and just
//     above eps2.
// Required: no disagreement, and for every finite eps2 at least one input in
// the ambiguous band (the double expression evaluated).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "lk_stop.hpp"

using namespace tbdk::lkstop;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()  // splitmix64
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float bits_float(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t float_bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static long g_bad = 0;

static void check_osc(float s)
{
    if (osc_small(s) != osc_exact(s)) {
        if (g_bad++ < 10) std::printf("osc mismatch at %a\n", (double)s);
    }
}

// one (ddx, ddy) of the epsilon test; returns whether it fell in the band
static bool check_eps(float ddx, float ddy, double eps2, EpsBounds b)
{
    const bool want = eps_exact(ddx, ddy, eps2);
    const float q = eps_q(ddx, ddy);
    const bool amb = eps_ambiguous(q, b);
    const bool got = amb ? eps_exact(ddx, ddy, eps2) : eps_below(q, b);
    if (got != want || eps_reached(ddx, ddy, eps2, b) != want) {
        if (g_bad++ < 10) std::printf("eps mismatch: eps2 %a ddx %a ddy %a q %a\n", eps2, (double)ddx, (double)ddy, (double)q);
    }
    return amb;
}

int main()
{
    // ---- the oscillation test
    long n_osc = 0;
    for (int sign = 0; sign < 2; ++sign) {
        const uint32_t c = float_bits(0.01f) | (sign ? 0x80000000u : 0u);
        for (int d = -64; d <= 64; ++d, ++n_osc) check_osc(bits_float(c + (uint32_t)d));
    }
    const float special[] = {0.f, -0.f, 1.f, -1.f, std::numeric_limits<float>::infinity(),
                             -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(),
                             std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max()};
    for (float s : special) check_osc(s);

    // ---- the epsilon test
    const double eps2s[] = {0.0, 1e-40, 1e-12, 1e-4, 0.25, 1e30, std::numeric_limits<double>::infinity()};
    for (double eps2 : eps2s) {
        const EpsBounds b = eps_bounds(eps2);
        long band = 0;
        const float root = (float)std::sqrt(eps2);  // (inf for inf)
        for (int i = 0; i < 10000000; ++i) {
            const uint64_t r = rnd();
            float ddx, ddy;
            if (i & 1) {
                ddx = bits_float((uint32_t)r);
                ddy = bits_float((uint32_t)(r >> 32));
            } else {
                // radius sqrt(eps2) (1 + t), |t| < 2^-19, any angle and signs
                const double t = ((double)(r & 0xFFFFF) / 0x100000 - 0.5) * 0x1p-18;
                const double ang = (double)((r >> 20) & 0xFFFFFF) / 0x1000000 * 1.5707963267948966;
                const double rad = std::isinf(eps2) ? 1e19 : std::sqrt(eps2) * (1.0 + t);
                ddx = (float)(rad * std::cos(ang)) * ((r >> 62) & 1 ? -1.f : 1.f);
                ddy = (float)(rad * std::sin(ang)) * ((r >> 63) & 1 ? -1.f : 1.f);
            }
            band += check_eps(ddx, ddy, eps2, b);
        }
        // the boundary: d around sqrt(eps2), d^2 at / below / above eps2
        const uint32_t rb = float_bits(root);
        for (int d = -8; d <= 8; ++d) {
            const uint32_t u = rb + (uint32_t)d;
            if (d < 0 && rb < (uint32_t)-d) continue;  // below +0
            const float v = bits_float(u);
            for (float sgn : {1.f, -1.f}) {
                band += check_eps(sgn * v, 0.f, eps2, b);
                band += check_eps(0.f, sgn * v, eps2, b);
                band += check_eps(sgn * v, sgn * 0.f, eps2, b);
            }
        }
        std::printf("eps2 %g: lo %a hi %a, %ld inputs in the band\n", eps2, (double)b.lo, (double)b.hi, band);
        if (std::isfinite(eps2) && band == 0) {
            std::printf("eps2 %g: the ambiguous band was never hit\n", eps2);
            ++g_bad;
        }
    }
    if (g_bad) {
        std::printf("lk stop predicates: %ld disagreements\n", g_bad);
        return 1;
    }
    std::printf("lk stop predicates ok (%ld oscillation inputs)\n", n_osc);
    return 0;
}
