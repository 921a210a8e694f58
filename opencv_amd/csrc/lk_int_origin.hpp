// lk_int_origin.hpp — the level setup of the several-points-per-wave PyrLK
// kernels (klt_lk_multi_body.inc, Scharr on the fly) for a window whose origin
// has a zero fraction: the point has integer coordinates at the level, as every
// corner from goodFeaturesToTrack has at level 0.
//
// There the bilinear weights are (iw00, iw01, iw10, iw11) = (16384, 0, 0, 0)
// (lkpyramid.cpp:227-234), and with |Ix|, |Iy| <= 4080 and 0 <= I <= 255
//     (16384 v + 8192) >> 14 == v          (the interpolated Ix / Iy),
//     (16384 I + 256) >> 9   == 32 I       (the interpolated I x32),
// so the window terms are the Scharr values and the pixels of column x
// themselves; column x + 1 and the row below the window are not read.
//
// With no column pair to feed a dot product, the u16 pairs are packed by rows:
// per source-row pair (j, j+1), j even, the bytes x-1, x, x+1 of the two rows'
// dwords as lo, mid, hi (u16 x 2), hd = hi - lo, sm = 3 (lo + hi) + 10 mid; the
// odd pair (j+1, j+2) of hd from its two even neighbours; then for derivative
// rows (r, r+1), r even (source rows r .. r+3):
//     Ix = 3 (hdE_r + hdE_r+2) + 10 hdO_r+1,      Iy = smE_r+2 - smE_r,
// the same integers modulo 2^16 as calcSharrDeriv's (lkpyramid.cpp:55-144),
// directly the int16 x 2 row pairs the Newton step reads.
//
// Host and device: tests/cpp/lk_int_origin_check.cpp runs this text against
// calcSharrDeriv followed by the general setup's bilinear on the CPU.  The
// packed operations are one instruction each on the device and plain uint32_t
// arithmetic on the host.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TBDK_LKI_HD __host__ __device__ inline
#else
#define TBDK_LKI_HD inline
#endif

namespace tbdk {
namespace lkint {

constexpr uint32_t kW0 = 0x00004000u, kW1 = 0u;  // bilinear_weights() of a zero fraction

#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short pk16 __attribute__((ext_vector_type(2)));
TBDK_LKI_HD uint32_t pk_add(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pk16, a) + __builtin_bit_cast(pk16, b));
}
TBDK_LKI_HD uint32_t pk_sub(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pk16, a) - __builtin_bit_cast(pk16, b));
}
TBDK_LKI_HD uint32_t pk_mul(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pk16, a) * __builtin_bit_cast(pk16, b));
}
// byte K of ua and of ub, zero-extended: (ua.byte[K], ub.byte[K]) as u16 x 2
template <int K>
TBDK_LKI_HD uint32_t rows_byte(uint32_t ua, uint32_t ub)
{
    return __builtin_amdgcn_perm(ub, ua, 0x0C040C00u + 0x00010001u * K);
}
// (high half of e0, low half of e1): the odd row pair between two even ones
TBDK_LKI_HD uint32_t odd_pair(uint32_t e0, uint32_t e1) { return __builtin_amdgcn_alignbit(e1, e0, 16); }
// c + half * m, half the low (HI false) or high int16 of `pair`
template <bool HI>
TBDK_LKI_HD int mad_half(uint32_t pair, int m, int c)
{
    int t;
    if constexpr (HI) asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(t) : "v"(pair), "v"(m), "s"(c));
    else asm("v_mad_i32_i16 %0, %1, %2, %3" : "=v"(t) : "v"(pair), "v"(m), "s"(c));
    return t;
}
#else
TBDK_LKI_HD uint32_t pk_add(uint32_t a, uint32_t b) { return ((a + b) & 0xFFFFu) | (((a >> 16) + (b >> 16)) << 16); }
TBDK_LKI_HD uint32_t pk_sub(uint32_t a, uint32_t b) { return ((a - b) & 0xFFFFu) | (((a >> 16) - (b >> 16)) << 16); }
TBDK_LKI_HD uint32_t pk_mul(uint32_t a, uint32_t b)
{
    return (((a & 0xFFFFu) * (b & 0xFFFFu)) & 0xFFFFu) | (((a >> 16) * (b >> 16)) << 16);
}
template <int K>
TBDK_LKI_HD uint32_t rows_byte(uint32_t ua, uint32_t ub)
{
    return ((ua >> (8 * K)) & 0xFFu) | (((ub >> (8 * K)) & 0xFFu) << 16);
}
TBDK_LKI_HD uint32_t odd_pair(uint32_t e0, uint32_t e1) { return (e0 >> 16) | (e1 << 16); }
template <bool HI>
TBDK_LKI_HD int mad_half(uint32_t pair, int m, int c)
{
    const int h = (int)(int16_t)(HI ? pair >> 16 : pair & 0xFFFFu);
    return (int)((uint32_t)c + (uint32_t)h * (uint32_t)m);
}
#endif

// The Scharr factors of a lane as u16 x 2: (3, 3) and (10, 10); (0, 0) for a
// lane that owns no window column, whose Ix / Iy pairs must be 0 (the general
// setup's zero weights: klt_lk_multi_body.inc)
struct Factors {
    uint32_t c3, c10;
};
TBDK_LKI_HD Factors factors(bool owns_column)
{
    Factors f;
    f.c3 = owns_column ? 0x00030003u : 0u;
    f.c10 = owns_column ? 0x000A000Au : 0u;
    return f;
}

// the horizontal terms of source rows (j, j+1) from their dwords (byte 0 is
// column x - 1): mid = the pixels of column x, hd, sm as above
TBDK_LKI_HD void src_pair(uint32_t ua, uint32_t ub, Factors f, uint32_t& mid, uint32_t& hd, uint32_t& sm)
{
    const uint32_t lo = rows_byte<0>(ua, ub), hi = rows_byte<2>(ua, ub);
    mid = rows_byte<1>(ua, ub);
    hd = pk_sub(hi, lo);
    sm = pk_add(pk_mul(pk_add(lo, hi), f.c3), pk_mul(mid, f.c10));
}

// Ix and Iy of derivative rows (r, r+1) from the even source pairs (r, r+1), (r+2, r+3)
TBDK_LKI_HD uint32_t ix_pair(uint32_t hd0, uint32_t hd1, Factors f)
{
    return pk_add(pk_mul(pk_add(hd0, hd1), f.c3), pk_mul(odd_pair(hd0, hd1), f.c10));
}
TBDK_LKI_HD uint32_t iy_pair(uint32_t sm0, uint32_t sm1) { return pk_sub(sm1, sm0); }

// The whole window column.  u[j], j = 0 .. WH+1: the dword of source row j
// (level row ipy - 1 + j) whose bytes are columns x-1 .. x+2 (u[WH+2], which the
// general setup reads, is not used).  IM as TBDK_LK_IPACK_FLY:
//   IM == 0:  ic[r] = rnd9 - (I(r, x) << 14), r < WH;
//   IM != 0:  ipk[q] = (32 I(2q, x), 32 I(2q+1, x)) as int16 x 2;
// gxk[q], gyk[q] = (Ix, Iy)(2q, x), (Ix, Iy)(2q+1, x) as int16 x 2, q < (WH+1)/2;
// the second half of the last pair of an odd WH is 0.
template <int WH, int IM>
TBDK_LKI_HD void column(const uint32_t (&u)[WH + 3], Factors f, int rnd9, int* ic, uint32_t* ipk, uint32_t* gxk,
                        uint32_t* gyk)
{
    constexpr int NP = (WH + 1) / 2;
    uint32_t m0, h0, s0, m1, h1, s1;
    src_pair(u[0], u[1], f, m0, h0, s0);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int r = 2 * q;
        const bool two = r + 1 < WH;
        // source rows (r+2, r+3); row r+3 feeds only derivative row r+1
        src_pair(u[r + 2], two ? u[r + 3] : 0u, f, m1, h1, s1);
        const uint32_t keep = two ? 0xFFFFFFFFu : 0x0000FFFFu;
        gxk[q] = ix_pair(h0, h1, f) & keep;
        gyk[q] = iy_pair(s0, s1) & keep;
        // I rows r, r+1 are source rows r+1, r+2: the odd pair of mid
        if constexpr (IM == 0) {
            ic[r] = mad_half<true>(m0, -(1 << 14), rnd9);
            if (two) ic[r + 1] = mad_half<false>(m1, -(1 << 14), rnd9);
        } else {
            ipk[q] = (odd_pair(m0, m1) << 5) & keep;
        }
        m0 = m1;
        h0 = h1;
        s0 = s1;
    }
}

}  // namespace lkint
}  // namespace tbdk
