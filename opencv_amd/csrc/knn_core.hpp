// knn_core.hpp — the arithmetic of cv::BackgroundSubtractorKNN's CPU class
// (video/src/bgfg_KNN.cpp: _cvCheckPixelBackgroundNP :394-506,
// _cvUpdatePixelBackgroundNP :343-392, apply()'s schedule :749-812) and of the
// cv::randu fills it makes of its three "next update" planes (core/src/rand.cpp:
// RNG_NEXT :75, randBits_ :87-143, randi_ :153-200, RNG::fill :571-623, :702-760;
// BLOCK_SIZE 1024, precomp.hpp:269), as __host__ __device__ functions.  knn.hip's
// kernels call them; so does the stand-alone host check
// (tests/cpp/knn_core_check.cpp), which is why this file includes nothing of HIP
// and compiles with a plain C++ compiler.
//
// A sample is `channels` bytes and the include flag; here it travels as one word,
// channel c in byte c and the flag in byte CN, and so does the pixel (flag byte 0).
// Every float operation once, in the reference's order, no contraction
// (-ffp-contract=off), IEEE division.  The classification is cut into steps (one
// sample at a time) so that a kernel can stream the sample planes and stop loading
// them when every lane is decided; the same steps run on the host.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef TBDK_HD
#if defined(__HIPCC__)
#define TBDK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TBDK_HD inline
#endif
#endif

namespace tbdk {
namespace knn_core {

constexpr int kMaxSamples = 16;  // nN; a pixel holds 3 * nN samples

// the reference's setters' types: fTb and fTau are floats, nShadowDetection a uchar
struct Settings {
    int32_t history, nsamples, knn_samples, detect_shadows, shadow_value;
    float dist2_threshold, shadow_threshold;
};

// what one apply() passes to every pixel
struct FrameParams {
    float Tb, tau;
    int32_t nN, nkNN, detect_shadows, shadow_value;
    int32_t short_counter, mid_counter, long_counter;  // as they are before this frame
};

// branch counts of the host runs (nullptr in a kernel)
struct Counts {
    int64_t early_backgrounds, include_by_pbf, shadows, zero_denominators, foreground, short_updates, mid_updates,
        long_updates;
};

template <int CN>
TBDK_HD uint32_t pack(const uint8_t* p, uint8_t flag)
{
    uint32_t s = (uint32_t)flag << (8 * CN);
    for (int c = 0; c < CN; ++c) s |= (uint32_t)p[c] << (8 * c);
    return s;
}
TBDK_HD uint32_t channel(uint32_t s, int c) { return (s >> (8 * c)) & 255u; }
template <int CN>
TBDK_HD uint32_t flag_of(uint32_t s)
{
    return (s >> (8 * CN)) & 255u;
}

// ---- _cvCheckPixelBackgroundNP ------------------------------------------------------------------------------------

// the first pass: Pbf, Pb and whether the pass returned 1
struct Classify {
    int32_t Pbf, Pb;
    bool background;
};

TBDK_HD void classify_start(Classify& s)
{
    s.Pbf = 0;
    s.Pb = 0;
    s.background = false;
}

// one sample of the first loop (:413-452); not to be called once s.background is set
template <int CN>
TBDK_HD void classify_add(Classify& s, uint32_t sample, uint32_t pixel, float Tb, int nkNN)
{
    float dData[CN];
    float dist2;
    if (CN == 3) {
        dData[0] = (float)channel(sample, 0) - (float)channel(pixel, 0);
        constexpr int i1 = CN > 1 ? 1 : 0, i2 = CN - 1;  // 1 and 2; written so that CN = 1 compiles
        dData[i1] = (float)channel(sample, 1) - (float)channel(pixel, 1);
        dData[i2] = (float)channel(sample, 2) - (float)channel(pixel, 2);
        dist2 = dData[0] * dData[0] + dData[i1] * dData[i1] + dData[i2] * dData[i2];
    } else {
        dist2 = 0.f;
        for (int c = 0; c < CN; ++c) {
            dData[c] = (float)channel(sample, c) - (float)channel(pixel, c);
            dist2 += dData[c] * dData[c];
        }
    }
    if (dist2 < Tb) {
        s.Pbf++;
        if (flag_of<CN>(sample)) {
            s.Pb++;
            if (s.Pb >= nkNN) s.background = true;
        }
    }
}

// the shadow pass: verdict -1 while undecided, then 0 (foreground) or 2 (shadow)
struct Shadow {
    int32_t Ps, verdict;
};

TBDK_HD void shadow_start(Shadow& s)
{
    s.Ps = 0;
    s.verdict = -1;
}

// one sample of the second loop (:464-503); not to be called once s.verdict >= 0
template <int CN>
TBDK_HD void shadow_add(Shadow& s, uint32_t sample, uint32_t pixel, float Tb, float tau, int nkNN, Counts* cnt)
{
    if (!flag_of<CN>(sample)) return;
    float numerator = 0.0f, denominator = 0.0f;
    for (int c = 0; c < CN; ++c) {
        numerator += (float)channel(pixel, c) * (float)channel(sample, c);
        denominator += (float)channel(sample, c) * (float)channel(sample, c);
    }
    if (denominator == 0) {
        s.verdict = 0;
        if (cnt) cnt->zero_denominators++;
        return;
    }
    if (numerator <= denominator && numerator >= tau * denominator) {
        const float a = numerator / denominator;
        float dist2a = 0.0f;
        for (int c = 0; c < CN; ++c) {
            const float dD = a * (float)channel(sample, c) - (float)channel(pixel, c);
            dist2a += dD * dD;
        }
        if (dist2a < Tb * a * a) {
            s.Ps++;
            if (s.Ps >= nkNN) s.verdict = 2;
        }
    }
}

// the mask byte of the function's result: 1 -> 0, 2 -> shadow_value, 0 -> 255 (KNNInvoker :588-602)
TBDK_HD uint8_t mask_value(int result, int shadow_value)
{
    return result == 1 ? 0 : result == 2 ? (uint8_t)shadow_value : 255;
}

TBDK_HD int next_index(int i, int nN) { return i >= nN - 1 ? 0 : i + 1; }

// One pixel of KNNInvoker::operator() on a model in the reference's layout: model is the pixel's 3 * nN samples of
// CN + 1 bytes, idx / nxt its index and next-update bytes (short, mid, long).  Returns the mask byte.
template <int CN>
inline uint8_t update_pixel(uint8_t* model, uint8_t* idx, const uint8_t* nxt, const uint8_t* data, const FrameParams& p,
                            Counts* cnt)
{
    const int nd = CN + 1, total = 3 * p.nN;
    const uint32_t pixel = pack<CN>(data, 0);
    Classify c;
    classify_start(c);
    for (int n = 0; n < total && !c.background; ++n)
        classify_add<CN>(c, pack<CN>(model + n * nd, model[n * nd + CN]), pixel, p.Tb, p.nkNN);
    int result = 0;
    uint8_t include = 0;
    if (c.background) {
        result = 1;
        include = 1;
        if (cnt) cnt->early_backgrounds++;
    } else {
        if (c.Pbf >= p.nkNN) {
            include = 1;
            if (cnt) cnt->include_by_pbf++;
        }
        if (p.detect_shadows) {
            Shadow s;
            shadow_start(s);
            for (int n = 0; n < total && s.verdict < 0; ++n)
                shadow_add<CN>(s, pack<CN>(model + n * nd, model[n * nd + CN]), pixel, p.Tb, p.tau, p.nkNN, cnt);
            if (s.verdict == 2) result = 2;
        }
        if (cnt) (result == 2 ? cnt->shadows : cnt->foreground)++;
    }
    // _cvUpdatePixelBackgroundNP: the offsets from the indices as they are before any update
    const int oL = nd * (idx[2] + p.nN * 2), oM = nd * (idx[1] + p.nN), oS = nd * idx[0];
    if (nxt[2] == p.long_counter) {
        for (int b = 0; b < nd; ++b) model[oL + b] = model[oM + b];
        idx[2] = (uint8_t)next_index(idx[2], p.nN);
        if (cnt) cnt->long_updates++;
    }
    if (nxt[1] == p.mid_counter) {
        for (int b = 0; b < nd; ++b) model[oM + b] = model[oS + b];
        idx[1] = (uint8_t)next_index(idx[1], p.nN);
        if (cnt) cnt->mid_updates++;
    }
    if (nxt[0] == p.short_counter) {
        for (int b = 0; b < CN; ++b) model[oS + b] = data[b];
        model[oS + CN] = include;
        idx[0] = (uint8_t)next_index(idx[0], p.nN);
        if (cnt) cnt->short_updates++;
    }
    return mask_value(result, p.shadow_value);
}

// One pixel of getBackgroundImage (:836-851): the first sample in order whose flag is set, else 0
template <int CN>
inline void background_pixel(const uint8_t* model, int nN, uint8_t* out)
{
    for (int c = 0; c < CN; ++c) out[c] = 0;
    for (int n = 0; n < 3 * nN; ++n)
        if (model[n * (CN + 1) + CN]) {
            for (int c = 0; c < CN; ++c) out[c] = model[n * (CN + 1) + c];
            return;
        }
}

// ---- apply()'s schedule -------------------------------------------------------------------------------------------

// what the object keeps on the host between frames
struct HostState {
    int32_t nframes;
    int32_t counters[3];  // short, mid, long
};

struct FramePlan {
    bool reinit;             // the model, indices, planes and counters are zeroed first (the RNG is not touched)
    double rate;
    int32_t periods[3];      // nShortUpdate, nMidUpdate, nLongUpdate
    int32_t counters[3];     // what the kernel compares the planes with
    bool fill[3];            // the planes redrawn after the kernel, in the order short, mid, long
    HostState after;
};

// The rates the reference's arithmetic is defined for: the three K quotients are finite and fit an int with
// the increments that follow.  Exactly 0 (a quotient by log(1) = 0), above 1 (the log of a negative number)
// and a NaN do not; exactly 1 does (log(0) = -inf, every quotient +0).
inline bool quotient_ok(double q) { return q == q && q >= 0 && q <= 2147483645.0; }

// false: learning_rate is one the reference has no defined result for; *plan is then not to be used
inline bool plan_frame(const HostState& h, int history, int nN, double learning_rate, FramePlan* plan)
{
    if (!(learning_rate == learning_rate) || learning_rate == 0 || learning_rate > 1) return false;
    FramePlan& f = *plan;
    HostState s = h;
    f.reinit = s.nframes == 0 || learning_rate >= 1;
    if (f.reinit) {
        s.nframes = 0;
        s.counters[0] = s.counters[1] = s.counters[2] = 0;
    }
    ++s.nframes;
    const int m = 2 * s.nframes < history ? 2 * s.nframes : history;
    f.rate = learning_rate >= 0 && s.nframes > 1 ? learning_rate : 1. / m;
    const double l1 = log(1 - f.rate);
    const double q0 = log(0.7) / l1, q1 = log(0.4) / l1, q2 = log(0.1) / l1;
    if (!quotient_ok(q0) || !quotient_ok(q1) || !quotient_ok(q2)) return false;
    const int Kshort = (int)q0 + 1;
    const int Kmid = (int)q1 - Kshort + 1;
    const int Klong = (int)q2 - Kshort - Kmid + 1;
    f.periods[0] = Kshort / nN + 1;
    f.periods[1] = Kmid / nN + 1;
    f.periods[2] = Klong / nN + 1;
    for (int i = 0; i < 3; ++i) {
        f.counters[i] = s.counters[i];
        s.counters[i]++;
        f.fill[i] = s.counters[i] >= f.periods[i];
        if (f.fill[i]) s.counters[i] = 0;
    }
    f.after = s;
    return true;
}

inline FrameParams frame_params(const Settings& s, const FramePlan& f)
{
    FrameParams p;
    p.Tb = s.dist2_threshold;
    p.tau = s.shadow_threshold;
    p.nN = s.nsamples;
    p.nkNN = s.knn_samples;
    p.detect_shadows = s.detect_shadows;
    p.shadow_value = s.shadow_value & 255;
    p.short_counter = f.counters[0];
    p.mid_counter = f.counters[1];
    p.long_counter = f.counters[2];
    return p;
}

// ---- cv::RNG and randu on a continuous CV_8U plane, range [0, d) ---------------------------------------------------

constexpr uint64_t kRngA = 4164903690ull;            // CV_RNG_COEFF
constexpr uint64_t kRngM = (kRngA << 32) - 1;        // one step is x' = x * A (mod m), see jump()
constexpr uint64_t kRngSlack = (1ull << 32) - kRngA; // a state lies in 0 .. m + kRngSlack after one step
constexpr int kRngBlock = 1024;                      // RNG::fill's BLOCK_SIZE
constexpr int kJumpBits = 32;

TBDK_HD uint64_t rng_next(uint64_t x) { return (uint64_t)(uint32_t)x * kRngA + (x >> 32); }

enum { RANDU_SMALL = 0, RANDU_BITS = 1, RANDU_DIV = 2 };

// RNG::fill's choice for CV_8U, low 0, high d (d >= 1): idiff = d - 1, fast_int_mode when d is a power of two,
// smallFlag when idiff <= 255; otherwise DivStruct (:609-619) with delta 0
struct RanduPlan {
    int32_t mode;
    uint32_t d, mask, M;
    int32_t sh1, sh2;
};

inline RanduPlan randu_plan(int d_)
{
    RanduPlan p;
    const uint32_t d = (uint32_t)d_;
    p.d = d;
    p.mask = d - 1;
    p.M = 0;
    p.sh1 = p.sh2 = 0;
    if ((p.mask & d) == 0) {
        p.mode = p.mask <= 255 ? RANDU_SMALL : RANDU_BITS;
    } else {
        p.mode = RANDU_DIV;
        int l = 0;
        while (((uint64_t)1 << l) < d) l++;
        p.M = (uint32_t)(((uint64_t)1 << 32) * (((uint64_t)1 << l) - d) / d) + 1;
        p.sh1 = l < 1 ? l : 1;
        p.sh2 = l - 1 > 0 ? l - 1 : 0;
    }
    return p;
}

TBDK_HD uint8_t saturate_u8(int v) { return (uint8_t)((unsigned)v <= 255u ? v : v > 0 ? 255 : 0); }

// the value one step gives in the modes that take a step per value
TBDK_HD uint8_t randu_value(const RanduPlan& p, uint64_t state)
{
    if (p.mode == RANDU_DIV) {
        const uint32_t t0 = (uint32_t)state;
        uint32_t v0 = (uint32_t)(((uint64_t)t0 * p.M) >> 32);
        v0 = (v0 + ((t0 - v0) >> p.sh1)) >> p.sh2;
        v0 = t0 - v0 * p.d;
        return saturate_u8((int)v0);
    }
    return saturate_u8((int)((uint32_t)state & p.mask));
}

// steps one block of len values costs
TBDK_HD int block_steps(const RanduPlan& p, int len) { return p.mode == RANDU_SMALL ? len / 4 + len % 4 : len; }

// the index, inside a block of len values, of the first value step s of the block gives
TBDK_HD int step_value(const RanduPlan& p, int s, int len)
{
    if (p.mode != RANDU_SMALL) return s;
    const int groups = len / 4;
    return s < groups ? 4 * s : 4 * groups + (s - groups);
}

// Steps [s0, s1) of a block of len <= 1024 values, from the state before step s0; value i of the block goes to
// put(i, value), in rising order of i.  Returns the state after step s1 - 1.
template <class Put>
TBDK_HD uint64_t randu_steps(const RanduPlan& p, uint64_t state, int s0, int s1, int len, Put put)
{
    if (p.mode == RANDU_SMALL) {
        const int groups = len / 4;
        for (int s = s0; s < s1; ++s) {
            state = rng_next(state);
            const uint32_t t = (uint32_t)state;
            if (s < groups) {
                put(4 * s, (uint8_t)(t & p.mask));
                put(4 * s + 1, (uint8_t)((t >> 8) & p.mask));
                put(4 * s + 2, (uint8_t)((t >> 16) & p.mask));
                put(4 * s + 3, (uint8_t)((t >> 24) & p.mask));
            } else {
                put(4 * groups + (s - groups), (uint8_t)(t & p.mask));
            }
        }
    } else {
        for (int s = s0; s < s1; ++s) {
            state = rng_next(state);
            put(s, randu_value(p, state));
        }
    }
    return state;
}

// One block from `state`, as randBits_ / randi_ fill it
template <class Put>
TBDK_HD uint64_t randu_block(const RanduPlan& p, uint64_t state, int len, Put put)
{
    return randu_steps(p, state, 0, block_steps(p, len), len, put);
}

// the whole plane, block after block, as the reference fills it
inline uint64_t randu_fill(const RanduPlan& p, uint64_t state, uint8_t* arr, int64_t total)
{
    for (int64_t j = 0; j < total; j += kRngBlock) {
        const int len = (int)(total - j < kRngBlock ? total - j : kRngBlock);
        uint8_t* a = arr + j;
        state = randu_block(p, state, len, [a](int i, uint8_t v) { a[i] = v; });
    }
    return state;
}

// ---- jump-ahead ---------------------------------------------------------------------------------------------------
//
// With x = hi * 2^32 + lo, x * A = hi * (A * 2^32) + lo * A, and A * 2^32 = m + 1, so x * A = lo * A + hi (mod m):
// one step multiplies by A modulo m = A * 2^32 - 1.  n steps from x0 give the residue r = x0 * A^n mod m, and the
// state itself is r or r + m.  A step's result is at most (2^32 - 1) * (A + 1) = m + kRngSlack, so r + m is possible
// only when r <= kRngSlack; such a start is not guessed (jump_units, jump).  0 and m are fixed points.
//
// The powers are kept in Montgomery form (p * 2^64 mod m), so that a product with one of them is two 64 x 64 -> 128
// multiplies and no division: `__int128` on the host, the high-half multiply on the device.

// a * b as (high, low) words
TBDK_HD void mul64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *hi = __umul64hi(a, b);
    *lo = a * b;
#else
    __extension__ typedef unsigned __int128 u128;
    const u128 t = (u128)a * b;
    *hi = (uint64_t)(t >> 64);
    *lo = (uint64_t)t;
#endif
}

// -1 / m mod 2^64, by Newton's iteration (each round doubles the correct low bits; m is odd)
constexpr uint64_t neg_inverse(uint64_t m)
{
    uint64_t inv = m;  // correct to 3 bits
    for (int i = 0; i < 6; ++i) inv *= 2 - m * inv;
    return ~inv + 1;
}
constexpr uint64_t kRngMNegInv = neg_inverse(kRngM);
static_assert(kRngM * (~kRngMNegInv + 1) == 1, "the inverse of m modulo 2^64");

// a * b / 2^64 mod m for a, b < m (Montgomery's reduction; m > 2^63, so the sum before the last step has 65 bits)
TBDK_HD uint64_t montmul(uint64_t a, uint64_t b)
{
    uint64_t thi, tlo, qhi, qlo;
    mul64(a, b, &thi, &tlo);
    mul64(tlo * kRngMNegInv, kRngM, &qhi, &qlo);  // tlo + qlo == 0 (mod 2^64): it carries unless both are 0
    uint64_t r = thi + qhi;
    bool carry = r < thi;
    const uint64_t r1 = r + (tlo != 0 ? 1u : 0u);
    carry = carry || r1 < r;
    return carry || r1 >= kRngM ? r1 - kRngM : r1;
}

// a * b mod m for a, b < m (host: building the tables, and the single-step form of the jump)
inline uint64_t mulmod(uint64_t a, uint64_t b)
{
    __extension__ typedef unsigned __int128 u128;
    return (uint64_t)((u128)a * b % kRngM);
}
inline uint64_t to_mont(uint64_t a)
{
    __extension__ typedef unsigned __int128 u128;
    return (uint64_t)(((u128)a << 64) % kRngM);
}

inline uint64_t powmod_a(uint64_t n)
{
    uint64_t r = 1, b = kRngA;
    for (; n; n >>= 1) {
        if (n & 1) r = mulmod(r, b);
        b = mulmod(b, b);
    }
    return r;
}

// (A^u)^(2^k) mod m in Montgomery form, built on the host when an object is created: u = 256 and 1024 steps (a
// block of the two kinds of fill; k < 32: any block of a plane) and u = 4 and 16 steps (a lane's share of a block,
// a sixty-fourth; k < 6)
constexpr int kLaneBits = 6, kLanes = 1 << kLaneBits;
struct JumpTables {
    uint64_t p256[kJumpBits], p1024[kJumpBits], p4[kLaneBits], p16[kLaneBits];
};

inline void jump_table(uint64_t unit, int bits, uint64_t* t)
{
    uint64_t a = powmod_a(unit);
    for (int k = 0; k < bits; ++k) {
        t[k] = to_mont(a);
        a = mulmod(a, a);
    }
}

inline void jump_tables(JumpTables* t)
{
    jump_table(256, kJumpBits, t->p256);
    jump_table(1024, kJumpBits, t->p1024);
    jump_table(4, kLaneBits, t->p4);
    jump_table(16, kLaneBits, t->p16);
}

// The state `count` units after x0, a unit being `steps` steps and table[k] = (A^steps)^(2^k) in Montgomery form
// (count < 2^bits).  An ambiguous residue falls back to the nearest earlier unit boundary that is not, and steps
// from there; boundary 0 is x0 itself.
TBDK_HD uint64_t jump_units(uint64_t x0, uint32_t count, int steps, const uint64_t* table, int bits)
{
    if (x0 == 0 || x0 == kRngM) return x0;
    const uint64_t r0 = x0 >= kRngM ? x0 - kRngM : x0;  // m > 2^63
    uint32_t c = count;
    uint64_t x = x0;
    for (; c > 0; --c) {
        uint64_t r = r0;
        for (int k = 0; k < bits; ++k)
            if (c >> k & 1) r = montmul(r, table[k]);
        if (r > kRngSlack) {
            x = r;
            break;
        }
    }
    for (uint64_t i = (uint64_t)(count - c) * (uint64_t)steps; i > 0; --i) x = rng_next(x);
    return x;
}

// A fill's work item: lane `lane` of the 64 that share block b.  It takes 4 (one step per four values) or 16 steps
// of the block, the last lane also what a short block's tail adds; its start is two jumps, to the block and
// inside it.  Value i of the block goes to put(i, value).  Returns the state after the lane's last step, which for
// the lane that ends the plane is the state after the fill; *last tells whether this lane ends the block.
template <class Put>
TBDK_HD uint64_t randu_lane(const RanduPlan& p, const uint64_t* block_table, const uint64_t* lane_table, uint64_t x0,
                            uint32_t b, int lane, int len, bool* last, Put put)
{
    const bool small = p.mode == RANDU_SMALL;
    const int unit = small ? 4 : 16, steps = block_steps(p, len);
    const int s0 = lane * unit < steps ? lane * unit : steps;
    const int s1 = lane == kLanes - 1 || (lane + 1) * unit > steps ? steps : (lane + 1) * unit;
    *last = s1 == steps && s0 < steps;
    if (s0 >= s1) return 0;
    uint64_t st = jump_units(x0, b, small ? 256 : 1024, block_table, kJumpBits);
    st = jump_units(st, (uint32_t)lane, unit, lane_table, kLaneBits);
    return randu_steps(p, st, s0, s1, len, put);
}

// the state n steps after x0, by the same rule with single steps as the unit (host; the tests' form of the claim)
inline uint64_t jump(uint64_t x0, uint64_t n)
{
    if (x0 == 0 || x0 == kRngM) return x0;
    const uint64_t r0 = x0 % kRngM;
    uint64_t nn = n, x = x0;
    for (; nn > 0; --nn) {
        const uint64_t r = mulmod(r0, powmod_a(nn));
        if (r > kRngSlack) {
            x = r;
            break;
        }
    }
    for (uint64_t i = n - nn; i > 0; --i) x = rng_next(x);
    return x;
}

}  // namespace knn_core
}  // namespace tbdk
