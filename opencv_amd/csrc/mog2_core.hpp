// mog2_core.hpp — the per-pixel arithmetic of cv::BackgroundSubtractorMOG2
// (video/src/bgfg_gaussmix2.cpp: MOG2Invoker::operator() :568-753,
// detectShadowGMM :476-521, getBackgroundImage_intern :884-925, and the
// per-frame constants apply() derives :859-881), as __host__ __device__
// functions.  mog2.hip's kernels call them; so does the stand-alone host check
// (tests/cpp/mog2_core_check.cpp), which is why this file includes nothing of
// HIP and compiles with a plain C++ compiler.
//
// Every float operation once, in the reference's order, no contraction
// (-ffp-contract=off), IEEE division.  A pixel's model is K modes held in three
// small arrays (weight, variance, mean[K][CN]); K is a template parameter and
// every loop over modes has a constant bound with the live count as a
// predicate, and every store at a computed position is a chain of selects, so
// that a kernel keeps the arrays in registers.  The same text runs on the host.
#pragma once

#include <float.h>
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
namespace mog2_core {

constexpr int kMaxMixtures = 8;

// what one apply() passes to every pixel
struct FrameParams {
    float alphaT, alpha1, prune;  // the learning rate, 1 - rate, -rate * fCT
    float Tb, TB, Tg;             // varThreshold, backgroundRatio, varThresholdGen
    float varInit, varMin, varMax, tau;
    int32_t nmixtures;
    int32_t detect_shadows;
    int32_t shadow_value;
};

// the reference's setters' types: varThreshold stays double, the others are floats
struct Settings {
    int32_t history, nmixtures, detect_shadows, shadow_value;
    double var_threshold;
    float var_threshold_gen, var_init, var_min, var_max, background_ratio, complexity_reduction, shadow_threshold;
};

// apply()'s schedule (:859-869): nframes is the count before this frame, learning_rate the caller's.
// Returns the rate used; *reinit tells whether the model is cleared first.
inline double schedule(int* nframes, int history, double learning_rate, bool* reinit)
{
    *reinit = *nframes == 0 || learning_rate >= 1;
    if (*reinit) *nframes = 0;
    ++*nframes;
    const int m = 2 * *nframes < history ? 2 * *nframes : history;
    return learning_rate >= 0 && *nframes > 1 ? learning_rate : 1. / m;
}

// the constants of one frame: alphaT, prune and Tb are narrowed from double as apply() does (:876-879),
// varMin / varMax are MOG2Invoker's MIN / MAX of the two given values (:560-561)
inline FrameParams frame_params(const Settings& s, double rate)
{
    FrameParams p;
    p.alphaT = (float)rate;
    p.alpha1 = 1.f - p.alphaT;
    p.prune = float(-rate * s.complexity_reduction);
    p.Tb = (float)s.var_threshold;
    p.TB = s.background_ratio;
    p.Tg = s.var_threshold_gen;
    p.varInit = s.var_init;
    p.varMin = s.var_min > s.var_max ? s.var_max : s.var_min;
    p.varMax = s.var_min < s.var_max ? s.var_max : s.var_min;
    p.tau = s.shadow_threshold;
    p.nmixtures = s.nmixtures;
    p.detect_shadows = s.detect_shadows;
    p.shadow_value = s.shadow_value & 255;
    return p;
}

// branch counts of the host runs (nullptr in a kernel)
struct Counts {
    int64_t fits, new_modes, replacements, prunes, fit_sorts, new_sorts, shadows, foreground, var_max_clamps,
        var_min_clamps, zero_denominators;
};

template <int CN, int K>
TBDK_HD void swap_modes(float* w, float* v, float* m, int i, int j)
{
    float t = w[i];
    w[i] = w[j];
    w[j] = t;
    t = v[i];
    v[i] = v[j];
    v[j] = t;
    for (int c = 0; c < CN; ++c) {
        t = m[i * CN + c];
        m[i * CN + c] = m[j * CN + c];
        m[j * CN + c] = t;
    }
}

// detectShadowGMM on the updated model
template <int CN, int K>
TBDK_HD bool detect_shadow(const float* w, const float* v, const float* m, int nmodes, const float* d,
                           const FrameParams& p, Counts* cnt)
{
    float tWeight = 0.f;
    int verdict = -1;  // undecided
#pragma unroll
    for (int mode = 0; mode < K; ++mode) {
        if (mode < nmodes && verdict < 0) {
            float numerator = 0.f, denominator = 0.f;
            for (int c = 0; c < CN; ++c) {
                numerator += d[c] * m[mode * CN + c];
                denominator += m[mode * CN + c] * m[mode * CN + c];
            }
            if (denominator == 0) {
                verdict = 0;
                if (cnt) cnt->zero_denominators++;
            } else {
                if (numerator <= denominator && numerator >= p.tau * denominator) {
                    const float a = numerator / denominator;
                    float dist2a = 0.f;
                    for (int c = 0; c < CN; ++c) {
                        const float dD = a * m[mode * CN + c] - d[c];
                        dist2a += dD * dD;
                    }
                    if (dist2a < p.Tb * v[mode] * a * a) verdict = 1;
                }
                if (verdict < 0) {
                    tWeight += w[mode];
                    if (tWeight > p.TB) verdict = 0;
                }
            }
        }
    }
    return verdict == 1;
}

// One pixel of MOG2Invoker::operator(): updates the model (w, v: K floats, m: K * CN floats, *nmodes_io)
// by the sample d and returns the mask byte.  p.nmixtures <= K.
template <int CN, int K>
TBDK_HD uint8_t update_pixel(float* w, float* v, float* m, int* nmodes_io, const float* d, const FrameParams& p,
                             Counts* cnt)
{
    bool background = false, fits = false;
    int nmodes = *nmodes_io;
    float totalWeight = 0.f;

    // the loop's bound is the live count, which a prune lowers while the loop runs:
    // after a prune below the last mode the last mode is not visited
#pragma unroll
    for (int mode = 0; mode < K; ++mode) {
        if (mode < nmodes) {
            float weight = p.alpha1 * w[mode] + p.prune;
            int pos = mode;  // mode - swap_count
            if (!fits) {
                const float var = v[mode];
                float dData[CN];
                // the reference's three-channel form, d0*d0 + d1*d1 + d2*d2, is this sum: 0 + x is x
                float dist2 = 0.f;
                for (int c = 0; c < CN; ++c) {
                    dData[c] = m[mode * CN + c] - d[c];
                    dist2 += dData[c] * dData[c];
                }
                if (totalWeight < p.TB && dist2 < p.Tb * var) background = true;
                if (dist2 < p.Tg * var) {
                    fits = true;
                    if (cnt) cnt->fits++;
                    weight += p.alphaT;
                    const float k = p.alphaT / weight;
                    for (int c = 0; c < CN; ++c) m[mode * CN + c] -= k * dData[c];
                    float varnew = var + k * (dist2 - var);
                    // MAX(a, b) is (a) < (b) ? (b) : (a), MIN(a, b) is (a) > (b) ? (b) : (a): a NaN passes both
                    if (cnt && varnew < p.varMin) cnt->var_min_clamps++;
                    varnew = varnew < p.varMin ? p.varMin : varnew;
                    if (cnt && varnew > p.varMax) cnt->var_max_clamps++;
                    varnew = varnew > p.varMax ? p.varMax : varnew;
                    v[mode] = varnew;
                    // the matched mode moves up while its new weight is not below the one above
                    bool moving = true;
#pragma unroll
                    for (int i = mode; i > 0; --i) {
                        if (moving) {
                            if (weight < w[i - 1]) {
                                moving = false;
                            } else {
                                swap_modes<CN, K>(w, v, m, i, i - 1);
                                pos = i - 1;
                            }
                        }
                    }
                    if (cnt && pos != mode) cnt->fit_sorts++;
                }
            }
            if (weight < -p.prune) {
                weight = 0.f;
                nmodes--;
                if (cnt) cnt->prunes++;
            }
#pragma unroll
            for (int j = 0; j <= mode; ++j)
                if (j == pos) w[j] = weight;
            totalWeight += weight;
        }
    }

    float invWeight = 0.f;
    if (fabsf(totalWeight) > FLT_EPSILON) invWeight = 1.f / totalWeight;
#pragma unroll
    for (int mode = 0; mode < K; ++mode)
        if (mode < nmodes) w[mode] *= invWeight;

    if (!fits && p.alphaT > 0.f) {
        // replace the weakest or add a new one
        int mode;
        if (nmodes == p.nmixtures) {
            mode = p.nmixtures - 1;
            if (cnt) cnt->replacements++;
        } else {
            mode = nmodes++;
        }
        if (cnt) cnt->new_modes++;
        const float wnew = nmodes == 1 ? 1.f : p.alphaT;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j == mode) {
                w[j] = wnew;
                v[j] = p.varInit;
                for (int c = 0; c < CN; ++c) m[j * CN + c] = d[c];
            } else if (nmodes != 1 && j < nmodes - 1) {
                w[j] *= p.alpha1;
            }
        }
        // its place: alphaT, not the stored weight, against the mode above
        bool moving = true, moved = false;
#pragma unroll
        for (int i = K - 1; i > 0; --i) {
            if (i <= nmodes - 1 && moving) {
                if (p.alphaT < w[i - 1]) {
                    moving = false;
                } else {
                    swap_modes<CN, K>(w, v, m, i, i - 1);
                    moved = true;
                }
            }
        }
        if (cnt && moved) cnt->new_sorts++;
    }

    *nmodes_io = nmodes;
    if (background) return 0;
    if (p.detect_shadows && detect_shadow<CN, K>(w, v, m, nmodes, d, p, cnt)) {
        if (cnt) cnt->shadows++;
        return (uint8_t)p.shadow_value;
    }
    if (cnt) cnt->foreground++;
    return 255;
}

// One pixel of getBackgroundImage_intern: the weighted mean of the first modes whose summed
// weight exceeds TB (the break comes after adding), times 1 / totalWeight; 0 without modes
// as three steps, so that a kernel can stream the modes: start, one bg_add per mode while open, bg_value
template <int CN>
struct BgAcc {
    float meanVal[CN];
    float totalWeight;
    bool open;
};

template <int CN>
TBDK_HD void bg_start(BgAcc<CN>& a)
{
    for (int c = 0; c < CN; ++c) a.meanVal[c] = 0.f;
    a.totalWeight = 0.f;
    a.open = true;
}

template <int CN>
TBDK_HD void bg_add(BgAcc<CN>& a, float weight, const float* mean, float TB)
{
    for (int c = 0; c < CN; ++c) a.meanVal[c] += weight * mean[c];
    a.totalWeight += weight;
    if (a.totalWeight > TB) a.open = false;
}

template <int CN>
TBDK_HD void bg_value(const BgAcc<CN>& a, float* out)
{
    float invWeight = 0.f;
    if (fabsf(a.totalWeight) > FLT_EPSILON) invWeight = 1.f / a.totalWeight;
    for (int c = 0; c < CN; ++c) out[c] = a.meanVal[c] * invWeight;
}

template <int CN>
TBDK_HD void background_pixel(const float* w, const float* m, int nmodes, float TB, float* out)
{
    BgAcc<CN> a;
    bg_start<CN>(a);
    for (int mode = 0; mode < nmodes && a.open; ++mode) bg_add<CN>(a, w[mode], m + mode * CN, TB);
    bg_value<CN>(a, out);
}

// saturate_cast<uchar>(float): cvRound (round half to even), then clamped to 0..255; NaN gives 0
TBDK_HD uint8_t saturate_u8(float x)
{
    const float r = rintf(x);
    return !(r > 0.f) ? 0 : r > 255.f ? 255 : (uint8_t)(int)r;
}

}  // namespace mog2_core
}  // namespace tbdk
