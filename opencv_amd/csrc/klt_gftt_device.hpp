// klt_gftt_device.hpp — device helpers shared by the two GFTT selection paths
// (klt_gftt.hip: one workgroup per ROI, candidates in LDS; klt_gftt_wide.hip:
// candidates in global scratch): the order-preserving float key, the ROI table
// lookup, the candidate sort key and the LDS key sorts.
#pragma once
#include <cstdint>

#include "tbdk_internal.hpp"

namespace tbdk {

// float -> int order-preserving key (for atomicMax on floats of either sign)
__device__ __forceinline__ int fkey(float f)
{
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float fkey_inv(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

// ROI r of the launch: from the kernel arguments when the table travels there
// (GfttArgs::inl), else from the table in memory
__device__ __forceinline__ GfttRoi roi_at(const GfttArgs& a, int r)
{
    if (a.ninl > 0) {
        const GfttRoiC c = a.inl[r];
        return GfttRoi{c.x, c.y, c.w, c.h, c.off, c.moff, c.cblk};
    }
    return a.rois[r];
}

// Candidate sort key: the reference order (value desc, then address desc,
// featureselect.cpp:56-64) is the descending order of
//   (orderable bits of the float value) << 32 | (y << 16 | x)
__device__ __forceinline__ uint64_t cand_key(float v, int y, int x)
{
    return ((uint64_t)((uint32_t)fkey(v) ^ 0x80000000u) << 32) | (uint32_t)((y << 16) | x);
}

constexpr int kSelThreads = 512;

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d)
{
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const int l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
    return ((uint64_t)(uint32_t)h2 << 32) | (uint32_t)l2;
}

// Bitonic sort of np2 keys, descending, E keys per thread in registers
// (element e = tid * E + u): stages with j < E swap registers, E <= j < 64E
// exchange across lanes of the wave (no barrier), only j >= 64E go through LDS.
template <int E>
__device__ __forceinline__ void sort_keys(uint64_t* keys, int np2, int tid)
{
    uint64_t x[E];
    const bool active = tid * E < np2;
#pragma unroll
    for (int u = 0; u < E; ++u) x[u] = active ? keys[tid * E + u] : 0ull;
    bool lds_dirty = false;
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < E) {
#pragma unroll
                for (int jj = E / 2; jj >= 1; jj >>= 1) {  // compile-time register indices
                    if (jj != j) continue;
#pragma unroll
                    for (int u = 0; u < E; ++u) {
                        if (u & jj) continue;
                        const int e = tid * E + u;
                        const bool desc = (e & k) == 0;
                        const uint64_t p = x[u], q = x[u | jj];
                        const bool sw = desc ? p < q : p > q;
                        x[u] = sw ? q : p;
                        x[u | jj] = sw ? p : q;
                    }
                }
            } else if (j < 64 * E) {
                const int d = j / E;
                const bool lower = (tid & d) == 0;
#pragma unroll
                for (int u = 0; u < E; ++u) {
                    const uint64_t y = shfl_xor_u64(x[u], d);
                    const int e = tid * E + u;
                    const bool desc = (e & k) == 0;
                    const bool take_max = lower == desc;
                    x[u] = take_max ? (x[u] > y ? x[u] : y) : (x[u] < y ? x[u] : y);
                }
            } else {
                if (lds_dirty) __syncthreads();  // previous LDS stage's reads are done
                if (active)
#pragma unroll
                    for (int u = 0; u < E; ++u) keys[tid * E + u] = x[u];
                __syncthreads();
                if (active)
#pragma unroll
                    for (int u = 0; u < E; ++u) {
                        const int e = tid * E + u;
                        const uint64_t y = keys[e ^ j];
                        const bool desc = (e & k) == 0;
                        const bool take_max = ((e & j) == 0) == desc;
                        x[u] = take_max ? (x[u] > y ? x[u] : y) : (x[u] < y ? x[u] : y);
                    }
                lds_dirty = true;
            }
        }
    }
    __syncthreads();
    if (active)
#pragma unroll
        for (int u = 0; u < E; ++u) keys[tid * E + u] = x[u];
    __syncthreads();
}

// Bitonic sort of np2 keys in LDS only (every stage a compare-exchange pass
// over LDS pairs): the path for ROIs with more than 4 * kSelThreads candidates.
// Slower than sort_keys, but it keeps the kernel's register footprint at that
// of sort_keys<4> (the register-resident sorts of 8-32 keys per thread needed
// 169 VGPRs, which made every select workgroup wait for PyrLK waves to drain).
__device__ __forceinline__ void sort_keys_lds(uint64_t* keys, int np2, int tid)
{
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < np2 / 2; p += kSelThreads) {
                const int e = ((p & ~(j - 1)) << 1) | (p & (j - 1));  // lower element of the pair
                const uint64_t x = keys[e], y = keys[e | j];
                const bool desc = (e & k) == 0;
                if (desc ? x < y : x > y) {
                    keys[e] = y;
                    keys[e | j] = x;
                }
            }
            __syncthreads();
        }
    }
}

// wave 0: the bin where the running count from the top first reaches target,
// and the count of keys in the bins above it (hist: 256 bins in LDS)
__device__ __forceinline__ void radix_pick(const int* hist, int target, int lane, int* out_bin, int* out_above)
{
    int h[4], t = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        h[u] = hist[4 * lane + u];
        t += h[u];
    }
    int suf = t;  // inclusive suffix sum over lanes >= lane
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(suf, d, 64);
        suf += lane + d < 64 ? o : 0;
    }
    int above = suf - t;  // keys in the bins of the lanes above
    if (above < target && suf >= target) {
#pragma unroll
        for (int u = 3; u >= 0; --u) {
            if (above + h[u] >= target) {
                *out_bin = 4 * lane + u;
                *out_above = above;
                break;
            }
            above += h[u];
        }
    }
}

}  // namespace tbdk
