// klt_gftt_wide.hip — the second ("wide") selection path of goodFeaturesToTrack
// for gfx950: ROIs whose candidates or accepted corners do not fit the LDS of
// gftt_select_kernel (klt_gftt.hip), whole frames above all.  Same semantics
// (imgproc/src/featureselect.cpp:361-516): threshold-to-zero at
// (float)(maxVal * q), 3x3 dilate-equal test on interior pixels, descending
// order of cand_key (value, then address), greedy min-distance acceptance,
// stop at max_corners.  The eigenvalue / response stage is the LDS path's.
//
// Three launches after it, all ROIs of the call batched in each; a ROI takes
// part when the LDS select reported overflow for it (counts[r] == -1), or
// always when the host routes the whole call here (GfttWide::all):
//   1. gftt_wide_gather: kWideParts workgroups per ROI.  From the
//      local-maximum words, the values and the strip maxima they apply the
//      select kernel's threshold and mask rules and append every candidate's
//      key to the ROI's key array in global scratch (one atomic per wave).
//      The order the keys land in depends on the atomics; nothing after it
//      does.  They also clear the ROI's cell grid.
//   2. gftt_wide_partition: one 512-thread workgroup per ROI with more keys than
//      one chunk (kWideChunk).  Every key lies between the threshold's and the
//      maximum's keys, so only the bits below their common prefix tell keys
//      apart; the ROI's keys are partitioned by the first kWideBinBits of those
//      bits into buckets, largest first (histogram, scan, scatter into the ROI's
//      second key array; the bucket ends into the start of the first).
//   3. gftt_wide_walk: one 512-thread workgroup per ROI.  It never sorts the
//      array: it pulls descending chunks that fit LDS, the next buckets that
//      together stay within what it still needs (between one and two times the
//      corners still missing, 512 at least), read from their own place only, so
//      a call that stops at max_corners sorts only what it consumes.  One bucket
//      larger than that (ties), or the unpartitioned array of a ROI of at most
//      one chunk, is split by a radix select over 256-bin LDS histograms of its
//      own keys, down to single keys if need be.  Each chunk is sorted by the
//      LDS path's sort_keys* and walked by one wave, 64 candidates per step with
//      that path's in-step dependency resolution.
//      Accepted corners live in a cell grid in global scratch.  The cell side
//      (gftt_wide_geometry, on the host) is the largest s with
//      2 (s-1)^2 < min_distance^2: any two pixels of a cell are closer than
//      min_distance, so a cell holds at most one corner, and the pixels closer
//      than min_distance to a candidate lie in at most 5 x 5 cells (radius <
//      min_distance <= sqrt(2) s).  The test of one candidate is 25 loads
//      whatever min_distance and however many corners are accepted.  Without a
//      distance test (min_distance < 1) a sorted chunk is written out by the
//      whole workgroup.  No loop in these kernels is bounded by min_distance.
// Built with -ffp-contract=off like the rest.
#include <cmath>

#include "klt_gftt_device.hpp"
#include "tbdk_internal.hpp"

namespace tbdk {

constexpr int kWideThreads = 256;  // gather workgroup
constexpr int kWideChunk = 4096;   // keys per sorted LDS chunk
constexpr int kWideBinBits = 11;   // buckets of a ROI with more keys than a chunk
constexpr int kWideBins = 1 << kWideBinBits;

// the ROI's part in this launch: routed here by the host, or by the LDS select's overflow report
__device__ __forceinline__ bool wide_takes(const GfttArgs& a, const GfttWide& w, int r)
{
    return w.all != 0 || a.counts[r] == -1;
}

template <bool masked>
__global__ __launch_bounds__(kWideThreads) void gftt_wide_gather_kernel(GfttArgs a, GfttWide w)
{
    const int r = blockIdx.x / kWideParts, part = blockIdx.x - r * kWideParts;
    if (!wide_takes(a, w, r)) return;
    const GfttRoi R = roi_at(a, r);
    const int tid = threadIdx.x, lane = tid & 63;
    const int gt = part * kWideThreads + tid, gn = kWideParts * kWideThreads;  // this thread among the ROI's
    // the cell grid of the walk, cleared (at most one cell per ROI pixel)
    if (w.rad >= 0) {  // a distance test (min_distance >= 1)
        const int nc = ((R.w + w.cell - 1) / w.cell) * ((R.h + w.cell - 1) / w.cell);
        uint32_t* cells = w.cells + R.off;
        for (int i = gt; i < nc; i += gn) cells[i] = 0u;
    }
    if (R.w < 3 || R.h < 3) return;  // no interior pixel: the count stays 0
    // ROI max and threshold as gftt_select_kernel has them
    const int nstrip = (R.w + kGfttStrip - 1) / kGfttStrip;
    int mk = INT_MIN;
    for (int b = R.cblk; b < R.cblk + nstrip; ++b) mk = a.blk_max[b] > mk ? a.blk_max[b] : mk;
    const float roi_max = masked && mk == INT_MIN ? 0.f : fkey_inv(mk);
    const float thr = (float)((double)roi_max * a.quality);
    GfttWideState* st = w.state + r;
    if (gt == 0) {
        st->thr = thr;
        st->vmax = roi_max;
    }
    uint64_t* keys = w.keys + R.off;
    const int kcap = (R.w - 2) * (R.h - 2);  // every candidate is an interior pixel of its own
    const float* Ep = a.eig + R.off;
    const uint8_t* Mp = masked ? a.mask + (size_t)R.y * a.mask_pitch + R.x : nullptr;
    const int ep = gftt_epitch(R.w);
    // this thread's n keys get consecutive places in the ROI's array: one atomic per wave
    auto place = [&](int n) {
        int inc = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            inc += lane >= d ? o : 0;
        }
        const int tot = __shfl(inc, 63, 64);
        int base = 0;
        if (lane == 0 && tot > 0) base = atomicAdd(&st->total, tot);
        return __shfl(base, 0, 64) + inc - n;
    };
    if (thr > 0.f) {
        const int nw = nstrip * R.h;
        for (int w0 = 0; w0 < nw; w0 += gn) {  // wave-uniform trip count
            const int wi = w0 + gt;
            const int sx = wi / R.h, y = wi - sx * R.h;
            const bool live = wi < nw && y >= 1 && y <= R.h - 2;  // rows 0 and h-1 have no word
            const uint64_t word = live ? a.lmax[R.moff + wi] : 0ull;
            const float* Er = Ep + (size_t)y * ep + sx * kGfttStrip - kGfttHalo;
            const float* Ec = Er + kGfttHalo;  // compact: the word's values packed in bit order
            const uint8_t* Mr = masked ? Mp + (size_t)y * a.mask_pitch + sx * kGfttStrip - kGfttHalo : nullptr;
            uint64_t in = 0ull;  // the word's bits that are candidates
            {
                uint64_t t = word;
                int rk = 0;
                while (t) {
                    const int x = __builtin_ctzll(t);
                    t &= t - 1ull;
                    const float v = a.compact ? Ec[rk] : Er[x];
                    ++rk;
                    bool ok = v > thr;
                    if constexpr (masked) ok = ok && Mr[x] != 0;
                    if (ok) in |= 1ull << x;
                }
            }
            int q = place(__popcll(in));
            while (in) {
                const int x = __builtin_ctzll(in);
                in &= in - 1ull;
                const float v = a.compact ? Ec[__popcll(word & ((1ull << x) - 1ull))] : Er[x];
                if (q < kcap) keys[q] = cand_key(v, y, sx * kGfttStrip + x - kGfttHalo);
                ++q;
            }
        }
    } else if (!a.compact) {
        // thr <= 0: the literal test (see gftt_select_kernel; compact launches have no candidate here)
        const int iw = R.w - 2, n = iw * (R.h - 2);
        for (int p0 = 0; p0 < n; p0 += gn) {
            const int p = p0 + gt;
            bool is = false;
            float v = 0.f;
            int x = 0, y = 0;
            if (p < n) {
                y = p / iw + 1;
                x = p - (y - 1) * iw + 1;
                const float* Ec = Ep + (size_t)y * ep + x;
                v = Ec[0] > thr ? Ec[0] : 0.f;
                is = v != 0.f;
                if constexpr (masked) is = is && Mp[(size_t)y * a.mask_pitch + x] != 0;
                if (is) {
                    float m = v;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const float q0 = Ec[dy * ep + dx];
                            const float q = q0 > thr ? q0 : 0.f;
                            m = q > m ? q : m;
                        }
                    is = v == m;
                }
            }
            const int q = place(is ? 1 : 0);
            if (is && q < kcap) keys[q] = cand_key(v, y, x);
        }
    }
}

// one pass of the walk's workgroup over a ROI's n keys, eight loads in flight per thread
template <typename F>
__device__ __forceinline__ void scan_keys(const uint64_t* __restrict__ keys, int n, int tid, F f)
{
    constexpr int U = 8;
    int i = tid;
    for (; i + (U - 1) * kSelThreads < n; i += U * kSelThreads) {
        uint64_t k[U];
#pragma unroll
        for (int u = 0; u < U; ++u) k[u] = keys[i + u * kSelThreads];
#pragma unroll
        for (int u = 0; u < U; ++u) f(k[u]);
    }
    for (; i < n; i += kSelThreads) f(keys[i]);
}

// The key range of a ROI: every key lies in [kmin, kmax] (thr < value <= ROI
// max), so in [L0, L0 + 2^wbits) with wbits the first bit in which the two differ
struct WideRange {
    uint64_t L0;
    int wbits;  // >= 32: the position bits differ
};
__device__ __forceinline__ WideRange wide_range(float thr, float vmax)
{
    const uint64_t kmin = cand_key(thr, 0, 0), kmax = cand_key(vmax, 0xFFFF, 0xFFFF);
    WideRange g;
    g.wbits = 64 - __builtin_clzll(kmin ^ kmax);
    g.L0 = g.wbits >= 64 ? 0ull : (kmin >> g.wbits) << g.wbits;
    return g;
}

// A ROI with more keys than one chunk: partitioned once by the top kWideBinBits
// bits below the common prefix, largest bucket first, into the ROI's second key
// array (histogram, scan, scatter; one workgroup per ROI).  The bucket ends
// (bucket d starts where d - 1 ends) go to the start of the ROI's first key
// array, which nothing reads after this: more than kWideChunk keys, so room for
// kWideBins ints.  A pull of the walk then reads its own buckets only.
__global__ __launch_bounds__(kSelThreads) void gftt_wide_partition_kernel(GfttArgs a, GfttWide w)
{
    __shared__ int pos[kWideBins];
    __shared__ int s_wsum[kSelThreads / 64];
    const int r = blockIdx.x;
    if (!wide_takes(a, w, r)) return;
    const GfttRoi R = roi_at(a, r);
    const int tid = threadIdx.x, lane = tid & 63;
    const GfttWideState st = w.state[r];
    const int total = min(st.total, max(0, (R.w - 2) * (R.h - 2)));
    if (total <= kWideChunk) return;
    uint64_t* keys = w.keys + R.off;
    uint64_t* keys2 = w.keys2 + R.off;
    const WideRange g = wide_range(st.thr, st.vmax);
    const uint64_t L0 = g.L0;
    const int sh1 = g.wbits - kWideBinBits;
    auto bucket = [&](uint64_t k) { return kWideBins - 1 - (int)min((k - L0) >> sh1, (uint64_t)(kWideBins - 1)); };
    for (int i = tid; i < kWideBins; i += kSelThreads) pos[i] = 0;
    __syncthreads();
    scan_keys(keys, total, tid, [&](uint64_t k) { atomicAdd(&pos[bucket(k)], 1); });
    __syncthreads();
    {  // exclusive scan: kWideBins / kSelThreads buckets per thread, waves, workgroup
        constexpr int PT = kWideBins / kSelThreads;
        int c[PT], sum = 0;
#pragma unroll
        for (int u = 0; u < PT; ++u) {
            c[u] = pos[tid * PT + u];
            sum += c[u];
        }
        int inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            inc += lane >= d ? o : 0;
        }
        if (lane == 63) s_wsum[tid >> 6] = inc;
        __syncthreads();
        int ex = inc - sum;
        for (int v = 0; v < (tid >> 6); ++v) ex += s_wsum[v];
#pragma unroll
        for (int u = 0; u < PT; ++u) {
            pos[tid * PT + u] = ex;
            ex += c[u];
        }
    }
    __syncthreads();
    scan_keys(keys, total, tid, [&](uint64_t k) {
        const int q = atomicAdd(&pos[bucket(k)], 1);
        if (q < total) keys2[q] = k;
    });
    __syncthreads();  // every read of keys is done: its start now holds the bucket ends
    int* ends = reinterpret_cast<int*>(keys);
    for (int i = tid; i < kWideBins; i += kSelThreads) ends[i] = pos[i];
}

// The walk kernel holds more wave-uniform state than the scalar registers take
// (the segment and the radix select around the chunk loop, the ROI and the
// grid inside it, the step's 64-bit lane masks).  Values that only enter
// per-lane arithmetic are therefore kept in vector registers, of which the
// kernel has room to spare: passing through an empty asm with a "v" constraint
// makes the compiler treat them as per-lane values.
// ... and values every lane reads from LDS alike, which steer the control flow,
// are declared uniform, so that the branches on them stay scalar
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T>
__device__ __forceinline__ T in_vgpr(T v)
{
    asm volatile("" : "+v"(v));
    return v;
}
template <typename T>
__device__ __forceinline__ T* in_vgpr(T* p)
{
    uint64_t v = reinterpret_cast<uint64_t>(p);
    asm volatile("" : "+v"(v));
    return reinterpret_cast<T*>(v);
}

// The walk.  LDS: the chunk's keys, the bucket ends, the radix histogram, a few words.
// four waves per SIMD, i.e. at most 128 VGPRs: two of these workgroups, or other kernels' waves, fit beside one
__global__ __launch_bounds__(kSelThreads) __attribute__((amdgpu_waves_per_eu(4))) void gftt_wide_walk_kernel(GfttArgs a,
                                                                                                          GfttWide w)
{
    __shared__ __attribute__((aligned(16))) uint64_t lk[kWideChunk];
    __shared__ int hist[256];
    __shared__ int s_pick[2];  // the radix pass's bin and the keys above it
    __shared__ int s_cnt, s_n, s_done;
    __shared__ int pos[kWideBins];  // bucket ends of a partitioned key array
    __shared__ int s_seg[2];
    const int r = blockIdx.x;
    if (!wide_takes(a, w, r)) return;
    const GfttRoi R = roi_at(a, r);
    const int tid = threadIdx.x;
    const GfttWideState st = w.state[r];
    const int total = min(st.total, max(0, (R.w - 2) * (R.h - 2)));
    // read once, here: nothing below goes back to the arguments or the ROI table
    const WideRange kr = wide_range(st.thr, st.vmax);
    const uint64_t L0 = in_vgpr(kr.L0);
    const int wbits = in_vgpr(kr.wbits);
    const uint64_t* keys = in_vgpr(w.keys + R.off);
    const uint64_t* keys2 = in_vgpr(w.keys2 + R.off);
    int32_t* count = in_vgpr(a.counts + r);
    uint32_t* cells = in_vgpr(w.cells + R.off);
    const bool use_dist = w.rad >= 0;  // the host's (min_distance >= 1)
    const double md2 = in_vgpr(a.min_distance * a.min_distance);
    const int cell = in_vgpr(w.cell), rad = in_vgpr(w.rad), rw = in_vgpr(R.w), rh = in_vgpr(R.h);
    const int gw = in_vgpr((R.w + w.cell - 1) / w.cell), gh = in_vgpr((R.h + w.cell - 1) / w.cell);
    const float rx = in_vgpr((float)R.x), ry = in_vgpr((float)R.y);
    const int maxc = a.max_corners;
    float2* out = in_vgpr(a.corners + (size_t)r * a.corner_stride);
    const bool bucketed = total > kWideChunk;  // partitioned by gftt_wide_partition_kernel
    if (bucketed) {
        const int* ends = reinterpret_cast<const int*>(keys);
        for (int i = tid; i < kWideBins; i += kSelThreads) pos[i] = ends[i];
        __syncthreads();
    }

    // The current segment: sn keys at sk, all within [sL, sL + sspan], the radix
    // select's first level at shift ssh.  Not bucketed: the ROI's whole array, once.
    // Bucketed: the next buckets that together stay within the target, or one
    // bucket alone, which the radix select then splits.
    const uint64_t* sk = nullptr;
    int sn = 0, ssh = 0, dcur = 0;
    uint64_t sL = 0ull, sspan = 0ull;
    bool first = true;
    int n = 0, remaining = 0;
    uint64_t hi = ~0ull;  // the segment's keys >= hi are consumed
    while (n < maxc) {
        // the thread id afresh in every round: the lane masks of its tests (tid == 0,
        // tid < 64, the sorts' and the pick's lane tests) then live inside the round
        // only, not in scalar register pairs across the whole loop
        const int t = in_vgpr(tid), tl = t & 63;
        const int need = maxc - n;
        // a chunk is at least half its target, so without a distance test one chunk of
        // target >= 2 need serves; with one, more chunks follow as corners are rejected
        const int target = need >= kWideChunk / 2 ? kWideChunk : max(2 * need, kSelThreads);
        if (remaining == 0) {  // the next segment
            if (!bucketed) {
                if (!first || total == 0) break;
                first = false;
                sk = keys;
                sn = total;
                sL = L0;
                sspan = in_vgpr(wbits >= 64 ? ~0ull : ((1ull << wbits) - 1ull));
                ssh = wbits - 8;
            } else {
                if (t == 0) {
                    int d = dcur, prev = d ? pos[d - 1] : 0;
                    while (d < kWideBins && pos[d] == prev) ++d;  // empty buckets
                    s_seg[0] = d;
                    if (d < kWideBins) {
                        ++d;  // the first bucket whatever its size
                        while (d < kWideBins && pos[d] - prev <= target) ++d;
                    }
                    s_seg[1] = d;
                }
                __syncthreads();
                const int d0 = uni(s_seg[0]), d1 = uni(s_seg[1]);
                __syncthreads();
                if (d0 >= kWideBins) break;
                const int start = d0 ? uni(pos[d0 - 1]) : 0;
                sk = keys2 + start;
                sn = min(uni(pos[d1 - 1]), total) - start;
                // the bucket's own range, should the radix select have to split it: only a
                // segment of one bucket can exceed the target (several together never do)
                const int sh1 = wbits - kWideBinBits;
                sL = L0 + ((uint64_t)(kWideBins - 1 - d0) << sh1);
                sspan = in_vgpr((1ull << sh1) - 1ull);
                ssh = sh1 >= 8 ? sh1 - 8 : 0;
                dcur = d1;
            }
            remaining = sn;
            hi = in_vgpr(~0ull);
            if (sn <= 0) break;  // (unreachable)
        }
        // ---- the next chunk: the segment's keys in [lo, hi), at most target of them, at least one
        uint64_t lo = in_vgpr(0ull);
        int cnt = remaining;
        if (remaining > target) {
            uint64_t L = sL, span = sspan;  // the level covers [L, L + span]
            int sh = ssh, tgt = target, acc = 0;  // acc: keys above the level, all taken
            for (;;) {
                if (t < 256) hist[t] = 0;
                if (t == 0) s_pick[0] = -1;
                __syncthreads();
                scan_keys(sk, sn, t, [&](uint64_t k) {
                    if (k < hi && k >= L && k - L <= span) atomicAdd(&hist[(int)min((k - L) >> sh, (uint64_t)255)], 1);
                });
                __syncthreads();
                if (t < 64) radix_pick(hist, tgt, t, &s_pick[0], &s_pick[1]);
                __syncthreads();
                const int bin = uni(s_pick[0]), above = uni(s_pick[1]);
                if (bin < 0) {  // fewer than tgt keys in the bins (cannot happen: remaining > target): take them all
                    lo = L;
                    cnt = 0;
                    for (int b = 0; b < 256; ++b) cnt += hist[b];
                    cnt += acc;
                    __syncthreads();
                    break;
                }
                const int hb = uni(hist[bin]);
                __syncthreads();  // hist is cleared by the next pass
                if (above + hb == tgt) {  // the bin completes the target exactly
                    lo = L + ((uint64_t)bin << sh);
                    cnt = acc + above + hb;
                    break;
                }
                if (2 * (acc + above) >= target || sh == 0) {  // the bins above it are chunk enough
                    // bin 255 has nothing above it, so bin + 1 stays inside the level's span
                    lo = L + ((uint64_t)(bin + 1) << sh);
                    cnt = acc + above;
                    break;
                }
                L += (uint64_t)bin << sh;  // into the bin: its keys alone, in bins 1/256 as wide
                span = (1ull << sh) - 1ull;
                acc += above;
                tgt -= above;
                sh = sh >= 8 ? sh - 8 : 0;
            }
        }
        if (cnt <= 0 || cnt > kWideChunk) break;  // (unreachable by the selection above)
        // ---- into LDS, sorted
        if (t == 0) s_cnt = 0;
        __syncthreads();
        scan_keys(sk, sn, t, [&](uint64_t k) {
            if (k < hi && k >= lo) {
                const int q = atomicAdd(&s_cnt, 1);
                if (q < kWideChunk) lk[q] = k;
            }
        });
        __syncthreads();
        cnt = uni(min(s_cnt, kWideChunk));
        int np2 = kSelThreads;
        while (np2 < cnt) np2 <<= 1;
        for (int i = cnt + t; i < np2; i += kSelThreads) lk[i] = 0ull;  // sorts last
        __syncthreads();
        switch (np2 / kSelThreads) {
        case 1: sort_keys<1>(lk, np2, t); break;
        case 2: sort_keys<2>(lk, np2, t); break;
        case 4: sort_keys<4>(lk, np2, t); break;
        default: sort_keys_lds(lk, np2, t); break;
        }
        __syncthreads();
        // ---- consume
        if (!use_dist) {  // every candidate is accepted, in order
            const int m = min(cnt, need);
            for (int i = t; i < m; i += kSelThreads) {
                const uint32_t kk = (uint32_t)lk[i];
                out[n + i] = make_float2((float)(int)(kk & 0xFFFF) + rx, (float)(int)(kk >> 16) + ry);
            }
            n += m;
        } else {
            if (t < 64) {
                bool done = false;
                for (int i0 = 0; i0 < cnt && !done; i0 += 64) {
                    const int i = i0 + tl;
                    const bool valid = i < cnt;
                    const uint32_t kk = valid ? (uint32_t)lk[i] : 0u;
                    const int ix = (int)(kk & 0xFFFF), iy = (int)(kk >> 16);
                    const float fx = (float)ix, fy = (float)iy;
                    // accepted corners closer than min_distance: in the cells the window touches
                    const int cx0 = max(ix - rad, 0) / cell, cx1 = min(ix + rad, rw - 1) / cell;
                    const int cy0 = max(iy - rad, 0) / cell, cy1 = min(iy + rad, rh - 1) / cell;
                    uint32_t cv[25];
#pragma unroll
                    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 5; ++dx) {
                            const int cy = cy0 + dy, cx = cx0 + dx;
                            const bool in = valid && cy <= cy1 && cx <= cx1;
                            const int ci = in ? cy * gw + cx : 0;  // cell 0 exists (a grid has >= 1 cell)
                            const uint32_t c = __hip_atomic_load(cells + ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            cv[dy * 5 + dx] = in ? c : 0u;
                        }
                    bool good = valid;
#pragma unroll
                    for (int j = 0; j < 25; ++j) {
                        const uint32_t c = cv[j] - 1u;  // ((y << 16) | x) + 1, 0: empty
                        const float dx = fx - (float)(int)(c & 0xFFFF), dy = fy - (float)(int)(c >> 16);
                        if (cv[j] != 0u && (double)(dx * dx + dy * dy) < md2) good = false;
                    }
                    // this step's earlier candidates closer than min_distance (only those
                    // still good can be accepted, so only they can reject)
                    const unsigned long long goodm = __ballot(good);
                    unsigned long long inb = 0ull;
                    for (unsigned long long m = goodm; m;) {
                        const int j = __builtin_ctzll(m);
                        m &= m - 1ull;
                        const float dx = fx - (float)__builtin_amdgcn_readlane(ix, j);
                        const float dy = fy - (float)__builtin_amdgcn_readlane(iy, j);
                        if (j < tl && (double)(dx * dx + dy * dy) < md2) inb |= 1ull << j;
                    }
                    // sequential acceptance, as gftt_select_kernel: lanes without in-step
                    // dependencies are final; the others, in order, are accepted iff no
                    // accepted earlier tl conflicts
                    const unsigned long long depm = __ballot(good && inb != 0ull);
                    unsigned long long accm = goodm & ~depm;
                    unsigned long long pend = depm;
                    while (pend) {
                        const int k = __builtin_ctzll(pend);
                        pend &= pend - 1ull;
                        const unsigned long long ik =
                            ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(inb >> 32), k) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)inb, k);
                        if (!(ik & accm)) accm |= 1ull << k;
                    }
                    // maxCorners: only the first (maxc - n) accepted of this step count
                    const int got = __popcll(accm);
                    if (n + got >= maxc) {
                        int keepn = maxc - n;
                        unsigned long long m = accm, kept = 0ull;
                        while (keepn-- > 0) {
                            const unsigned long long low = m & (~m + 1ull);
                            kept |= low;
                            m &= m - 1ull;
                        }
                        accm = kept;
                        done = true;
                    }
                    if ((accm >> tl) & 1ull) {
                        const int pos = n + __popcll(accm & ((1ull << tl) - 1ull));
                        out[pos] = make_float2(fx + rx, fy + ry);
                        const int ci = min(iy / cell, gh - 1) * gw + min(ix / cell, gw - 1);
                        __hip_atomic_store(cells + ci, kk + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    n += __popcll(accm);
                    // the cells written are read by other lanes in the next step
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                }
                if (tl == 0) {
                    s_n = n;
                    s_done = done ? 1 : 0;
                }
            }
            __syncthreads();
            n = uni(s_n);
            if (uni(s_done)) break;
        }
        hi = lo;
        remaining -= cnt;
        __syncthreads();  // lk, s_cnt, s_n are rewritten by the next chunk
    }
    if (tid == 0) *count = n;
}

hipError_t launch_gftt_wide(const GfttArgs& a, const GfttWide& w, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(w.state, 0, sizeof(GfttWideState) * (size_t)a.nroi, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)a.nroi * kWideParts);
    if (a.mask) hipLaunchKernelGGL(gftt_wide_gather_kernel<true>, grid, dim3(kWideThreads), 0, s, a, w);
    else hipLaunchKernelGGL(gftt_wide_gather_kernel<false>, grid, dim3(kWideThreads), 0, s, a, w);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gftt_wide_partition_kernel, dim3(a.nroi), dim3(kSelThreads), 0, s, a, w);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gftt_wide_walk_kernel, dim3(a.nroi), dim3(kSelThreads), 0, s, a, w);
    return hipGetLastError();
}

}  // namespace tbdk
