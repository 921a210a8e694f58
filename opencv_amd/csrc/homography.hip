// homography.hip — tbdk_find_homography: cv::findHomography (method 0 and
// RANSAC) batched over point sets, one wave per set, nothing on the host.  The
// arithmetic is homography_core.hpp's; this file decides who computes what.
//
// The accepted 4-point subsets depend on the RNG and on checkSubset only, never
// on an evaluation (evaluations only shorten the loop: niters never grows).  So
// the loop runs in batches of 64 iterations:
//   1. the wave draws the next min(64, niters - done) accepted subsets, every
//      lane running the same serial chain (wave-uniform);
//   2. lane j solves subset j's 4-point DLT, its Jacobi state in LDS;
//   3. lanes over points: the float error test of each hypothesis, ballot and
//      popcount per 64 pairs;
//   4. the batch is scanned in order with the reference's rule; the scan stops
//      at the first index >= niters and what was computed beyond it is dropped.
// Then the mask is written from the winning model, the inliers are compacted in
// place, lane e < 45 sums entry e of LtL over them in point order, one Jacobi
// gives the re-fit, and the LM step reduces its sums across the wave.
//
// LDS per workgroup (DESIGN.md §5 "findHomography"): the pairs (64 KB, 4096 of
// them), 64 solver columns (135 doubles each, entry e of lane l at double
// e * 64 + l, so a lane's bank pair depends on l alone and the data-dependent
// indices of the Jacobi never conflict), the batch's models and subsets.
#include "box_fit.hpp"
#include "homography_core.hpp"
#include "tbdk_internal.hpp"

namespace tbdk {

namespace {

namespace hc = homography_core;

constexpr int kCap = TBDK_HOMOGRAPHY_MAX_PAIRS;
constexpr int kBatch = 64;

struct LdsPairs {
    const float2 *s, *d;
    __device__ hc::Pt M(int i) const { return hc::Pt{s[i].x, s[i].y}; }
    __device__ hc::Pt m(int i) const { return hc::Pt{d[i].x, d[i].y}; }
};

// the four pairs of one lane's subset: sub[i * 64] is its i-th index
struct SubsetPairs {
    const float2 *s, *d;
    const int* sub;
    __device__ hc::Pt M(int i) const { return hc::Pt{s[sub[i * kBatch]].x, s[sub[i * kBatch]].y}; }
    __device__ hc::Pt m(int i) const { return hc::Pt{d[sub[i * kBatch]].x, d[sub[i * kBatch]].y}; }
};

__device__ __forceinline__ double wave_max_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// the LM step's sums over the inliers: lane l takes pairs l, l + 64, ..., a
// fixed butterfly combines; the sums go to *cur in LDS (every lane writes the
// same values)
struct WaveSums {
    LdsPairs p;
    int n, lane;
    __device__ double operator()(const double* h, bool jac, hc::LmSums* cur) const
    {
        hc::LmSums part;
        hc::lm_zero(&part);
        for (int i = lane; i < n; i += 64) hc::lm_point(h, p.M(i), p.m(i), jac, &part);
        const double S = wave_sum_f64(part.S);
        if (!jac) return S;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 36; i++) cur->A[i] = wave_sum_f64(part.A[i]);
#pragma unroll
        for (int i = 0; i < 8; i++) cur->v[i] = wave_sum_f64(part.v[i]);
        cur->S = S;
        cur->rinf = wave_max_f64(part.rinf);
        __syncthreads();
        return S;
    }
};

// RANSACUpdateNumIters, kept out of line: inlined, log's and pow's constants are
// hoisted over the whole RANSAC loop and cost it scalar registers
__device__ __noinline__ int wave_update_num_iters(double confidence, double ep, int niters)
{
    return hc::update_num_iters(confidence, ep, niters, nullptr);
}

// runKernel on pairs [0, n) by the whole wave: the centroid and deviation sums
// walk the pairs in order (every lane the same), lane e < 45 sums entry e of
// LtL in point order, every lane then runs the same Jacobi on its own column.
// `xchg` is 45 doubles of LDS.  False where runKernel returns 0 (H untouched).
__device__ bool wave_run_kernel(const LdsPairs& pairs, int n, const hc::Ws& ws, double* xchg, int lane, double* H)
{
    hc::Norm nm;
    if (!hc::normalize(pairs, n, &nm)) return false;
    int j = 0, k = lane < 45 ? lane : 0;
    while (k >= 9 - j) k -= 9 - j, ++j;
    k += j;
    double acc = 0;
    if (lane < 45)
        for (int i = 0; i < n; i++) acc += hc::ltl_term(j, k, nm, pairs.M(i), pairs.m(i));
    if (lane < 45) xchg[lane] = acc;
    __syncthreads();
    for (int e = 0; e < 45; ++e) ws.at(e) = xchg[e];
    __syncthreads();
    hc::solve_ltl(ws, nm, H);
    return true;
}

__global__ __launch_bounds__(64) void find_homography_kernel(
    const float2* __restrict__ src, const float2* __restrict__ dst, const uint8_t* __restrict__ status,
    const int32_t* __restrict__ offsets, int nsets, int method, double thr, int max_iters, double confidence,
    int refine, tbdk_homography* __restrict__ out, uint8_t* __restrict__ mask)
{
    __shared__ float2 sa[kCap], sb[kCap];
    __shared__ double wsm[hc::kWsDoubles * 64];
    __shared__ double hyp[kBatch * 9];
    __shared__ int sub[4 * kBatch];
    __shared__ int hok[kBatch];
    const int e = blockIdx.x;
    if (e >= nsets) return;
    const int lane = threadIdx.x;
    const int beg = offsets[e], end = offsets[e + 1];
    int m = 0;
    for (int j0 = beg; j0 < end; j0 += 64) {
        const int j = j0 + lane;
        const bool ok = j < end && (status == nullptr || status[j]);
        const unsigned long long bal = __ballot(ok);
        const int pos = m + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        if (ok && pos < kCap) {
            sa[pos] = src[j];
            sb[pos] = dst[j];
        }
        m += __popcll(bal);
    }
    __syncthreads();
    const bool over = m > kCap;  // never truncated: the set reports npoints = -1
    const int n = over ? 0 : m;
    const hc::Ws ws{wsm + lane, 64};
    const LdsPairs all{sa, sb};
    const float t = hc::inlier_bound(thr);
    double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int iters = 0, ninl = 0;
    bool have = false;
    const bool ransac = n > 4 && method == TBDK_HOMOGRAPHY_RANSAC;
    // the mask, each byte once: under RANSAC the model's inliers, else every status != 0 pair of a fitted set
    auto write_mask = [&](const hc::ModelF& mf) {
        int pos0 = 0;
        for (int j0 = beg; j0 < end; j0 += 64) {
            const int j = j0 + lane;
            const bool ok = j < end && (status == nullptr || status[j]);
            const unsigned long long bal = __ballot(ok);
            const int pos = pos0 + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
            if (j < end)
                mask[j] = (ok && have && (!ransac || hc::is_inlier(mf, t, all.M(pos), all.m(pos)))) ? 1 : 0;
            pos0 += __popcll(bal);
        }
    };
    if (ransac) {
        RansacRng rng;
        int niters = max_iters > 1 ? max_iters : 1, max_good = 0, base = 0;
        bool stop = false;
        while (base < niters && !stop) {
            // 1. the next accepted subsets (wave-uniform)
            const int nb = niters - base < kBatch ? niters - base : kBatch;
            int nsub = 0;
            for (; nsub < nb; ++nsub) {
                int i0, i1, i2, i3;
                if (!hc::get_subset(all, n, rng, &i0, &i1, &i2, &i3)) {
                    stop = true;
                    break;
                }
                if (lane == 0) {
                    sub[nsub] = i0;
                    sub[kBatch + nsub] = i1;
                    sub[2 * kBatch + nsub] = i2;
                    sub[3 * kBatch + nsub] = i3;
                }
            }
            __syncthreads();
            // 2. lanes over hypotheses
            if (lane < nsub) {
                const SubsetPairs sp{sa, sb, sub + lane};
                double Hh[9];
                const bool ok = hc::run_kernel(sp, 4, ws, Hh);
                hok[lane] = ok;
                if (ok) {
#pragma unroll
                    for (int i = 0; i < 9; i++) hyp[lane * 9 + i] = Hh[i];
                }
            }
            __syncthreads();
            // 3. lanes over points
            int mygood = 0;
            for (int j = 0; j < nsub; ++j) {
                if (!__builtin_amdgcn_readfirstlane(hok[j])) continue;
                const hc::ModelF mf = hc::model_f(hyp + j * 9);
                int good = 0;
                for (int c0 = 0; c0 < n; c0 += 64) {
                    const int i = c0 + lane;
                    good += __popcll(__ballot(i < n && hc::is_inlier(mf, t, all.M(i), all.m(i))));
                }
                if (lane == j) mygood = good;
            }
            // 4. the serial scan, the reference's rule
            for (int j = 0; j < nsub && base + j < niters; ++j) {
                iters = base + j + 1;
                const int good = __shfl(mygood, j, 64);
                if (!__builtin_amdgcn_readfirstlane(hok[j])) continue;
                if (good > (max_good > 3 ? max_good : 3)) {
                    max_good = good;
#pragma unroll
                    for (int i = 0; i < 9; i++) H[i] = hyp[j * 9 + i];
                    niters = wave_update_num_iters(confidence, (double)(n - good) / n, niters);
                }
            }
            base += nsub;
            __syncthreads();
        }
        have = max_good > 0;
        const hc::ModelF mf = hc::model_f(H);
        if (mask) write_mask(mf);
        if (have) {
            // the inliers, compacted in place in point order (a pair never moves up)
            int cnt = 0;
            for (int c0 = 0; c0 < n; c0 += 64) {
                const int i = c0 + lane;
                float2 a = make_float2(0.f, 0.f), b = a;
                if (i < n) a = sa[i], b = sb[i];
                const bool in = i < n && hc::is_inlier(mf, t, hc::Pt{a.x, a.y}, hc::Pt{b.x, b.y});
                const unsigned long long bal = __ballot(in);
                const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                                     __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                __syncthreads();
                if (in) sa[pos] = a, sb[pos] = b;
                cnt += __popcll(bal);
            }
            __syncthreads();
            ninl = cnt;
        }
    }
    // runKernel on all pairs (method 0, 4 pairs) or on the inliers; there a degenerate set keeps the RANSAC model
    const bool lsq = !ransac && n >= 4;
    if (lsq || (have && ninl > 0)) {
        const bool ok = wave_run_kernel(all, lsq ? n : ninl, ws, hyp, lane, H);
        if (lsq) have = ok, ninl = ok ? n : 0;
    }
    if (!ransac && mask) write_mask(hc::ModelF{});
    if (have && n > 4 && ninl > 0 && refine)
        hc::lm_refine(WaveSums{all, ninl, lane}, ws, reinterpret_cast<hc::LmSums*>(hyp), H);
    if (lane == 0) {
        tbdk_homography o;
#pragma unroll
        for (int i = 0; i < 9; i++) o.h[i] = H[i];
        o.npoints = over ? -1 : m;
        o.ninliers = ninl;
        o.iters = iters;
        o.valid = have ? 1 : 0;
        out[e] = o;
    }
}

}  // namespace

}  // namespace tbdk

using namespace tbdk;

extern "C" {

int tbdk_homography_default_params(tbdk_homography_params* p)
{
    if (!p) return TBDK_EINVAL;
    p->method = TBDK_HOMOGRAPHY_RANSAC;
    p->reproj_threshold = 3.0;
    p->max_iters = 2000;
    p->confidence = 0.995;
    p->refine = 1;
    return TBDK_OK;
}

int tbdk_find_homography(tbdk_ctx* ctx, const float* src_pts, const float* dst_pts, const uint8_t* status,
                         const int32_t* offsets, int nsets, const tbdk_homography_params* params,
                         tbdk_homography* out, uint8_t* mask, void* stream)
{
    if (!ctx || nsets < 0 || !params) return TBDK_EINVAL;
    if (params->method != TBDK_HOMOGRAPHY_LSQ && params->method != TBDK_HOMOGRAPHY_RANSAC) return TBDK_EINVAL;
    if (params->max_iters < 1 || params->max_iters > 10000) return TBDK_EINVAL;
    // the reference asserts confidence in (0, 1); a NaN threshold has no meaning
    if (!(params->confidence > 0.0 && params->confidence < 1.0) || params->reproj_threshold != params->reproj_threshold)
        return TBDK_EINVAL;
    if (params->refine != 0 && params->refine != 1) return TBDK_EINVAL;
    if (nsets == 0) return TBDK_OK;
    if (!src_pts || !dst_pts || !offsets || !out) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double thr = params->reproj_threshold <= 0 ? 3.0 : params->reproj_threshold;
    const int rec = timing_begin(ctx, "find_homography", s);
    hipLaunchKernelGGL(find_homography_kernel, dim3(nsets), dim3(64), 0, s, reinterpret_cast<const float2*>(src_pts),
                       reinterpret_cast<const float2*>(dst_pts), status, offsets, nsets, params->method, thr,
                       params->max_iters, params->confidence, params->refine, out, mask);
    const hipError_t e = hipGetLastError();
    timing_end(ctx, rec, s);
    return e == hipSuccess ? TBDK_OK : (e == hipErrorOutOfMemory ? TBDK_ENOMEM : TBDK_EHIP);
}

}  // extern "C"
