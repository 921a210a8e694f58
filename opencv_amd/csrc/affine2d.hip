// affine2d.hip — tbdk_estimate_affine_2d: cv::estimateAffine2D and
// cv::estimateAffinePartial2D (RANSAC and LMEDS) batched over point sets, one
// workgroup of four waves per set, nothing on the host.  The arithmetic is
// affine2d_core.hpp's; this file decides who computes what.
//
// The accepted subsets depend on the RNG and on checkSubset only, never on an
// evaluation (evaluations only shorten RANSAC's loop; LMEDS's count is fixed up
// front).  So the loop runs in batches of 64 iterations:
//   1. every thread draws the next min(64, niters - done) accepted subsets, all
//      running the same serial chain; thread j keeps subset j;
//   2. thread j solves subset j in closed form (no Jacobi per hypothesis);
//   3. wave w takes hypotheses w, w + 4, ...: lanes over points, the float
//      error of each pair; RANSAC counts the inliers by ballot, LMEDS keeps the
//      errors in the wave's own LDS strip and selects the element of rank
//      count/2 by a radix select over the bit patterns, one ballot count per bit;
//   4. every thread scans the batch in order with the reference's rule; the scan
//      stops at the first index >= niters and what lies beyond it is dropped.
// Then the mask is written from the winning model, the inliers are compacted in
// place, and the LM step runs with its sums reduced over the block in a fixed
// order and its 6x6 or 4x4 eigen solve on one thread.
//
// LDS per workgroup (DESIGN.md §5 "estimateAffine2D"): the pairs (64 KB, 4096
// of them), four error strips (64 KB), the batch's models and scores, the LM
// step's sums and one solver column.
#include "affine2d_core.hpp"
#include "box_fit.hpp"
#include "tbdk_internal.hpp"

namespace tbdk {

namespace {

namespace ac = affine2d_core;
namespace hc = homography_core;

constexpr int kCap = TBDK_AFFINE2D_MAX_PAIRS;
constexpr int kBatch = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct LdsPairs {
    const float2 *s, *d;
    __device__ hc::Pt M(int i) const { return hc::Pt{s[i].x, s[i].y}; }
    __device__ hc::Pt m(int i) const { return hc::Pt{d[i].x, d[i].y}; }
};

__device__ __forceinline__ double wave_max_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// The position of this thread among the block's flagged threads, in thread
// order, and their number.  Two barriers: after the first, whatever the caller
// read before the call has been read by every thread and `wc` is free.
__device__ __forceinline__ int block_prefix(bool flag, int* wc, int* total)
{
    const int w = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wc[w] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const int c = wc[k];
        off += k < w ? c : 0;
        tot += c;
    }
    *total = tot;
    return off + pos;
}

// RANSACUpdateNumIters, kept out of line (log's and pow's constants would be hoisted over the loop)
__device__ __noinline__ int block_update_num_iters(double confidence, double ep, int model_points, int niters)
{
    return ac::update_num_iters(confidence, ep, model_points, niters, nullptr);
}

// inliers of model `mf` among pairs [0, n), counted by one wave (every wave gets the same number)
__device__ __forceinline__ int wave_count_inliers(const LdsPairs& p, int n, const ac::ModelF& mf, float t, int lane)
{
    int good = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        good += __popcll(__ballot(i < n && ac::is_inlier(mf, t, p.M(i), p.m(i))));
    }
    return good;
}

// The LM step's parts that the block spreads: the sums over the inliers
// (thread t takes pairs t, t + 256, ...; a butterfly per wave, then the four
// waves' values added in wave order, so every thread holds the same sums), the
// eigen solve on thread 0 with its result passed through LDS.
template <int N>
struct BlockStep {
    static constexpr int K = N * (N + 1) / 2 + N + 2;  // the doubles of LmSums<N>
    LdsPairs p;
    int n;
    hc::Ws ws;
    double* red;  // kWaves * K
    double* xch;  // N

    __device__ double sums(const double* h, bool jac, ac::LmSums<N>* cur) const
    {
        const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
        ac::LmSums<N> part;
        ac::lm_zero(&part);
        for (int i = tid; i < n; i += kThreads) ac::lm_point<N>(h, p.M(i), p.m(i), jac, &part);
        double* pv = reinterpret_cast<double*>(&part);
        __syncthreads();  // red and *cur are free
        if (jac) {
#pragma unroll
            for (int k = 0; k < K - 1; ++k) {
                const double v = wave_sum_f64(pv[k]);
                if (lane == 0) red[w * K + k] = v;
            }
            const double r = wave_max_f64(part.rinf);
            if (lane == 0) red[w * K + K - 1] = r;
        } else {
            const double v = wave_sum_f64(part.S);
            if (lane == 0) red[w * K + K - 2] = v;
        }
        __syncthreads();
        double S = red[K - 2];
#pragma unroll
        for (int k = 1; k < kWaves; ++k) S += red[k * K + K - 2];
        if (jac) {
            double* cv = reinterpret_cast<double*>(cur);
            if (tid < K - 1) {
                double v = red[tid];
                for (int k = 1; k < kWaves; ++k) v += red[k * K + tid];
                cv[tid] = v;
            } else if (tid == K - 1) {
                double v = red[tid];
                for (int k = 1; k < kWaves; ++k) v = fmax(v, red[k * K + tid]);
                cv[tid] = v;
            }
            __syncthreads();
        }
        return S;
    }

    __device__ void solve(const ac::LmSums<N>* cur, const double* D, double lambda, double* d) const
    {
        if (threadIdx.x == 0) {
            double dd[N];
            ac::lm_solve<N>(ws, cur, D, lambda, dd);
#pragma unroll
            for (int i = 0; i < N; ++i) xch[i] = dd[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) d[i] = xch[i];
        __syncthreads();
    }

    __device__ double inv_diag_max(const ac::LmSums<N>* cur, const double* D) const
    {
        if (threadIdx.x == 0) xch[0] = ac::lm_inv_diag_max<N>(ws, cur, D);
        __syncthreads();
        const double v = xch[0];
        __syncthreads();
        return v;
    }
};

template <int MP>
__global__ __launch_bounds__(kThreads) void estimate_affine2d_kernel(
    const float2* __restrict__ src, const float2* __restrict__ dst, const uint8_t* __restrict__ status,
    const int32_t* __restrict__ offsets, int nsets, int method, double thr, int max_iters, double confidence,
    int refine_iters, tbdk_affine2d* __restrict__ out, uint8_t* __restrict__ mask)
{
    constexpr int N = MP == 3 ? 6 : 4;
    constexpr int K = BlockStep<N>::K;
    __shared__ float2 sa[kCap], sb[kCap];
    __shared__ float errs[kWaves * kCap];
    __shared__ double hyp[kBatch * 6];
    __shared__ double wsm[hc::kWsDoubles];
    __shared__ double curm[K];
    __shared__ double red[kWaves * K];
    __shared__ double xch[N];
    __shared__ int score[kBatch];
    __shared__ int wc[kWaves];
    const int e = blockIdx.x;
    if (e >= nsets) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int beg = offsets[e], end = offsets[e + 1];
    int m = 0;
    for (int j0 = beg; j0 < end; j0 += kThreads) {
        const int j = j0 + tid;
        const bool ok = j < end && (status == nullptr || status[j]);
        int tot;
        const int pos = m + block_prefix(ok, wc, &tot);
        if (ok && pos < kCap) {
            sa[pos] = src[j];
            sb[pos] = dst[j];
        }
        m += tot;
    }
    __syncthreads();
    const bool over = m > kCap;  // never truncated: the set reports npoints = -1
    const int n = over ? 0 : m;
    const LdsPairs all{sa, sb};
    const bool lmeds = method == TBDK_AFFINE2D_LMEDS;
    float t = ac::inlier_bound(thr);
    double M[6] = {1, 0, 0, 0, 1, 0};
    int iters = 0, ninl = 0;
    bool have = false, all_ones = false;
    if (n == MP) {
        // the kernel alone, mask all ones; a degenerate set gives the solver's NaN matrix, as in the reference
        const int idx[3] = {0, 1, 2};
        ac::run_kernel<MP>(all, idx, M);
        have = all_ones = true;
        ninl = n;
    } else if (n > MP) {
        RansacRng rng;
        int niters = lmeds ? ac::lmeds_num_iters(confidence, MP, max_iters, nullptr) : (max_iters > 1 ? max_iters : 1);
        const int max_attempts = lmeds ? ac::kMaxAttemptsLmeds : ac::kMaxAttemptsRansac;
        int max_good = 0, base = 0;
        double min_median = DBL_MAX;
        bool stop = false;
        while (base < niters && !stop) {
            // 1. the next accepted subsets (block-uniform); thread j keeps subset j
            const int nb = niters - base < kBatch ? niters - base : kBatch;
            int my[3] = {0, 0, 0};
            int nsub = 0;
            for (; nsub < nb; ++nsub) {
                int idx[3] = {0, 0, 0};
                if (!ac::get_subset<MP>(all, n, rng, max_attempts, idx)) {
                    stop = true;
                    break;
                }
                if (tid == nsub) my[0] = idx[0], my[1] = idx[1], my[2] = idx[2];
            }
            // 2. threads over hypotheses
            if (tid < nsub) {
                double Mh[6];
                ac::run_kernel<MP>(all, my, Mh);
#pragma unroll
                for (int i = 0; i < 6; i++) hyp[tid * 6 + i] = Mh[i];
            }
            __syncthreads();
            // 3. waves over hypotheses, lanes over points
            for (int j = w; j < nsub; j += kWaves) {
                const ac::ModelF mf = ac::model_f(hyp + j * 6);
                if (!lmeds) {
                    const int good = wave_count_inliers(all, n, mf, t, lane);
                    if (lane == 0) score[j] = good;
                } else {
                    // a lane reads back only what it wrote itself: no exchange between lanes goes through the strip
                    float* eb = errs + w * kCap;
                    for (int i = lane; i < n; i += 64) eb[i] = ac::reproj_error(mf, all.M(i), all.m(i));
                    const unsigned bits = ac::rank_select(
                        [&](unsigned msk, unsigned want) {
                            int c = 0;
                            for (int c0 = 0; c0 < n; c0 += 64) {
                                const int i = c0 + lane;
                                c += __popcll(__ballot(i < n && (__float_as_uint(eb[i]) & msk) == want));
                            }
                            return c;
                        },
                        n / 2);
                    if (lane == 0) score[j] = (int)bits;
                }
            }
            __syncthreads();
            // 4. the serial scan, the reference's rule
            for (int j = 0; j < nsub && base + j < niters; ++j) {
                iters = base + j + 1;
                const int sc = score[j];
                if (!lmeds) {
                    if (sc > (max_good > MP - 1 ? max_good : MP - 1)) {
                        max_good = sc;
#pragma unroll
                        for (int i = 0; i < 6; i++) M[i] = hyp[j * 6 + i];
                        niters = block_update_num_iters(confidence, (double)(n - sc) / n, MP, niters);
                    }
                } else {
                    const double median = __uint_as_float((unsigned)sc);
                    if (median < min_median) {
                        min_median = median;
#pragma unroll
                        for (int i = 0; i < 6; i++) M[i] = hyp[j * 6 + i];
                    }
                }
            }
            base += nsub;
            __syncthreads();
        }
        if (!lmeds) {
            have = max_good > 0;
        } else if (min_median < DBL_MAX) {
            t = ac::inlier_bound(ac::lmeds_sigma(min_median, n, MP));
            have = true;
        }
        if (have) {
            ninl = wave_count_inliers(all, n, ac::model_f(M), t, lane);
            have = ninl >= MP;  // LMEDS's result; RANSAC's consensus is larger by its rule
        }
        if (!have) {
            ninl = 0;
            M[0] = M[4] = 1;
            M[1] = M[2] = M[3] = M[5] = 0;
        }
    }
    const ac::ModelF mf = ac::model_f(M);
    // the mask, each byte once
    if (mask) {
        int pos0 = 0;
        for (int j0 = beg; j0 < end; j0 += kThreads) {
            const int j = j0 + tid;
            const bool ok = j < end && (status == nullptr || status[j]);
            int tot;
            const int pos = pos0 + block_prefix(ok, wc, &tot);
            if (j < end) mask[j] = (ok && have && (all_ones || ac::is_inlier(mf, t, all.M(pos), all.m(pos)))) ? 1 : 0;
            pos0 += tot;
        }
    }
    if (have && n > MP && refine_iters > 0) {
        // the inliers, compacted in place in point order (a pair never moves up)
        int cnt = 0;
        for (int c0 = 0; c0 < n; c0 += kThreads) {
            const int i = c0 + tid;
            float2 a = make_float2(0.f, 0.f), b = a;
            if (i < n) a = sa[i], b = sb[i];
            const bool in = i < n && ac::is_inlier(mf, t, hc::Pt{a.x, a.y}, hc::Pt{b.x, b.y});
            int tot;
            const int pos = cnt + block_prefix(in, wc, &tot);
            if (in) sa[pos] = a, sb[pos] = b;
            cnt += tot;
        }
        __syncthreads();
        const BlockStep<N> step{all, cnt, hc::Ws{wsm, 1}, red, xch};
        ac::LmSums<N>* cur = reinterpret_cast<ac::LmSums<N>*>(curm);
        if (MP == 3) {
            ac::lm_refine<N>(step, cur, refine_iters, M);
        } else {
            double h[4];
            ac::partial_pack(M, h);
            ac::lm_refine<N>(step, cur, refine_iters, h);
            ac::partial_unpack(h, M);
        }
    }
    if (tid == 0) {
        tbdk_affine2d o;
#pragma unroll
        for (int i = 0; i < 6; i++) o.m[i] = M[i];
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

int tbdk_affine2d_default_params(tbdk_affine2d_params* p)
{
    if (!p) return TBDK_EINVAL;
    p->model = TBDK_AFFINE2D_FULL;
    p->method = TBDK_AFFINE2D_RANSAC;
    p->reproj_threshold = 3.0;
    p->max_iters = 2000;
    p->confidence = 0.99;
    p->refine_iters = 10;
    return TBDK_OK;
}

int tbdk_estimate_affine_2d(tbdk_ctx* ctx, const float* src_pts, const float* dst_pts, const uint8_t* status,
                            const int32_t* offsets, int nsets, const tbdk_affine2d_params* params,
                            tbdk_affine2d* out, uint8_t* mask, void* stream)
{
    if (!ctx || nsets < 0 || !params) return TBDK_EINVAL;
    if (params->model != TBDK_AFFINE2D_FULL && params->model != TBDK_AFFINE2D_PARTIAL) return TBDK_EINVAL;
    if (params->method != TBDK_AFFINE2D_RANSAC && params->method != TBDK_AFFINE2D_LMEDS) return TBDK_EINVAL;
    if (params->max_iters < 1 || params->max_iters > 10000) return TBDK_EINVAL;
    // the reference asserts confidence in (0, 1); it takes the threshold as given, but a non-finite one has no meaning
    if (!(params->confidence > 0.0 && params->confidence < 1.0) || !isfinite(params->reproj_threshold))
        return TBDK_EINVAL;
    if (params->refine_iters < 0 || params->refine_iters > 100) return TBDK_EINVAL;
    if (nsets == 0) return TBDK_OK;
    if (!src_pts || !dst_pts || !offsets || !out) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float2* sp = reinterpret_cast<const float2*>(src_pts);
    const float2* dp = reinterpret_cast<const float2*>(dst_pts);
    const int rec = timing_begin(ctx, "estimate_affine2d", s);
    if (params->model == TBDK_AFFINE2D_FULL)
        hipLaunchKernelGGL(estimate_affine2d_kernel<3>, dim3(nsets), dim3(kThreads), 0, s, sp, dp, status, offsets, nsets,
                           params->method, params->reproj_threshold, params->max_iters, params->confidence,
                           params->refine_iters, out, mask);
    else
        hipLaunchKernelGGL(estimate_affine2d_kernel<2>, dim3(nsets), dim3(kThreads), 0, s, sp, dp, status, offsets, nsets,
                           params->method, params->reproj_threshold, params->max_iters, params->confidence,
                           params->refine_iters, out, mask);
    const hipError_t e = hipGetLastError();
    timing_end(ctx, rec, s);
    return e == hipSuccess ? TBDK_OK : (e == hipErrorOutOfMemory ? TBDK_ENOMEM : TBDK_EHIP);
}

}  // extern "C"
