// klt_lk.hip — sparse pyramidal Lucas-Kanade for gfx950, one wave64 per point,
// every pyramid level in one launch.
//
// Numerics follow the CPU cv::calcOpticalFlowPyrLK (LKTrackerInvoker,
// video/src/lkpyramid.cpp:178-695), not the CUDA texture path:
//   * 14-bit fixed-point bilinear weights iw = cvRound(w * 2^14)       (:227-234)
//   * I patch scaled by 32, Scharr derivatives in int16                (:268-420)
//   * Scharr (calcSharrDeriv :55-144) is recomputed on the fly from the
//     LDS-staged (win+3)^2 u8 window; outside the level it is 0, as the
//     BORDER_CONSTANT frame of the reference derivative image (:1357)
//   * minEig gate, eps^2 and oscillation-halving rules                 (:442-652)
//   * L1 error / 32 at level 0                                          (:654-693)
// The G-matrix and b-vector sums are formed EXACTLY (integer products, int32
// lane partials, reduced in double which is exact below 2^53) and rounded to
// float once; the reference sums the same integer terms in float in SSE2-lane
// order.  The two differ only by the reference's float rounding (see the
// oracle's ORC_ACCUM_EXACT / ORC_ACCUM_SSE2 modes and DESIGN.md §Numerics).
// Built with -ffp-contract=off: every remaining float/double expression is
// evaluated exactly as written in the reference.
#include "tbdk_internal.hpp"

namespace tbdk {

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ int round_even(float v) { return __float2int_rn(v); }

size_t lk_smem_bytes(int win_w, int win_h)
{
    const int SW = win_w + 3, SH = win_h + 3;
    size_t b = align_up(SW * SH, 16);
    b += align_up((win_w + 1) * (win_h + 1) * 4, 16);
    b += align_up(win_w * win_h * 2, 16);
    b += align_up(win_w * win_h * 4, 16);
    return b;
}

// BACK (lk_sparse_back_kernel, tbdk_lk_sparse_fb): the backward pass of the
// forward-backward check.  The launch's pyramids are swapped by the host; the
// point starts at the forward pass's result (next_pts, read only) and is
// skipped when the forward status is 0; flags are 0 and there is no error
// pass.  The epilogue compares the point tracked back with prev_pts and clears
// status where the check fails; next_pts / err / iters are not written.
// The body is klt_lk_body.inc, included by both kernels (as in klt_lk_multi.hip:
// the forward kernel's instructions stay as they were).
__global__ __launch_bounds__(64) void lk_sparse_kernel(LkArgs a)
{
    constexpr bool BACK = false;
    const LkBack bk{};
#include "klt_lk_body.inc"
}

// the backward pass of the forward-backward check
__global__ __launch_bounds__(64) void lk_sparse_back_kernel(LkArgs a, LkBack bk)
{
    constexpr bool BACK = true;
#include "klt_lk_body.inc"
}

hipError_t launch_lk_sparse_back(const LkArgs& a, const LkBack& b, hipStream_t s)
{
    const size_t smem = lk_smem_bytes(a.win_w, a.win_h);
    hipLaunchKernelGGL(lk_sparse_back_kernel, dim3(a.n), dim3(64), smem, s, a, b);
    return hipGetLastError();
}

hipError_t launch_lk_sparse(const LkArgs& a, hipStream_t s)
{
    const size_t smem = lk_smem_bytes(a.win_w, a.win_h);
    hipLaunchKernelGGL(lk_sparse_kernel, dim3(a.n), dim3(64), smem, s, a);
    return hipGetLastError();
}

}  // namespace tbdk
