// klt_lk_multi.hip — sparse pyramidal LK with several points per wave (gfx950).
//
// Same algorithm and bit-identical results as klt_lk_strip.hip / klt_lk.hip
// (CPU calcOpticalFlowPyrLK numerics, LKTrackerInvoker video/src/lkpyramid.cpp:178-695,
// exact integer sums rounded once to float), laid out so that the per-point
// bookkeeping of a Newton step is shared by P = 64 / WW points:
//   * lane = one window column x of one point: point k of the wave owns lanes
//     [1 + k*WW, 1 + (k+1)*WW) (win 21: 3 points, lane 0 idle), and each lane
//     keeps all WH rows of its column (I patch x32, interpolated Scharr Ix/Iy,
//     the J column pairs) in VGPRs for every Newton iteration of the level;
//   * the bilinear weights, the 2x2 solve and the stopping tests run once per
//     lane for all P points at the cost of one (they are per-point values held
//     by every lane of the point), where the one-point-per-wave kernel spends a
//     wave-wide instruction on a single point's scalar math;
//   * per-point sums over the point's WW lanes: prefix scans over the wave with
//     six DPP adds (row_shr 1/2/4/8, row_bcast 15/31), each lane reading its
//     point's segment (end - start) back by ds_bpermute; exact for any window
//     by a lo/hi split of every partial with the hi parts of up to three sums
//     packed into one scan (seg_sum_exact), rounded once to float — the same
//     value as the exact int64 sum of the other kernels;
//   * control flow stays wave-uniform (levels, Newton steps while any point is
//     active, J reloads when any point's integer origin moved), so every DPP and
//     bpermute runs with all lanes on; a point that stopped keeps its values by
//     selects.
#include <type_traits>

#include "lk_device.hpp"
#include "lk_int_origin.hpp"
#include "lk_stop.hpp"

namespace tbdk {

namespace {

using namespace lkdev;

// inclusive prefix sum over the 64 lanes (all lanes active), modulo 2^32
__device__ __forceinline__ uint32_t scan64(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

// M independent scans advanced step by step together: each DPP reads a value
// written two or more instructions earlier, so no wait states are needed
// between the dependent adds of one scan (a lone scan64 needs one per step)
template <int M>
__device__ __forceinline__ void scan64_n(uint32_t (&v)[M])
{
#define TBDK_SCAN_STEP(ctrl, rmask, bc)                                                                    \
    _Pragma("unroll") for (int m = 0; m < M; ++m) v[m] +=                                                  \
        (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[m], ctrl, rmask, 0xF, bc);
    TBDK_SCAN_STEP(0x111, 0xF, true)   // row_shr:1
    TBDK_SCAN_STEP(0x112, 0xF, true)   // row_shr:2
    TBDK_SCAN_STEP(0x114, 0xF, true)   // row_shr:4
    TBDK_SCAN_STEP(0x118, 0xF, true)   // row_shr:8
    TBDK_SCAN_STEP(0x142, 0xA, false)  // row_bcast:15 -> rows 1, 3
    TBDK_SCAN_STEP(0x143, 0xC, false)  // row_bcast:31 -> rows 2, 3
#undef TBDK_SCAN_STEP
}

// segment total of a scanned value: prefix at the point's last lane minus the
// prefix at the lane before its first (lane 0 is idle and holds 0, so every
// point has such a lane)
__device__ __forceinline__ uint32_t seg_total(uint32_t scanned, int e4, int s4)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute(e4, (int)scanned) -
           (uint32_t)__builtin_amdgcn_ds_bpermute(s4, (int)scanned);
}

// Exact per-point sums of N <= 3 int32 lane partials (|partial| < 2^30): every
// lane gets its own point's sum, rounded once to float.  Each partial is split
// as hi * 2^26 + lo (0 <= lo < 2^26, -16 <= hi < 16).  The lo parts are scanned
// one per value (a point's lo total is below 21 * 2^26 < 2^31, exact as a
// modulo-2^32 difference); the hi parts of all N values share ONE scan, packed
// in 11-bit fields (a point's hi total lies in [-16*21, 15*21] and every field
// below the top one is recovered by sign extension).  hi * 2^26 + lo in double
// is the exact integer sum; the one float rounding gives the same value as the
// exact int64 sum of the other kernels.  e4 / s4: byte addresses of the point's
// last lane and of the lane before its first.
//
// Fast path, taken by the whole wave when every partial lies in (-2^FB, 2^FB):
// a point's total is then below 31 * 2^26 < 2^31 in magnitude (FB 26: windows
// up to 31 wide), or 63 * 2^25 (FB 25: a point spread over all 63 lanes, the
// one-point steps below), exact as a modulo-2^32 difference of plain scans, and
// its int -> float conversion is the same single rounding.  The split path
// holds for segments of up to 63 lanes (lo totals below 63 * 2^26 < 2^32, hi
// totals in [-16 * 63, 15 * 63], inside an 11-bit field).
template <int N, int FB = 26>
__device__ __forceinline__ void seg_sum_exact(const int (&v)[N], int e4, int s4, float (&out)[N], bool* split = nullptr)
{
    static_assert(N >= 1 && N <= 3, "three 11-bit fields per packed scan");
    static_assert(FB <= 26, "hi parts are v >> 26");
    bool big = false;
#pragma unroll
    for (int k = 0; k < N; ++k) big |= (uint32_t)v[k] + (1u << FB) >= (2u << FB);
    const bool slow = __builtin_amdgcn_ballot_w64(big) != 0;  // wave-uniform
    if (split) *split = slow;
    if (!slow) {
        uint32_t sv[N];
#pragma unroll
        for (int k = 0; k < N; ++k) sv[k] = (uint32_t)v[k];
        scan64_n(sv);
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = (float)(int)seg_total(sv[k], e4, s4);
        return;
    }
    uint32_t sc[N + 1];  // lo parts, then the packed hi parts
    sc[N] = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sc[k] = (uint32_t)v[k] & 0x3FFFFFFu;
        sc[N] += (uint32_t)(v[k] >> 26) << (11 * k);
    }
    scan64_n(sc);
    int h = (int)seg_total(sc[N], e4, s4);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int hk = k + 1 < N ? (int)((uint32_t)h << 21) >> 21 : h;  // sign-extended low field
        h = (h - hk) >> 11;
        const uint32_t l = seg_total(sc[k], e4, s4);
        out[k] = (float)((double)hk * 67108864.0 + (double)l);  // exact in double, one rounding
    }
}

// per-point sum of small lane values (no split: |total| < 2^31)
__device__ __forceinline__ int seg_sum_small(int v, int e4, int s4)
{
    return (int)seg_total(scan64((uint32_t)v), e4, s4);
}

// p0 . w0 + p1 . w1 + c: the reference's bilinear sum started from a per-row
// VGPR constant (the three-operand v_dot2_i32_i16 keeps c; the compiler
// otherwise copies c and accumulates with v_dot2c)
__device__ __forceinline__ int bilin_c(uint32_t p0, uint32_t p1, uint32_t w0, uint32_t w1, int c)
{
    int t;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(t) : "v"(p1), "v"(w1), "v"(c));
    return sdot2(p0, w0, t);
}

// (t0 >> SH, t1 >> SH) as int16 x 2 in two instructions: t0 >> SH, then the
// SDWA form of the second shift writes only the high word (WORD_1) of the
// result, keeping the low word
template <int SH>
__device__ __forceinline__ uint32_t pack_shr(int t0, int t1)
{
    uint32_t d = (uint32_t)(t0 >> SH);
    asm("v_ashrrev_i32_sdwa %0, %2, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD"
        : "+v"(d)
        : "v"(t1), "i"(SH));
    return d;
}
__device__ __forceinline__ uint32_t pack_diff(int t0, int t1) { return pack_shr<9>(t0, t1); }

__device__ __forceinline__ bool any_lane(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }


}  // namespace

// waves per workgroup (tuning builds may change it; the kernel uses no LDS, so
// one-wave workgroups let a finished wave's slot be refilled at once)
// I x32 kept as packed row pairs and subtracted from the J pairs by one packed
// op per row pair (1), or folded into each row's J rounding constant (0, one
// VGPR per row; tuning builds)
// How I enters the Newton step's b sums (tuning builds may change it):
//   0: folded into each row's J rounding constant (one VGPR per row)
//   1: I pairs packed by rows, one v_pk_sub per row pair and step
//   2: b = sum(Jd * g) - sum(I * g): the second sum (per lane, per level) is
//      made once in the level setup, so the step needs no I at all; the final
//      error recomputes the I rows from the level
#ifndef TBDK_LK_IPACK
#define TBDK_LK_IPACK 1  // derivative-plane instance (94 VGPRs -> 5 waves per SIMD)
#endif
#ifndef TBDK_LK_IPACK_FLY
#define TBDK_LK_IPACK_FLY 0  // Scharr-on-the-fly instance
#endif
// The Scharr-on-the-fly setup's arm for waves whose windows all have an integer
// origin at the level (lk_int_origin.hpp; the same results).  0 compiles it out,
// for tools/lk_valu_count.py to count the kernel without it.
#ifndef TBDK_LK_INT_ORIGIN
#define TBDK_LK_INT_ORIGIN 1
#endif

// Probe builds (-DTBDK_LK_TRACE, tools/probe_lk_trace.py): every wave writes
// one record of sixteen u64 (at its launch's base + its wave index, no atomics:
// a device-wide atomic counter serialises the waves' exits) to a device buffer
// set by tbdk_probe_lk_trace():
// start / end (s_memrealtime, 100 MHz), HW_ID | XCC_ID << 32, n << 32 | wave,
// the launch's point-list key, Newton steps | reloads << 16 | max iters << 32,
// then 16 u32 phase stamps (ticks after start): per level L, [4L] its start,
// [4L+1] the setup's G sums done, [4L+2] the first J window loaded (the probe
// waits for it there), [4L+3] its Newton steps done; [12] the error pass done;
// [13] the point's coordinates arrived (start: the wave's first instruction),
// [14] the first level's source rows arrived (FLY; the probe waits for them
// there), [15] its window terms done (before the G sums); bits 48..55 of the
// steps word: the levels whose G sums took seg_sum_exact's split path, bits
// 56..63: the levels whose setup took the integer-origin arm.  Not in the
// product library.
#ifdef TBDK_LK_TRACE
__device__ unsigned long long* g_lk_trace;
__device__ unsigned int g_lk_trace_cap;
static unsigned g_lk_trace_next;  // host: records handed out so far
#endif

// FLY: the Scharr derivatives of the window are computed from the u8 level in
// the level setup instead of read from the pyramid's derivative planes (same
// values; the planes need not exist).
// DENSE (klt_dense.hip, cv::cuda::DensePyrLKOpticalFlow): the points are the
// pixel grid, and a point's interpolated window (I x32, Ix, Iy) is read from
// the level's case images instead of interpolated in the setup: the window of
// pixel (x, y) at level L has the sub-pixel phase (x mod 2^L, y mod 2^L) / 2^L
// and origin (x >> L, y >> L) - half, so every window element is element
// (y >> L) - half + r, (x >> L) - half + c of the case image of that phase,
// the same integers the planes setup computes (the phase's weights applied to
// the same pyramid and derivative-plane values).  The Newton steps are this
// kernel's.  Outputs: the flow (next - pixel) and the status plane.
// BACK (lk_multi_back_kernel, tbdk_lk_sparse_fb): the backward pass of the
// forward-backward check.  The launch's pyramids are swapped by the host; a
// point starts at the forward pass's result (next_pts, read only) and is
// skipped when the forward status is 0; flags are 0 and there is no error
// pass.  The epilogue compares the point tracked back with prev_pts and
// clears status where the check fails; next_pts / err / iters are not written.
//
// The body is klt_lk_multi_body.inc, included by both kernels.  A device
// function template called from both was tried first: inlined into
// lk_multi_kernel it compiled to other instructions than the kernel had (the
// window-21 Scharr-on-the-fly instance: 124 VGPRs for 125, another schedule),
// while the included text leaves every forward instance's instructions as they
// were (compared by disassembly).
template <int WW, int WH, bool FLY, bool DENSE = false>
__global__ __launch_bounds__(64) void lk_multi_kernel(LkArgs a)
{
    constexpr bool BACK = false;
    const LkBack bk{};
#include "klt_lk_multi_body.inc"
}

// the backward pass of the forward-backward check: a kernel of its own name,
// Scharr on the fly
template <int WW, int WH>
__global__ __launch_bounds__(64) void lk_multi_back_kernel(LkArgs a, LkBack bk)
{
    constexpr bool BACK = true, FLY = true, DENSE = false;
#include "klt_lk_multi_body.inc"
}

#define TBDK_MULTI_WINDOWS(X) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) X(23) X(25) X(27) X(29) X(31)

bool lk_multi_supported(int win_w, int win_h)
{
    if (win_w != win_h) return false;
    switch (win_w) {
#define TBDK_CASE(W) case W:
        TBDK_MULTI_WINDOWS(TBDK_CASE)
#undef TBDK_CASE
        return true;
    default:
        return false;
    }
}

hipError_t launch_lk_multi(const LkArgs& a, bool fly, hipStream_t s)
{
    if (!lk_multi_supported(a.win_w, a.win_h)) return hipErrorNotSupported;
    const int per_wg = 64 / a.win_w;  // one wave of P points
    const dim3 grid((a.n + per_wg - 1) / per_wg), block(64);
#ifdef TBDK_LK_TRACE
    LkArgs at = a;
    at.trace_base = g_lk_trace_next;
    g_lk_trace_next += grid.x;
    const LkArgs& la = at;
#else
    const LkArgs& la = a;
#endif
    switch (a.win_w) {
#define TBDK_CASE(W)                                                                    \
    case W:                                                                             \
        if (fly) hipLaunchKernelGGL((lk_multi_kernel<W, W, true>), grid, block, 0, s, la);  \
        else hipLaunchKernelGGL((lk_multi_kernel<W, W, false>), grid, block, 0, s, la); \
        break;
        TBDK_MULTI_WINDOWS(TBDK_CASE)
#undef TBDK_CASE
    default:
        return hipErrorNotSupported;
    }
    return hipGetLastError();
}

hipError_t launch_lk_multi_back(const LkArgs& a, const LkBack& b, hipStream_t s)
{
    if (!lk_multi_supported(a.win_w, a.win_h)) return hipErrorNotSupported;
    const int per_wg = 64 / a.win_w;  // one wave of P points
    const dim3 grid((a.n + per_wg - 1) / per_wg), block(64);
#ifdef TBDK_LK_TRACE
    LkArgs at = a;
    at.trace_base = g_lk_trace_next;
    g_lk_trace_next += grid.x;
    const LkArgs& la = at;
#else
    const LkArgs& la = a;
#endif
    switch (a.win_w) {
#define TBDK_CASE(W)                                                              \
    case W:                                                                       \
        hipLaunchKernelGGL((lk_multi_back_kernel<W, W>), grid, block, 0, s, la, b); \
        break;
        TBDK_MULTI_WINDOWS(TBDK_CASE)
#undef TBDK_CASE
    default:
        return hipErrorNotSupported;
    }
    return hipGetLastError();
}

hipError_t launch_lk_multi_dense(const LkArgs& a, hipStream_t s)
{
    if (!lk_multi_supported(a.win_w, a.win_h)) return hipErrorNotSupported;
    const int per_wg = 64 / a.win_w;  // one wave of P points
    const dim3 grid((a.n + per_wg - 1) / per_wg), block(64);
    switch (a.win_w) {
#define TBDK_CASE(W)                                                                          \
    case W:                                                                                   \
        hipLaunchKernelGGL((lk_multi_kernel<W, W, false, true>), grid, block, 0, s, a);       \
        break;
        TBDK_MULTI_WINDOWS(TBDK_CASE)
#undef TBDK_CASE
    default:
        return hipErrorNotSupported;
    }
    return hipGetLastError();
}

}  // namespace tbdk

#ifdef TBDK_LK_TRACE
extern "C" int tbdk_probe_lk_trace(void* buf, unsigned cap)
{
    unsigned long long* p = static_cast<unsigned long long*>(buf);
    cap /= 16;  // records of sixteen u64
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(tbdk::g_lk_trace), &p, sizeof(p)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(tbdk::g_lk_trace_cap), &cap, sizeof(cap)) != hipSuccess)
        return -2;
    tbdk::g_lk_trace_next = 0;
    return 0;
}
// records handed out since tbdk_probe_lk_trace (waves that exit early, with no
// valid point, leave theirs zero)
extern "C" int tbdk_probe_lk_trace_count(unsigned* n)
{
    *n = tbdk::g_lk_trace_next;
    return 0;
}
#endif
