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
// The level walk is lk_walk.hpp; this file is its window policy for one-channel
// u8 levels of any window size, staged in LDS.
#include "lk_walk.hpp"

namespace tbdk {

size_t lk_smem_bytes(int win_w, int win_h)
{
    const int SW = win_w + 3, SH = win_h + 3;
    size_t b = align_up(SW * SH, 16);
    b += align_up((win_w + 1) * (win_h + 1) * 4, 16);
    b += align_up(win_w * win_h * 2, 16);
    b += align_up(win_w * win_h * 4, 16);
    return b;
}

namespace {

using namespace lkdev;

// the window of one point in LDS: sI the (win+3)^2 u8 pixels of I from
// (ipx-1, ipy-1), sD their Scharr pairs on the (win+1)^2 grid, sP the patch
// (x32), sG its interpolated (Ix, Iy) pairs.  Lane l handles patch pixels
// l, l + 64, ...
struct LdsWin {
    const int lane, winW, winH, area, SW, SH, DW;
    uint8_t* sI;
    int32_t* sD;
    int16_t* sP;
    int32_t* sG;
    // lane -> pixel maps of the three grids (p = lane + 64k): the start and
    // the step of 64 as (column, row)
    const int qx, qy, lx0, ly0, dq, dqy, dx0, dy0, sq, sqy, sx0, sy0;

    __device__ __forceinline__ LdsWin(const LkArgs& a, uint8_t* smem, int lane_)
        : lane(lane_), winW(a.win_w), winH(a.win_h), area(winW * winH), SW(winW + 3), SH(winH + 3), DW(winW + 1),
          qx(64 % winW), qy(64 / winW), lx0(lane % winW), ly0(lane / winW), dq(64 % DW), dqy(64 / DW),
          dx0(lane % DW), dy0(lane / DW), sq(64 % SW), sqy(64 / SW), sx0(lane % SW), sy0(lane / SW)
    {
        sI = smem;
        sD = reinterpret_cast<int32_t*>(smem + align_up(SW * SH, 16));
        sP = reinterpret_cast<int16_t*>(reinterpret_cast<uint8_t*>(sD) + align_up(DW * (winH + 1) * 4, 16));
        sG = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(sP) + align_up(area * 2, 16));
    }

    __device__ __forceinline__ int win_w() const { return winW; }
    __device__ __forceinline__ int win_h() const { return winH; }
    __device__ __forceinline__ bool gate(float, float, int ix, int iy, const LkLevel& L) const
    {
        return out_of_level(ix, iy, winW, winH, L.w, L.h);
    }
    __device__ __forceinline__ void release() const { __syncthreads(); }

    __device__ __forceinline__ void setup(const LkLevel& L, int ipx, int ipy, float fa, float fb, float& A11,
                                          float& A12, float& A22)
    {
        const float FLT_SCALE = 1.f / (1 << 20);
        int iw00, iw01, iw10, iw11;
        bilinear_weights_int(fa, fb, iw00, iw01, iw10, iw11);
        // ---- stage the (win+3)^2 u8 window of I starting at (ipx-1, ipy-1)
        {
            const uint8_t* base = L.I + (size_t)(ipy - 1 + L.ipad) * L.ipitch + (ipx - 1 + L.ipad);
            int sx = sx0, sy = sy0;
            for (int p = lane; p < SW * SH; p += 64) {
                sI[p] = base[(size_t)sy * L.ipitch + sx];
                sx += sq;
                sy += sqy;
                if (sx >= SW) {
                    sx -= SW;
                    sy += 1;
                }
            }
        }
        __syncthreads();
        // ---- Scharr derivatives on the (win+1)^2 grid; 0 outside the level
        {
            int dx = dx0, dy = dy0;
            for (int p = lane; p < DW * (winH + 1); p += 64) {
                const int X = ipx + dx, Y = ipy + dy;
                int32_t packed = 0;
                if (X >= 0 && X < L.w && Y >= 0 && Y < L.h) {
                    const uint8_t* r0 = sI + dy * SW + dx;  // row Y-1, col X-1
                    const uint8_t* r1 = r0 + SW;
                    const uint8_t* r2 = r1 + SW;
                    const int t0l = (r0[0] + r2[0]) * 3 + r1[0] * 10;
                    const int t0r = (r0[2] + r2[2]) * 3 + r1[2] * 10;
                    const int t1l = r2[0] - r0[0], t1c = r2[1] - r0[1], t1r = r2[2] - r0[2];
                    const int ix = t0r - t0l;
                    const int iy = (t1r + t1l) * 3 + t1c * 10;
                    packed = (int32_t)(((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16));
                }
                sD[p] = packed;
                dx += dq;
                dy += dqy;
                if (dx >= DW) {
                    dx -= DW;
                    dy += 1;
                }
            }
        }
        __syncthreads();
        // ---- I patch (x32), interpolated derivatives, G partial sums
        int a11 = 0, a12 = 0, a22 = 0;
        int px = lx0, py = ly0;
        for (int p = lane; p < area; p += 64) {
            const uint8_t* s = sI + (py + 1) * SW + (px + 1);
            const int ival = descale(s[0] * iw00 + s[1] * iw01 + s[SW] * iw10 + s[SW + 1] * iw11, W_BITS1 - 5);
            const int32_t* d = sD + py * DW + px;
            const int32_t d00 = d[0], d01 = d[1], d10 = d[DW], d11 = d[DW + 1];
            const int ix = descale((int16_t)d00 * iw00 + (int16_t)d01 * iw01 + (int16_t)d10 * iw10 +
                                       (int16_t)d11 * iw11, W_BITS1);
            const int iy = descale((d00 >> 16) * iw00 + (d01 >> 16) * iw01 + (d10 >> 16) * iw10 +
                                       (d11 >> 16) * iw11, W_BITS1);
            sP[p] = (int16_t)ival;
            sG[p] = (int32_t)(((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16));
            a11 += ix * ix;
            a12 += ix * iy;
            a22 += iy * iy;
            next_pixel(px, py);
        }
        A11 = (float)wave_sum_f64((double)a11) * FLT_SCALE;
        A12 = (float)wave_sum_f64((double)a12) * FLT_SCALE;
        A22 = (float)wave_sum_f64((double)a22) * FLT_SCALE;
    }

    __device__ __forceinline__ void next_pixel(int& px, int& py) const
    {
        px += qx;
        py += qy;
        if (px >= winW) {
            px -= winW;
            py += 1;
        }
    }

    // J(x + fa, y + fb) x 32 - I at patch pixel p = (px, py), jb the window's origin in J
    __device__ __forceinline__ int j_diff(const uint8_t* jb, int jpitch, int p, int px, int py, int iw00, int iw01,
                                          int iw10, int iw11) const
    {
        const uint8_t* q = jb + (size_t)py * jpitch + px;
        const int jv = descale(q[0] * iw00 + q[1] * iw01 + q[jpitch] * iw10 + q[jpitch + 1] * iw11, W_BITS1 - 5);
        return jv - sP[p];
    }

    __device__ __forceinline__ void step(const LkLevel& L, int inx, int iny, float fa, float fb, float& fb1,
                                         float& fb2) const
    {
        const float FLT_SCALE = 1.f / (1 << 20);
        int iw00, iw01, iw10, iw11;
        bilinear_weights_int(fa, fb, iw00, iw01, iw10, iw11);
        const uint8_t* jb = L.J + (size_t)(iny + L.jpad) * L.jpitch + (inx + L.jpad);
        int b1 = 0, b2 = 0;
        int px = lx0, py = ly0;
        for (int p = lane; p < area; p += 64) {
            const int diff = j_diff(jb, L.jpitch, p, px, py, iw00, iw01, iw10, iw11);
            const int32_t g = sG[p];
            b1 += diff * (int16_t)g;
            b2 += diff * (g >> 16);
            next_pixel(px, py);
        }
        fb1 = (float)wave_sum_f64((double)b1) * FLT_SCALE;
        fb2 = (float)wave_sum_f64((double)b2) * FLT_SCALE;
    }

    __device__ __forceinline__ float error(const LkLevel& L, int inx, int iny, float fa, float fb) const
    {
        int iw00, iw01, iw10, iw11;
        bilinear_weights_int(fa, fb, iw00, iw01, iw10, iw11);
        const uint8_t* jb = L.J + (size_t)(iny + L.jpad) * L.jpitch + (inx + L.jpad);
        int e = 0;
        int px = lx0, py = ly0;
        for (int p = lane; p < area; p += 64) {
            const int diff = j_diff(jb, L.jpitch, p, px, py, iw00, iw01, iw10, iw11);
            const int ad = diff < 0 ? -diff : diff;
            e += ad;
            sG[p] = ad;  // (the derivatives have had their last use: level 0, after the iteration)
            next_pixel(px, py);
        }
        // the reference adds |diff| in a float in window order (lkpyramid.cpp:677-692):
        // the exact sum while that stays within 2^24, where every partial sum is
        // exact; beyond it each addition rounds, and the same chain is run here
        const double esum = wave_sum_f64((double)e);
        float errval = (float)esum;
        if (esum > 16777216.0) {  // block-uniform
            __syncthreads();
            errval = 0.f;
            for (int p = 0; p < area; ++p) errval += (float)sG[p];
        }
        return errval * 1.f / (float)(32 * winW * winH);
    }
};

}  // namespace

__global__ __launch_bounds__(64) void lk_sparse_kernel(LkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int i = seg_point(a, xcd_swizzle(blockIdx.x, gridDim.x));
    if (i < 0) return;
    LdsWin win(a, smem, threadIdx.x);
    lk_walk_point(a, i, threadIdx.x == 0, win);
}

// The backward pass of the forward-backward check (tbdk_lk_sparse_fb).  The
// launch's pyramids are swapped by the host; the point starts at the forward
// pass's result (next_pts, read only) and is skipped when the forward status
// is 0; flags are 0 and there is no error pass.  The epilogue compares the
// point tracked back with prev_pts and clears status where the check fails;
// next_pts / err / iters are not written.
__global__ __launch_bounds__(64) void lk_sparse_back_kernel(LkArgs a, LkBack bk)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int i = seg_point(a, xcd_swizzle(blockIdx.x, gridDim.x));
    if (i < 0) return;
    const int lane = threadIdx.x;
    const float o0x = a.prev_pts[2 * i], o0y = a.prev_pts[2 * i + 1];  // the forward pass's start
    if (!a.status[i]) {  // lost by the forward pass: takes no part (block-uniform)
        if (lane == 0) {
            if (bk.back_pts) {
                bk.back_pts[2 * i] = o0x;
                bk.back_pts[2 * i + 1] = o0y;
            }
            if (bk.fb_err) bk.fb_err[i] = __builtin_inff();
        }
        return;
    }
    LdsWin win(a, smem, lane);
    LkWalkOut o;
    lk_walk(a, 0, false, a.next_pts[2 * i], a.next_pts[2 * i + 1], 0.f, 0.f, win, o);
    if (lane == 0) {
        const float dx = fabsf(o0x - o.x), dy = fabsf(o0y - o.y);
        const float d = fmaxf(dx, dy);
        if (bk.back_pts) {
            bk.back_pts[2 * i] = o.x;
            bk.back_pts[2 * i + 1] = o.y;
        }
        if (bk.fb_err) bk.fb_err[i] = o.status ? d : __builtin_inff();
        if (!(o.status && d < bk.thr)) a.status[i] = 0;
    }
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
