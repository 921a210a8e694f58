// klt_subpix.hip — cv::cornerSubPix for a batch of points (tbdk_corner_sub_pix).
//
// The reference has a CPU implementation only (imgproc/src/cornersubpix.cpp:44-156
// on getRectSubPix, imgproc/src/samplers.cpp:129-268); this is its arithmetic,
// bit for bit, on the device:
//   1. per iteration one (2*win_w+3) x (2*win_h+3) float patch around the point,
//      by the reference's three code paths: the 8-bit inside path with its
//      running `prev` (samplers.cpp:232-262; prev depends on the left neighbour's
//      t only, so every pixel is computed on its own), and the generic path
//      inside and at the border (replicated rows and columns, :129-216) for
//      8-bit rectangles that touch the border and for float images;
//   2. central differences of the patch, weighted by the window mask
//      (float products of two expf tables made on the host: the device expf does
//      not round like glibc's), as five double terms per window pixel;
//   3. the five sums a, b, c, bb1, bb2 in double, in raster order: double
//      addition is not associative, so each sum is one serial chain;
//   4. the 2x2 solve, the stops and the revert of cornersubpix.cpp:134-154.
//
// Mapping: one 64-lane workgroup (one wave) per point.  All lanes compute the
// patch and the per-pixel terms into LDS; lanes 0..4 then walk one chain each
// over the terms (plain adds from LDS, no multiplies on the chain).  Control
// flow is uniform over the wave, so a point's stop needs no vote.  Rows are
// read with their device counts: blocks beyond a row's count leave at once.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "tbdk_internal.hpp"

namespace tbdk {

namespace {

constexpr int kSubpixMaxWin = 15;
constexpr int kSubpixLanes = 64;

struct SubpixArgs {
    const uint8_t* img;
    int w, h, pitch;          // pitch in bytes
    float2* corners;
    const int32_t* counts;    // per row, or null: every row full
    int row_cap;
    int win_w, win_h;         // half sizes
    int zero_w, zero_h;       // half sizes of the zero zone, -1: none
    int max_iters;
    double eps;               // squared
    float ex[2 * kSubpixMaxWin + 1], ey[2 * kSubpixMaxWin + 1];  // expf(-x*x) per column / row of the window
};

template <int PX>
__device__ __forceinline__ float subpix_px(const uint8_t* img, int pitch, int y, int x)
{
    const uint8_t* row = img + (size_t)y * (size_t)pitch;
    if constexpr (PX == TBDK_PIX_F32)
        return reinterpret_cast<const float*>(row)[x];
    else if constexpr (PX == TBDK_PIX_U16)
        return (float)reinterpret_cast<const uint16_t*>(row)[x];
    else
        return (float)row[x];
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cvFloor of a patch origin, kept inside +-2^30 so that the rectangle
// arithmetic below cannot overflow (the results are those of the unclamped
// value: beyond the image every tap is a replicated edge pixel); NaN gives a
// finite value
__device__ __forceinline__ float subpix_floor(float v) { return fminf(fmaxf(floorf(v), -1073741824.f), 1073741824.f); }

template <int PX>
__global__ __launch_bounds__(kSubpixLanes) void corner_sub_pix_kernel(const SubpixArgs a)
{
    extern __shared__ double s_dyn[];
    __shared__ double s_res[5];
    const int lane = threadIdx.x;
    const int row = blockIdx.x / a.row_cap, idx = blockIdx.x - row * a.row_cap;
    int cnt = a.counts ? a.counts[row] : a.row_cap;
    if (cnt > a.row_cap) cnt = a.row_cap;
    if (idx >= cnt) return;

    const int ww = 2 * a.win_w + 1, wh = 2 * a.win_h + 1, n = ww * wh;
    const int pw = ww + 2, ph = wh + 2;
    double* s_term = s_dyn;                                   // [5][n]
    float* s_mask = reinterpret_cast<float*>(s_term + 5 * n);  // [n]
    float* s_patch = s_mask + n;                              // [ph][pw]

    for (int k = lane; k < n; k += kSubpixLanes) {
        const int i = k / ww, j = k - i * ww;
        float m = a.ey[i] * a.ex[j];
        if (a.zero_w >= 0 && i >= a.win_h - a.zero_h && i <= a.win_h + a.zero_h && j >= a.win_w - a.zero_w &&
            j <= a.win_w + a.zero_w)
            m = 0.f;
        s_mask[k] = m;
    }

    float2* out = a.corners + (size_t)row * (size_t)a.row_cap + idx;
    const float2 cT = *out;
    float2 cI = cT;
    int iter = 0;
    double err = 0;
    const uint8_t* img = a.img;
    const int W = a.w, H = a.h, pitch = a.pitch;

    do {
        // ---- getRectSubPix(src, (pw, ph), cI) ----
        const float cx = cI.x - (float)(pw - 1) * 0.5f, cy = cI.y - (float)(ph - 1) * 0.5f;
        const float fx = subpix_floor(cx), fy = subpix_floor(cy);
        const int ipx = (int)fx, ipy = (int)fy;
        float fa = cx - fx, fb = cy - fy;
        const bool inside = 0 <= ipx && ipx < W - pw && 0 <= ipy && ipy < H - ph;
        if (PX == TBDK_PIX_U8 && inside) {
            fa = fa > 0.0001f ? fa : 0.0001f;
            const float a12 = fa * (1.f - fb), a22 = fa * fb, b1 = 1.f - fb, b2 = fb;
            const float a1 = 1.f - fa;
            const double s = (1. - (double)fa) / (double)fa;
            for (int k = lane; k < pw * ph; k += kSubpixLanes) {
                const int i = k / pw, j = k - i * pw;
                const int y = ipy + i, x = ipx + j;
                float prev;
                if (j == 0) {
                    prev = a1 * (b1 * subpix_px<PX>(img, pitch, y, x) + b2 * subpix_px<PX>(img, pitch, y + 1, x));
                } else {
                    const float tp = a12 * subpix_px<PX>(img, pitch, y, x) + a22 * subpix_px<PX>(img, pitch, y + 1, x);
                    prev = (float)((double)tp * s);
                }
                const float t = a12 * subpix_px<PX>(img, pitch, y, x + 1) + a22 * subpix_px<PX>(img, pitch, y + 1, x + 1);
                s_patch[k] = prev + t;
            }
        } else {
            const float a11 = (1.f - fa) * (1.f - fb), a12 = fa * (1.f - fb), a21 = (1.f - fa) * fb, a22 = fa * fb;
            const float b1 = 1.f - fb, b2 = fb;
            // adjustRect's columns: [rx, rwid) interpolate, the others replicate
            int base, rx, rwid;
            if (ipx >= 0) {
                base = ipx;
                rx = 0;
            } else {
                base = 0;
                rx = -ipx < pw ? -ipx : pw;
            }
            if (ipx < W - pw) {
                rwid = pw;
            } else {
                rwid = W - ipx - 1;
                if (rwid < 0) {
                    base += rwid;
                    rwid = 0;
                }
            }
            base -= rx;
            for (int k = lane; k < pw * ph; k += kSubpixLanes) {
                const int i = k / pw, j = k - i * pw;
                const int y0 = clampi(ipy + i, 0, H - 1), y1 = clampi(ipy + i + 1, 0, H - 1);
                float v;
                if (j >= rx && j < rwid) {
                    const int x0 = clampi(base + j, 0, W - 1), x1 = clampi(base + j + 1, 0, W - 1);
                    v = subpix_px<PX>(img, pitch, y0, x0) * a11 + subpix_px<PX>(img, pitch, y0, x1) * a12 +
                        subpix_px<PX>(img, pitch, y1, x0) * a21 + subpix_px<PX>(img, pitch, y1, x1) * a22;
                } else {
                    const int x = clampi(base + (j >= rwid ? rwid : rx), 0, W - 1);
                    v = subpix_px<PX>(img, pitch, y0, x) * b1 + subpix_px<PX>(img, pitch, y1, x) * b2;
                }
                s_patch[k] = v;
            }
        }
        __syncthreads();
        // ---- the five terms of every window pixel ----
        for (int k = lane; k < n; k += kSubpixLanes) {
            const int i = k / ww, j = k - i * ww;
            const float* sp = s_patch + (i + 1) * pw + (j + 1);
            const double m = (double)s_mask[k];
            const double tgx = (double)(sp[1] - sp[-1]);
            const double tgy = (double)(sp[pw] - sp[-pw]);
            const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
            const double px = (double)(j - a.win_w), py = (double)(i - a.win_h);
            s_term[k] = gxx;
            s_term[n + k] = gxy;
            s_term[2 * n + k] = gyy;
            s_term[3 * n + k] = gxx * px + gxy * py;
            s_term[4 * n + k] = gxy * px + gyy * py;
        }
        __syncthreads();
        // ---- a, b, c, bb1, bb2: one raster-order chain per lane ----
        if (lane < 5) {
            const double* tp = s_term + lane * n;
            double acc = 0;
            int k = 0;
            for (; k + 8 <= n; k += 8) {
                const double t0 = tp[k], t1 = tp[k + 1], t2 = tp[k + 2], t3 = tp[k + 3];
                const double t4 = tp[k + 4], t5 = tp[k + 5], t6 = tp[k + 6], t7 = tp[k + 7];
                acc += t0;
                acc += t1;
                acc += t2;
                acc += t3;
                acc += t4;
                acc += t5;
                acc += t6;
                acc += t7;
            }
            for (; k < n; ++k) acc += tp[k];
            s_res[lane] = acc;
        }
        __syncthreads();
        const double sa = s_res[0], sb = s_res[1], sc = s_res[2], bb1 = s_res[3], bb2 = s_res[4];
        const double det = sa * sc - sb * sb;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
        const double scale = 1.0 / det;
        float2 cI2;
        cI2.x = (float)((double)cI.x + sc * scale * bb1 - sb * scale * bb2);
        cI2.y = (float)((double)cI.y - sb * scale * bb1 + sa * scale * bb2);
        const float dx = cI2.x - cI.x, dy = cI2.y - cI.y;
        err = (double)(dx * dx + dy * dy);
        cI = cI2;
        if (cI.x < 0 || cI.x >= (float)W || cI.y < 0 || cI.y >= (float)H) break;
    } while (++iter < a.max_iters && err > a.eps);

    if (fabsf(cI.x - cT.x) > (float)a.win_w || fabsf(cI.y - cT.y) > (float)a.win_h) cI = cT;
    if (lane == 0) *out = cI;
}

size_t subpix_smem(int win_w, int win_h)
{
    const size_t n = (size_t)(2 * win_w + 1) * (2 * win_h + 1);
    return n * 5 * sizeof(double) + n * sizeof(float) + (size_t)(2 * win_w + 3) * (2 * win_h + 3) * sizeof(float);
}

bool subpix_params_ok(const tbdk_subpix_params* p)
{
    return p && p->win_w >= 1 && p->win_w <= kSubpixMaxWin && p->win_h >= 1 && p->win_h <= kSubpixMaxWin &&
           p->criteria >= 1 && p->criteria <= 3 && std::isfinite(p->epsilon);
}

// the window's two exponential tables, as cornersubpix.cpp:71-80 computes them
// (glibc's expf on the host), and the zero zone where the reference applies it
void subpix_tables(const tbdk_subpix_params* p, float* ex, float* ey, int* zero_w, int* zero_h)
{
    for (int j = 0; j < 2 * p->win_w + 1; ++j) {
        const float x = (float)(j - p->win_w) / p->win_w;
        ex[j] = std::exp(-x * x);
    }
    for (int i = 0; i < 2 * p->win_h + 1; ++i) {
        const float y = (float)(i - p->win_h) / p->win_h;
        ey[i] = std::exp(-y * y);
    }
    const bool zone = p->zero_w >= 0 && p->zero_h >= 0 && p->zero_w * 2 + 1 < 2 * p->win_w + 1 &&
                      p->zero_h * 2 + 1 < 2 * p->win_h + 1;
    *zero_w = zone ? p->zero_w : -1;
    *zero_h = zone ? p->zero_h : -1;
}

}  // namespace

int subpix_launch(tbdk_ctx* ctx, const void* img, int pix, int width, int height, int pitch, float* corners,
                  const int32_t* counts, int nrows, int row_cap, const tbdk_subpix_params* p, hipStream_t s)
{
    if (!ctx || !subpix_params_ok(p) || nrows < 0 || row_cap < 0) return TBDK_EINVAL;
    const int bpp = pix == TBDK_PIX_U8 ? 1 : pix == TBDK_PIX_U16 ? 2 : pix == TBDK_PIX_F32 ? 4 : 0;
    if (bpp == 0) return TBDK_EINVAL;
    const int64_t total = (int64_t)nrows * row_cap;
    if (total == 0) return TBDK_OK;
    if (total > 0x7FFFFFFF || !img || !corners || width < 2 * p->win_w + 5 || height < 2 * p->win_h + 5 ||
        reinterpret_cast<uintptr_t>(img) % (uintptr_t)bpp != 0 || pitch % bpp != 0 ||
        (int64_t)pitch < (int64_t)width * bpp)
        return TBDK_EINVAL;
    SubpixArgs a;
    a.img = static_cast<const uint8_t*>(img);
    a.w = width;
    a.h = height;
    a.pitch = pitch;
    a.corners = reinterpret_cast<float2*>(corners);
    a.counts = counts;
    a.row_cap = row_cap;
    a.win_w = p->win_w;
    a.win_h = p->win_h;
    a.max_iters = (p->criteria & 1) ? std::min(std::max(p->max_count, 1), 100) : 100;
    const double eps = (p->criteria & 2) ? std::max(p->epsilon, 0.) : 0.;
    a.eps = eps * eps;
    std::memset(a.ex, 0, sizeof(a.ex));
    std::memset(a.ey, 0, sizeof(a.ey));
    subpix_tables(p, a.ex, a.ey, &a.zero_w, &a.zero_h);
    DeviceGuard g(ctx->device);
    const size_t smem = subpix_smem(p->win_w, p->win_h);
    const dim3 grid((unsigned)total), block(kSubpixLanes);
    int rec = timing_begin(ctx, "corner_sub_pix", s);
    if (pix == TBDK_PIX_F32)
        hipLaunchKernelGGL(corner_sub_pix_kernel<TBDK_PIX_F32>, grid, block, smem, s, a);
    else if (pix == TBDK_PIX_U16)
        hipLaunchKernelGGL(corner_sub_pix_kernel<TBDK_PIX_U16>, grid, block, smem, s, a);
    else
        hipLaunchKernelGGL(corner_sub_pix_kernel<TBDK_PIX_U8>, grid, block, smem, s, a);
    const hipError_t e = hipGetLastError();
    timing_end(ctx, rec, s);
    return map_status(e);
}

}  // namespace tbdk

using namespace tbdk;

extern "C" {

int tbdk_subpix_default_params(tbdk_subpix_params* p)
{
    if (!p) return TBDK_EINVAL;
    p->win_w = p->win_h = 10;
    p->zero_w = p->zero_h = -1;
    p->criteria = 3;
    p->max_count = 20;
    p->epsilon = 0.03;
    return TBDK_OK;
}

int tbdk_corner_sub_pix_mask(const tbdk_subpix_params* p, float* mask)
{
    if (!subpix_params_ok(p) || !mask) return TBDK_EINVAL;
    float ex[2 * kSubpixMaxWin + 1], ey[2 * kSubpixMaxWin + 1];
    int zw, zh;
    subpix_tables(p, ex, ey, &zw, &zh);
    const int ww = 2 * p->win_w + 1, wh = 2 * p->win_h + 1;
    for (int i = 0; i < wh; ++i)
        for (int j = 0; j < ww; ++j) {
            const bool zero = zw >= 0 && i >= p->win_h - zh && i <= p->win_h + zh && j >= p->win_w - zw && j <= p->win_w + zw;
            mask[i * ww + j] = zero ? 0.f : ey[i] * ex[j];
        }
    return TBDK_OK;
}

int tbdk_corner_sub_pix(tbdk_ctx* ctx, const void* img, int pix, int width, int height, int pitch, float* corners,
                        const int32_t* counts, int nrows, int row_cap, const tbdk_subpix_params* params, void* stream)
{
    return subpix_launch(ctx, img, pix, width, height, pitch, corners, counts, nrows, row_cap, params,
                         static_cast<hipStream_t>(stream));
}

}  // extern "C"
