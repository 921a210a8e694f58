// frontend.hip — the image front end of the detection-driven loop on gfx950:
// cv::cvtColor (8-bit, the six codes the sample's path needs) and
// cv::resize(INTER_LINEAR) for u8 images, bit-exact with the CPU functions
// (tests/_frontend_oracle.py, pinned to them by tests/golden/frontend_cases.npz),
// plus the two fused into one pass for the loop's common case
// (BGR/BGRA frame -> gray -> resized gray, samples/gpu/tbd.cpp:573-578).
//
//   gray   : RGB2Gray<uchar> (imgproc/src/color_rgb.simd.hpp:647), the fixed-point
//            form of color.simd_helpers.hpp:16-20: (B*1868 + G*9617 + R*4899 + 8192) >> 14
//   resize : the 11-bit fixed-point path of imgproc/src/resize.cpp, not the
//            INTER_LINEAR_EXACT of hog.hip: per-axis tables made on the host as
//            the reference makes them (:3609-3702: float fx, cvFloor, the sx < 0
//            and sx >= width-1 clamps, saturate_cast<short>(c*2048)), HResizeLinear
//            (:1492) and the uchar VResizeLinear (:1578) in the kernel; both
//            scales exactly 2 is INTER_AREA (:3523, ResizeAreaFastVec :2534),
//            equal sizes a copy (:3745).
//
// Threading follows warp.hip: one thread per four destination elements of a
// row (pixels of a gray destination, bytes of an interleaved one), one 32-bit
// store where the address allows it, scalar tail.  These are streaming kernels:
// a thread has 12-16 source bytes (colour conversion) or its 8-16 taps
// (resize) outstanding before its first use, 256-thread workgroups at full
// occupancy keep 24-32 KB of loads in flight per CU.  The only floating point
// is the host-side coefficient generation (the file is built with
// -ffp-contract=off like the rest).
#include <cmath>
#include <cstring>

#include "tbdk_internal.hpp"

namespace tbdk {

namespace {

constexpr int kB2Y = 1868, kG2Y = 9617, kR2Y = 4899, kYuvShift = 14;

struct Gray3 {
    int c0, c1, c2;  // weights of channels 0..2
};

__device__ __forceinline__ int to_gray(int v0, int v1, int v2, Gray3 g)
{
    return (v0 * g.c0 + v1 * g.c1 + v2 * g.c2 + (1 << (kYuvShift - 1))) >> kYuvShift;
}

__device__ __forceinline__ void store4(uint8_t* D, int x0, int n, const uint8_t* out)
{
    if (x0 + 4 <= n && ((reinterpret_cast<uintptr_t>(D + x0) & 3) == 0)) {
        *reinterpret_cast<uint32_t*>(D + x0) =
            (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < n) D[x0 + k] = out[k];
    }
}

// four pixels of SCN bytes each, from x0 on, into px[4 * SCN] (whole words when
// all four are inside the row and the address is word aligned)
template <int SCN>
__device__ __forceinline__ void load4px(const uint8_t* S, int x0, int w, uint8_t* px)
{
    const uint8_t* p = S + (size_t)x0 * SCN;
    if (x0 + 4 <= w && ((reinterpret_cast<uintptr_t>(p) & 3) == 0)) {
        uint32_t wd[SCN];
#pragma unroll
        for (int i = 0; i < SCN; ++i) wd[i] = reinterpret_cast<const uint32_t*>(p)[i];
#pragma unroll
        for (int i = 0; i < 4 * SCN; ++i) px[i] = (uint8_t)(wd[i >> 2] >> (8 * (i & 3)));
    } else {
#pragma unroll
        for (int i = 0; i < 4 * SCN; ++i) px[i] = x0 + i / SCN < w ? p[i] : (uint8_t)0;
    }
}

// ---- cvtColor ----

template <int SCN>
__global__ __launch_bounds__(256) void cvt_gray_kernel(const uint8_t* src, int spitch, uint8_t* dst, int dpitch, int w,
                                                       Gray3 g)
{
    const int y = blockIdx.y;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x0 >= w) return;
    uint8_t px[4 * SCN], out[4];
    load4px<SCN>(src + (size_t)y * spitch, x0, w, px);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = (uint8_t)to_gray(px[k * SCN], px[k * SCN + 1], px[k * SCN + 2], g);
    store4(dst + (size_t)y * dpitch, x0, w, out);
}

// BGR -> BGRA (alpha 255): four pixels, 12 bytes in, 16 out
__global__ __launch_bounds__(256) void cvt_bgr2bgra_kernel(const uint8_t* src, int spitch, uint8_t* dst, int dpitch,
                                                           int w)
{
    const int y = blockIdx.y;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x0 >= w) return;
    uint8_t px[12];
    load4px<3>(src + (size_t)y * spitch, x0, w, px);
    uint8_t* D = dst + (size_t)y * dpitch;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint8_t o[4] = {px[3 * k], px[3 * k + 1], px[3 * k + 2], 255};
        store4(D, 4 * (x0 + k), 4 * w, o);  // whole pixels: all four bytes or none
    }
}

// gray -> BGR: four pixels, 4 bytes in, 12 out (three words)
__global__ __launch_bounds__(256) void cvt_gray2bgr_kernel(const uint8_t* src, int spitch, uint8_t* dst, int dpitch,
                                                           int w)
{
    const int y = blockIdx.y;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x0 >= w) return;
    uint8_t px[4];
    load4px<1>(src + (size_t)y * spitch, x0, w, px);
    uint8_t* D = dst + (size_t)y * dpitch;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uint8_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = px[(4 * q + k) / 3];
        store4(D, 3 * x0 + 4 * q, 3 * w, o);
    }
}

// ---- resize ----

// per destination column: the first tap's pixel index, the second's (sx + 1,
// or sx again where the reference's clamp made its weight 0), and the weights
struct XTap {
    int sx0, sx1;
    int a;  // a0 | a1 << 16 (0..2048 each)
};
// per destination row: the two source rows (clipped) and their weights
struct YTap {
    int y0, y1, b0, b1;
};

__device__ __forceinline__ int vresize(int t0, int t1, int b0, int b1)
{
    return (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
}

struct ResizeArgs {
    const uint8_t* src;
    int spitch;
    uint8_t* dst;
    int dpitch;
    int dw, dh;  // destination pixels
    const XTap* xt;
    const YTap* yt;
    int area2;  // both scales exactly 2: (a + b + c + d + 2) >> 2
    Gray3 g;    // fused kernel only
};

// interleaved u8 of CN channels; a thread makes four destination bytes
template <int CN>
__global__ __launch_bounds__(256) void resize_linear_kernel(ResizeArgs a)
{
    const int y = blockIdx.y;
    const int e0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int n = a.dw * CN;
    if (e0 >= n) return;
    uint8_t out[4];
    if (a.area2) {
        const uint8_t* S0 = a.src + (size_t)(2 * y) * a.spitch;
        const uint8_t* S1 = S0 + a.spitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = e0 + k < n ? e0 + k : n - 1;
            const int dx = e / CN, c = e - dx * CN, i = 2 * dx * CN + c;
            out[k] = (uint8_t)((S0[i] + S0[i + CN] + S1[i] + S1[i + CN] + 2) >> 2);
        }
    } else {
        const YTap yt = a.yt[y];
        const uint8_t* S0 = a.src + (size_t)yt.y0 * a.spitch;
        const uint8_t* S1 = a.src + (size_t)yt.y1 * a.spitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = e0 + k < n ? e0 + k : n - 1;
            const int dx = e / CN, c = e - dx * CN;
            const XTap xt = a.xt[dx];
            const int i0 = xt.sx0 * CN + c, i1 = xt.sx1 * CN + c, a0 = xt.a & 0xffff, a1 = xt.a >> 16;
            const int t0 = S0[i0] * a0 + S0[i1] * a1, t1 = S1[i0] * a0 + S1[i1] * a1;
            out[k] = (uint8_t)vresize(t0, t1, yt.b0, yt.b1);
        }
    }
    store4(a.dst + (size_t)y * a.dpitch, e0, n, out);
}

// BGR(A) / RGB(A) -> gray -> resized gray in one pass: every source tap is
// converted to gray, then interpolated, so the bits are those of
// cvt_gray_kernel followed by resize_linear_kernel<1>
template <int SCN>
__global__ __launch_bounds__(256) void cvt_resize_gray_kernel(ResizeArgs a)
{
    const int y = blockIdx.y;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x0 >= a.dw) return;
    uint8_t out[4];
    const Gray3 g = a.g;
    if (a.area2) {
        const uint8_t* S0 = a.src + (size_t)(2 * y) * a.spitch;
        const uint8_t* S1 = S0 + a.spitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dx = x0 + k < a.dw ? x0 + k : a.dw - 1;
            const uint8_t *p0 = S0 + (size_t)(2 * dx) * SCN, *p1 = S1 + (size_t)(2 * dx) * SCN;
            out[k] = (uint8_t)((to_gray(p0[0], p0[1], p0[2], g) + to_gray(p0[SCN], p0[SCN + 1], p0[SCN + 2], g) +
                                to_gray(p1[0], p1[1], p1[2], g) + to_gray(p1[SCN], p1[SCN + 1], p1[SCN + 2], g) + 2) >>
                               2);
        }
    } else {
        const YTap yt = a.yt[y];
        const uint8_t* S0 = a.src + (size_t)yt.y0 * a.spitch;
        const uint8_t* S1 = a.src + (size_t)yt.y1 * a.spitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dx = x0 + k < a.dw ? x0 + k : a.dw - 1;
            const XTap xt = a.xt[dx];
            const int a0 = xt.a & 0xffff, a1 = xt.a >> 16;
            const uint8_t *p00 = S0 + (size_t)xt.sx0 * SCN, *p01 = S0 + (size_t)xt.sx1 * SCN;
            const uint8_t *p10 = S1 + (size_t)xt.sx0 * SCN, *p11 = S1 + (size_t)xt.sx1 * SCN;
            const int t0 = to_gray(p00[0], p00[1], p00[2], g) * a0 + to_gray(p01[0], p01[1], p01[2], g) * a1;
            const int t1 = to_gray(p10[0], p10[1], p10[2], g) * a0 + to_gray(p11[0], p11[1], p11[2], g) * a1;
            out[k] = (uint8_t)vresize(t0, t1, yt.b0, yt.b1);
        }
    }
    store4(a.dst + (size_t)y * a.dpitch, x0, a.dw, out);
}

// ---- host: coefficient tables ----

// saturate_cast<short>(float): cvRound (half to even under the default rounding mode)
inline int sat_short(float v)
{
    const long r = std::lrintf(v);
    return (int)(r < -32768 ? -32768 : (r > 32767 ? 32767 : r));
}

// resize.cpp:3609-3664 for INTER_LINEAR (ksize 2), u8
void make_xtab(int sw, int dw, XTap* out)
{
    const double inv_scale = (double)dw / sw, scale = 1. / inv_scale;
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * scale - 0.5);
        int sx = (int)std::floor(fx);
        fx -= sx;
        if (sx < 0) fx = 0, sx = 0;
        if (sx >= sw - 1) fx = 0, sx = sw - 1;
        const int a0 = sat_short((1.f - fx) * 2048), a1 = sat_short(fx * 2048);
        // past xmax the reference writes S[sx] * 2048 and never reads S[sx + cn];
        // a1 is 0 there, so the second tap may be the first again
        out[dx] = XTap{sx, sx + 1 < sw ? sx + 1 : sx, a0 | (a1 << 16)};
    }
}

// resize.cpp:3666-3702 and the row clip of resizeGeneric_Invoker (:1825)
void make_ytab(int sh, int dh, YTap* out)
{
    const double inv_scale = (double)dh / sh, scale = 1. / inv_scale;
    for (int dy = 0; dy < dh; ++dy) {
        float fy = (float)((dy + 0.5) * scale - 0.5);
        const int sy = (int)std::floor(fy);
        fy -= sy;
        const int y0 = sy < 0 ? 0 : (sy >= sh ? sh - 1 : sy), y1 = sy + 1 < 0 ? 0 : (sy + 1 >= sh ? sh - 1 : sy + 1);
        out[dy] = YTap{y0, y1, sat_short((1.f - fy) * 2048), sat_short(fy * 2048)};
    }
}

}  // namespace

// The context's table cache: a few (source, destination) size pairs, each with
// its device tables.  A repeated size allocates, uploads and waits for nothing.
// A new size takes the least recently used slot.  A slot that held tables before
// may still be read by kernels of earlier calls, on any stream the caller used
// (a hit records nothing, so the slot does not know its readers): the eviction
// drains the device before it overwrites the tables in place, so calls of one
// context on different streams need no ordering by the caller, however many
// sizes are live.
struct FrontScratch {
    static constexpr int kSlots = 8;
    struct Slot {
        int sw = 0, sh = 0, dw = 0, dh = 0;
        XTap* xt = nullptr;
        YTap* yt = nullptr;
        int cap_x = 0, cap_y = 0;
        uint64_t used = 0;
    } slot[kSlots];
    uint64_t tick = 0;
    std::mutex mu;
};

void front_release(tbdk_ctx* ctx)
{
    FrontScratch* F = ctx->front;
    if (!F) return;
    for (auto& sl : F->slot) {
        if (sl.xt) (void)hipFree(sl.xt);
        if (sl.yt) (void)hipFree(sl.yt);
    }
    delete F;
    ctx->front = nullptr;
}

// the slots' tables over their capacity; every key forgotten, so the next call
// of any size builds and uploads its tables again
hipError_t front_debug_fill(tbdk_ctx* ctx, int byte, int64_t* bytes)
{
    FrontScratch* F = ctx->front;
    if (!F) return hipSuccess;
    std::lock_guard<std::mutex> lk(F->mu);
    for (auto& sl : F->slot) {
        sl.sw = sl.sh = sl.dw = sl.dh = 0;
        const std::pair<void*, size_t> bufs[] = {{sl.xt, sizeof(XTap) * (size_t)sl.cap_x},
                                                 {sl.yt, sizeof(YTap) * (size_t)sl.cap_y}};
        for (const auto& b : bufs) {
            if (!b.first || !b.second) continue;
            const hipError_t e = hipMemset(b.first, byte, b.second);
            if (e != hipSuccess) return e;
            *bytes += (int64_t)b.second;
        }
    }
    return hipSuccess;
}

namespace {

int front_tables(tbdk_ctx* ctx, int sw, int sh, int dw, int dh, const XTap** xt, const YTap** yt, hipStream_t s)
{
    if (!ctx->front) ctx->front = new (std::nothrow) FrontScratch();
    FrontScratch* F = ctx->front;
    if (!F) return TBDK_ENOMEM;
    std::lock_guard<std::mutex> lk(F->mu);
    FrontScratch::Slot* pick = &F->slot[0];
    for (auto& sl : F->slot) {
        if (sl.xt && sl.sw == sw && sl.sh == sh && sl.dw == dw && sl.dh == dh) {
            sl.used = ++F->tick;
            *xt = sl.xt, *yt = sl.yt;
            return TBDK_OK;
        }
        if (sl.used < pick->used) pick = &sl;
    }
    if (pick->cap_x < dw) {
        if (pick->xt) (void)hipFree(pick->xt);
        pick->xt = nullptr, pick->cap_x = 0;
        if (dev_alloc(&pick->xt, sizeof(XTap) * (size_t)dw, ctx->opt_alloc_fill) != hipSuccess) return TBDK_ENOMEM;
        pick->cap_x = dw;
    }
    if (pick->cap_y < dh) {
        if (pick->yt) (void)hipFree(pick->yt);
        pick->yt = nullptr, pick->cap_y = 0;
        pick->sw = 0;  // not a valid entry until both tables exist
        if (dev_alloc(&pick->yt, sizeof(YTap) * (size_t)dh, ctx->opt_alloc_fill) != hipSuccess) return TBDK_ENOMEM;
        pick->cap_y = dh;
    }
    std::vector<XTap> hx((size_t)dw);
    std::vector<YTap> hy((size_t)dh);
    make_xtab(sw, dw, hx.data());
    make_ytab(sh, dh, hy.data());
    pick->sw = 0;
    // a new size only: wait for the earlier readers of this slot, whatever their
    // stream (a slot never used has none), then copy before returning (the host
    // tables are locals)
    hipError_t e = pick->used ? hipDeviceSynchronize() : hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(pick->xt, hx.data(), sizeof(XTap) * (size_t)dw, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pick->yt, hy.data(), sizeof(YTap) * (size_t)dh, hipMemcpyHostToDevice);
    if (e != hipSuccess) return map_status(e);
    pick->sw = sw, pick->sh = sh, pick->dw = dw, pick->dh = dh;
    pick->used = ++F->tick;
    *xt = pick->xt, *yt = pick->yt;
    return TBDK_OK;
}

bool overlaps(const uint8_t* src, int sh, int spitch, int srow, const uint8_t* dst, int dh, int dpitch, int drow)
{
    const uint8_t* s1 = src + (size_t)(sh - 1) * spitch + srow;
    const uint8_t* d1 = dst + (size_t)(dh - 1) * dpitch + drow;
    return dst < s1 && src < d1;
}

constexpr int kMaxDim = 1 << 15;  // keeps every byte offset of a row inside int

bool gray_code(int code, int* scn, Gray3* g)
{
    switch (code) {
    case TBDK_COLOR_BGR2GRAY: *scn = 3, *g = Gray3{kB2Y, kG2Y, kR2Y}; return true;
    case TBDK_COLOR_RGB2GRAY: *scn = 3, *g = Gray3{kR2Y, kG2Y, kB2Y}; return true;
    case TBDK_COLOR_BGRA2GRAY: *scn = 4, *g = Gray3{kB2Y, kG2Y, kR2Y}; return true;
    case TBDK_COLOR_RGBA2GRAY: *scn = 4, *g = Gray3{kR2Y, kG2Y, kB2Y}; return true;
    default: return false;
    }
}

inline dim3 row_grid(int elems, int rows) { return dim3((elems + 4 * 256 - 1) / (4 * 256), rows); }

}  // namespace

int front_cvt_color(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, uint8_t* dst,
                    int dst_pitch, int code, hipStream_t s)
{
    if (!ctx || !src || !dst || width <= 0 || height <= 0 || width > kMaxDim || height > kMaxDim) return TBDK_EINVAL;
    int scn = 0, dcn = 1;
    Gray3 g{};
    if (gray_code(code, &scn, &g)) dcn = 1;
    else if (code == TBDK_COLOR_BGR2BGRA) scn = 3, dcn = 4;
    else if (code == TBDK_COLOR_GRAY2BGR) scn = 1, dcn = 3;
    else return TBDK_EINVAL;
    if (src_pitch < (int64_t)width * scn || dst_pitch < (int64_t)width * dcn) return TBDK_EINVAL;
    if (overlaps(src, height, src_pitch, width * scn, dst, height, dst_pitch, width * dcn)) return TBDK_EINVAL;
    const dim3 grid = row_grid(width, height), block(256);
    const int rec = timing_begin(ctx, "cvt_color", s);
    if (code == TBDK_COLOR_BGR2BGRA)
        hipLaunchKernelGGL(cvt_bgr2bgra_kernel, grid, block, 0, s, src, src_pitch, dst, dst_pitch, width);
    else if (code == TBDK_COLOR_GRAY2BGR)
        hipLaunchKernelGGL(cvt_gray2bgr_kernel, grid, block, 0, s, src, src_pitch, dst, dst_pitch, width);
    else if (scn == 3)
        hipLaunchKernelGGL(cvt_gray_kernel<3>, grid, block, 0, s, src, src_pitch, dst, dst_pitch, width, g);
    else
        hipLaunchKernelGGL(cvt_gray_kernel<4>, grid, block, 0, s, src, src_pitch, dst, dst_pitch, width, g);
    timing_end(ctx, rec, s);
    return map_status(hipGetLastError());
}

// gray_code < 0: plain resize of cn channels; else the fused colour -> gray -> resize
static int front_resize_impl(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, int cn,
                             int code, uint8_t* dst, int dst_width, int dst_height, int dst_pitch, hipStream_t s)
{
    if (!ctx || !src || !dst || width <= 0 || height <= 0 || dst_width <= 0 || dst_height <= 0 || width > kMaxDim ||
        height > kMaxDim || dst_width > kMaxDim || dst_height > kMaxDim)
        return TBDK_EINVAL;
    Gray3 g{};
    int dcn = cn;
    if (code >= 0) {
        if (!gray_code(code, &cn, &g)) return TBDK_EINVAL;
        dcn = 1;
    } else if (cn != 1 && cn != 3 && cn != 4) {
        return TBDK_EINVAL;
    }
    if (src_pitch < (int64_t)width * cn || dst_pitch < (int64_t)dst_width * dcn) return TBDK_EINVAL;
    if (overlaps(src, height, src_pitch, width * cn, dst, dst_height, dst_pitch, dst_width * dcn)) return TBDK_EINVAL;
    if (dst_width == width && dst_height == height) {  // the reference copies
        if (code >= 0) return front_cvt_color(ctx, src, width, height, src_pitch, dst, dst_pitch, code, s);
        const int rec = timing_begin(ctx, "resize_linear", s);
        const hipError_t e = hipMemcpy2DAsync(dst, (size_t)dst_pitch, src, (size_t)src_pitch, (size_t)width * cn,
                                              (size_t)height, hipMemcpyDeviceToDevice, s);
        timing_end(ctx, rec, s);
        return map_status(e);
    }
    ResizeArgs a{};
    a.src = src, a.spitch = src_pitch, a.dst = dst, a.dpitch = dst_pitch, a.dw = dst_width, a.dh = dst_height;
    a.area2 = width == 2 * dst_width && height == 2 * dst_height;
    a.g = g;
    if (!a.area2) {
        const int rc = front_tables(ctx, width, height, dst_width, dst_height, &a.xt, &a.yt, s);
        if (rc != TBDK_OK) return rc;
    }
    const dim3 grid = row_grid(dst_width * dcn, dst_height), block(256);
    const int rec = timing_begin(ctx, code >= 0 ? "cvt_resize_gray" : "resize_linear", s);
    if (code >= 0) {
        if (cn == 3) hipLaunchKernelGGL(cvt_resize_gray_kernel<3>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(cvt_resize_gray_kernel<4>, grid, block, 0, s, a);
    } else if (cn == 1) {
        hipLaunchKernelGGL(resize_linear_kernel<1>, grid, block, 0, s, a);
    } else if (cn == 3) {
        hipLaunchKernelGGL(resize_linear_kernel<3>, grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL(resize_linear_kernel<4>, grid, block, 0, s, a);
    }
    timing_end(ctx, rec, s);
    return map_status(hipGetLastError());
}

int front_resize_linear(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, int cn, uint8_t* dst,
                        int dst_width, int dst_height, int dst_pitch, hipStream_t s)
{
    return front_resize_impl(ctx, src, width, height, src_pitch, cn, -1, dst, dst_width, dst_height, dst_pitch, s);
}

int front_cvt_resize_gray(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, int code,
                          uint8_t* dst, int dst_width, int dst_height, int dst_pitch, hipStream_t s)
{
    if (code < 0) return TBDK_EINVAL;
    return front_resize_impl(ctx, src, width, height, src_pitch, 0, code, dst, dst_width, dst_height, dst_pitch, s);
}

}  // namespace tbdk

using namespace tbdk;

extern "C" {

int tbdk_cvt_color_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, uint8_t* dst,
                      int dst_pitch, int code, void* stream)
{
    if (!ctx) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    return front_cvt_color(ctx, src, width, height, src_pitch, dst, dst_pitch, code, static_cast<hipStream_t>(stream));
}

int tbdk_resize_linear_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, int cn,
                          uint8_t* dst, int dst_width, int dst_height, int dst_pitch, void* stream)
{
    if (!ctx) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    return front_resize_linear(ctx, src, width, height, src_pitch, cn, dst, dst_width, dst_height, dst_pitch,
                               static_cast<hipStream_t>(stream));
}

int tbdk_cvt_resize_gray_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, int code,
                            uint8_t* dst, int dst_width, int dst_height, int dst_pitch, void* stream)
{
    if (!ctx) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    return front_cvt_resize_gray(ctx, src, width, height, src_pitch, code, dst, dst_width, dst_height, dst_pitch,
                                 static_cast<hipStream_t>(stream));
}

}  // extern "C"
