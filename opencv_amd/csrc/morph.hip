// morph.hip — cv::erode / cv::dilate / cv::morphologyEx (OPEN, CLOSE) on 8UC1
// device images (imgproc/src/morph.dispatch.cpp, morph.simd.hpp).
//
// The result of one pass is, per pixel, the min (erode) or max (dilate) over
// the element's non-zero positions of the border-extended image: that is what
// the reference's FilterEngine computes, for a rectangle as a row pass then a
// column pass (the extension is separable, so the two passes over it give the
// same min / max as the rectangle at once), for any other element as one 2-D
// pass.  One kernel does all three: a workgroup stages its 64 x 16 output tile
// plus the element's halo in LDS, with the border resolved while staging
// (remap_core.hpp's closed-form borderInterpolate, which holds for images
// smaller than the element), then every lane walks the element's row masks over
// LDS.  The row pass is the kw x 1 element, the column pass the 1 x kh one.
// The element travels in the kernel arguments (31 row masks, 124 bytes): a call
// uploads nothing, allocates nothing once the context's scratch has the size,
// and never synchronises.
//
// LDS: bytes, a row of the staged tile is 64 + kw - 1 <= 94 bytes.  A wave reads
// 64 consecutive bytes of one row per tap: 16 dwords, one bank each, four lanes
// per dword (a broadcast), so no conflict whatever the row length.
#include <cstring>

#include "morph_host.hpp"
#include "remap_core.hpp"
#include "tbdk_internal.hpp"

namespace tbdk {
namespace {

static_assert(TBDK_BORDER_CONSTANT == remap_core::kConstant && TBDK_BORDER_REPLICATE == remap_core::kReplicate &&
                  TBDK_BORDER_REFLECT == remap_core::kReflect && TBDK_BORDER_REFLECT_101 == remap_core::kReflect101,
              "border values");

constexpr int kTileW = 64, kTileH = 16, kThreads = 256;
constexpr int kMaxSide = morph_host::kMaxSide;
constexpr int kLdsBytes = (kTileW + kMaxSide - 1) * (kTileH + kMaxSide - 1);

struct MorphArgs {
    const uint8_t* src;
    uint8_t* dst;
    int width, height, spitch, dpitch;
    int kw, kh, ax, ay;
    int border;   // TBDK_BORDER_*
    int bval;     // what a pixel outside counts as under BORDER_CONSTANT
    uint32_t rows[kMaxSide];
};

template <bool DILATE>
__global__ __launch_bounds__(kThreads) void morph_kernel(const MorphArgs a)
{
    __shared__ uint8_t tile[kLdsBytes];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int lw = kTileW + a.kw - 1, lh = kTileH + a.kh - 1;
    // stage the tile and its halo; rows and columns past the image's last tile
    // pixel are staged too (border-mapped, so every index stays inside) and never used
    for (int i = threadIdx.x; i < lw * lh; i += kThreads) {
        const int ly = i / lw, lx = i - ly * lw;
        const int sx = remap_core::border_interp(x0 - a.ax + lx, a.width, a.border);
        const int sy = remap_core::border_interp(y0 - a.ay + ly, a.height, a.border);
        tile[i] = (sx < 0 || sy < 0) ? (uint8_t)a.bval : a.src[(size_t)sy * a.spitch + sx];
    }
    __syncthreads();
    const int tx = threadIdx.x % kTileW;
    for (int ty = threadIdx.x / kTileW; ty < kTileH; ty += kThreads / kTileW) {
        const int x = x0 + tx, y = y0 + ty;
        if (x >= a.width || y >= a.height) continue;
        int v = DILATE ? 0 : 255;
        for (int r = 0; r < a.kh; ++r) {
            const uint8_t* row = tile + (ty + r) * lw + tx;
            for (uint32_t m = a.rows[r]; m; m &= m - 1) {
                const int t = row[__builtin_ctz(m)];
                v = DILATE ? (t > v ? t : v) : (t < v ? t : v);
            }
        }
        a.dst[(size_t)y * a.dpitch + x] = (uint8_t)v;
    }
}

struct Image {
    const uint8_t* p;
    int pitch;
};

// one element application src -> dst (the ranges may not overlap unless the element is 1 x 1 and src == dst)
hipError_t launch_pass(bool dilate, const Image& src, uint8_t* dst, int dpitch, int width, int height, int kw, int kh,
                       int ax, int ay, const uint32_t* rows, int border, int bval, hipStream_t s)
{
    MorphArgs a;
    std::memset(&a, 0, sizeof a);
    a.src = src.p;
    a.dst = dst;
    a.width = width;
    a.height = height;
    a.spitch = src.pitch;
    a.dpitch = dpitch;
    a.kw = kw;
    a.kh = kh;
    a.ax = ax;
    a.ay = ay;
    a.border = border;
    a.bval = bval;
    for (int i = 0; i < kh; ++i) a.rows[i] = rows[i];
    const dim3 grid((width + kTileW - 1) / kTileW, (height + kTileH - 1) / kTileH);
    if (dilate)
        hipLaunchKernelGGL(morph_kernel<true>, grid, dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL(morph_kernel<false>, grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

struct Pass {
    bool dilate;
    int kw, kh, ax, ay;
    const uint32_t* rows;
};

}  // namespace

hipError_t blob_scratch(tbdk_ctx* ctx, void** buf, size_t* cap, size_t need)
{
    if (*cap >= need) return hipSuccess;
    if (*buf) (void)hipFree(*buf);  // waits for the device: nothing reads the old block any more
    *buf = nullptr;
    *cap = 0;
    const hipError_t e = dev_alloc(buf, need, ctx->opt_alloc_fill);
    if (e == hipSuccess) *cap = need;
    return e;
}

}  // namespace tbdk

using namespace tbdk;

extern "C" {

int tbdk_structuring_element(int shape, int kw, int kh, int anchor_x, int anchor_y, uint8_t* out)
{
    return morph_host::structuring_element(shape, kw, kh, anchor_x, anchor_y, out) ? TBDK_OK : TBDK_EINVAL;
}

int tbdk_morph_u8(tbdk_ctx* ctx, int op, const uint8_t* src, int width, int height, int src_pitch, uint8_t* dst,
                  int dst_pitch, const uint8_t* element, int kw, int kh, int anchor_x, int anchor_y, int iterations,
                  int border_type, int border_value, void* stream)
{
    if (!ctx || !src || !dst) return TBDK_EINVAL;
    if (op != TBDK_MORPH_ERODE && op != TBDK_MORPH_DILATE && op != TBDK_MORPH_OPEN && op != TBDK_MORPH_CLOSE)
        return TBDK_EINVAL;
    if (width < 1 || height < 1 || width > 65535 || height > 65535 || src_pitch < width || dst_pitch < width)
        return TBDK_EINVAL;
    if (border_type != TBDK_BORDER_CONSTANT && border_type != TBDK_BORDER_REPLICATE &&
        border_type != TBDK_BORDER_REFLECT && border_type != TBDK_BORDER_REFLECT_101)
        return TBDK_EINVAL;
    if (border_value < -1 || border_value > 255) return TBDK_EINVAL;
    morph_host::Plan plan;
    if (!morph_host::make_plan(element, kw, kh, anchor_x, anchor_y, iterations, &plan)) return TBDK_EINVAL;

    // the element applications, in order
    uint32_t kOne[kMaxSide];  // a column: one entry in each of up to 31 rows
    for (int i = 0; i < kMaxSide; ++i) kOne[i] = 1u;
    const uint32_t row_mask[1] = {(1u << plan.kw) - 1u};  // a row: kw <= 31 entries
    Pass passes[2 * 2 * 64];
    int n = 0;
    const bool first_dilate = op == TBDK_MORPH_DILATE || op == TBDK_MORPH_CLOSE;
    const int stages = (op == TBDK_MORPH_OPEN || op == TBDK_MORPH_CLOSE) ? 2 : 1;
    if (!plan.copy) {
        if (!plan.rect && plan.passes > 64) return TBDK_EINVAL;
        for (int st = 0; st < stages; ++st) {
            const bool dil = st == 0 ? first_dilate : !first_dilate;
            for (int it = 0; it < plan.passes; ++it) {
                if (!plan.rect) {
                    passes[n++] = Pass{dil, plan.kw, plan.kh, plan.ax, plan.ay, plan.rows};
                    continue;
                }
                if (plan.kw > 1) passes[n++] = Pass{dil, plan.kw, 1, plan.ax, 0, row_mask};
                if (plan.kh > 1) passes[n++] = Pass{dil, 1, plan.kh, 0, plan.ay, kOne};
            }
        }
    }
    // src and dst may be one image or overlap: then no pass reads what another workgroup of it writes
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + (size_t)(height - 1) * src_pitch + width;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (size_t)(height - 1) * dst_pitch + width;
    const bool overlap = s0 < d1 && d0 < s1;
    // (with two or more passes the first writes scratch and the last reads it)
    const Pass identity{false, 1, 1, 0, 0, kOne};
    if (n == 0) {
        if (src == dst && src_pitch == dst_pitch) return TBDK_OK;  // a copy onto itself
        passes[n++] = identity;
    }
    if (n == 1 && overlap) passes[n++] = identity;  // through scratch, then copied out

    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t plane = ((size_t)width * height + 255) & ~(size_t)255;
    uint8_t* buf[2] = {nullptr, nullptr};
    if (n > 1) {
        const hipError_t e = blob_scratch(ctx, &ctx->morph_buf, &ctx->morph_cap, plane * (n > 2 ? 2 : 1));
        if (e != hipSuccess) return map_status(e);
        buf[0] = static_cast<uint8_t*>(ctx->morph_buf);
        buf[1] = buf[0] + plane;
    }
    // under BORDER_CONSTANT a pixel outside counts as the border value; the default one is neutral
    const int rec = timing_begin(ctx, "morph", s);
    hipError_t e = hipSuccess;
    Image cur{src, src_pitch};
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        const Pass& p = passes[i];
        const bool last = i == n - 1;
        uint8_t* out = last ? dst : buf[i & 1];
        const int opitch = last ? dst_pitch : width;
        const int bval = border_value >= 0 ? border_value : (p.dilate ? 0 : 255);
        e = launch_pass(p.dilate, cur, out, opitch, width, height, p.kw, p.kh, p.ax, p.ay, p.rows, border_type, bval, s);
        cur = Image{out, opitch};
    }
    timing_end(ctx, rec, s);
    return map_status(e);
}

}  // extern "C"
