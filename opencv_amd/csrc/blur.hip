// blur.hip — cv::GaussianBlur on 8-bit device images (the integer path,
// GaussianBlurFixedPoint of imgproc/src/smooth.simd.hpp) and cv::threshold on 8U
// and 32F device images, with THRESH_OTSU (imgproc/src/thresh.cpp).
//
// The blur is one launch.  An image row is width * cn bytes and the kernel works
// on bytes: tap i of the row pass lies i * cn bytes on.  A workgroup of 256 lanes
// owns a tile of 128 bytes x 32 rows of the output.  It
//   1. stages the tile and its halo in LDS as bytes, the border resolved while
//      staging (remap_core.hpp's closed-form borderInterpolate, which holds for
//      images smaller than the kernel; BORDER_CONSTANT stages zeros, which is what
//      leaving the terms out amounts to).  A tile whose halo lies inside the image
//      takes no border branch and, where pointer and pitch allow, loads dwords;
//   2. row pass: a lane makes four neighbouring 8.8 sums H = min(65535, sum kx s)
//      from dword reads (two aligned dwords and v_alignbyte per tap) and stores
//      them as four 16-bit words (one 8-byte write);
//   3. column pass: a lane makes four neighbouring outputs
//      min(255, (sum ky H + 32768) >> 16) from one 8-byte read per tap, applies the
//      optional threshold stage and stores a dword (bytes at an unaligned or
//      partial position).
// No 16-bit plane goes to memory; the coefficients travel in the kernel arguments.
// The 32-bit column sum cannot reach 2^32 (at most 31 * 256 * 65535), so the
// reference's saturating 32-bit adds never act.
//
// LDS: 248 x 62 bytes of source and 128 x 62 words of H at most, 31.3 KB, five
// workgroups a CU.  Row pass: the 32 lanes of a row read consecutive dwords, the
// two rows a wave covers lie a multiple of 4 bytes apart, so a wave's read
// touches at most two distinct dwords per bank half.  Column pass: a lane reads 8
// bytes, 32 lanes one H row of 256 bytes: consecutive, conflict-free whatever the
// row stride.
#include <cmath>
#include <cstring>
#include <limits>

#include "blur_host.hpp"
#include "remap_core.hpp"
#include "tbdk_internal.hpp"

namespace tbdk {

hipError_t blob_scratch(tbdk_ctx* ctx, void** buf, size_t* cap, size_t need);  // morph.hip

namespace {

static_assert(TBDK_BORDER_CONSTANT == remap_core::kConstant && TBDK_BORDER_REPLICATE == remap_core::kReplicate &&
                  TBDK_BORDER_REFLECT == remap_core::kReflect && TBDK_BORDER_REFLECT_101 == remap_core::kReflect101 &&
                  TBDK_BORDER_WRAP == remap_core::kWrap,
              "border values");
static_assert(TBDK_THRESH_BINARY == blur_host::kBinary && TBDK_THRESH_TOZERO_INV == blur_host::kToZeroInv &&
                  TBDK_THRESH_OTSU == blur_host::kOtsu && TBDK_THRESH_TRIANGLE == blur_host::kTriangle,
              "threshold types");

constexpr int kTileW = 128, kTileH = 32, kThreads = 256;  // bytes x rows
constexpr int kMaxK = blur_host::kMaxK;
constexpr int kGroups = kTileW / 4;                               // four-byte groups a tile row
constexpr int kMaxLw = 2 * ((kMaxK / 2) * 4) + kTileW;            // staged row, bytes (cn 4, 31 taps): 248
constexpr int kMaxLh = kTileH + kMaxK - 1;                        // staged rows: 62

// v > ithresh ? hi : lo, each a constant or (-1) v itself
struct ThreshRule {
    int ithresh, hi, lo;
};

struct BlurArgs {
    const uint8_t* src;
    uint8_t* dst;
    int width, height, cn, spitch, dpitch;
    int kw, kh, border;
    int fuse;  // != 0: rule applied to every output byte
    ThreshRule rule;
    uint16_t kx[kMaxK + 1], ky[kMaxK + 1];
};

__device__ __forceinline__ int apply_rule(const ThreshRule& r, int v)
{
    return v > r.ithresh ? (r.hi < 0 ? v : r.hi) : (r.lo < 0 ? v : r.lo);
}

// KW, KH > 0: the sizes are compile-time (a.kw == KW, a.kh == KH); 0: run-time sizes up to 31
template <int KW, int KH>
__global__ __launch_bounds__(kThreads) void blur_kernel(const BlurArgs a)
{
    __shared__ uint32_t s_src[kMaxLw / 4 * kMaxLh + 1];  // + 1: the row pass reads one dword past its last tap
    __shared__ uint2 s_h[kGroups * kMaxLh];
    const int kw = KW ? KW : a.kw, kh = KH ? KH : a.kh, cn = a.cn;
    const int ax = kw / 2, ay = kh / 2;
    const int wb = a.width * cn;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int padl = (ax * cn + 3) & ~3, padr = ((kw - 1 - ax) * cn + 3) & ~3;
    const int lwd = (padl + kTileW + padr) >> 2;  // staged row, dwords
    const int lh = kTileH + kh - 1;
    const int gx0 = x0 - padl, gy0 = y0 - ay;     // the staged tile's first byte column and row

    // 1. stage
    const bool inside = gx0 >= 0 && gx0 + 4 * lwd <= wb && gy0 >= 0 && gy0 + lh <= a.height;
    if (inside && ((reinterpret_cast<uintptr_t>(a.src) | (unsigned)a.spitch) & 3) == 0) {
        for (int i = threadIdx.x; i < lwd * lh; i += kThreads) {
            const int ly = i / lwd, lx = i - ly * lwd;
            s_src[i] = *reinterpret_cast<const uint32_t*>(a.src + (size_t)(gy0 + ly) * a.spitch + gx0 + 4 * lx);
        }
    } else if (inside) {
        for (int i = threadIdx.x; i < lwd * lh; i += kThreads) {
            const int ly = i / lwd, lx = i - ly * lwd;
            const uint8_t* p = a.src + (size_t)(gy0 + ly) * a.spitch + gx0 + 4 * lx;
            s_src[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
    } else {
        // columns and rows past the image's last tile pixel are staged too (border-mapped, so every index stays
        // inside) and never stored
        for (int i = threadIdx.x; i < lwd * lh; i += kThreads) {
            const int ly = i / lwd, lx = i - ly * lwd;
            const int sy = remap_core::border_interp(gy0 + ly, a.height, a.border);
            uint32_t v = 0;
            for (int q = 0; q < 4; ++q) {
                const int gb = gx0 + 4 * lx + q;
                const int px = gb >= 0 ? gb / cn : -((-gb + cn - 1) / cn);  // floor
                const int c = gb - px * cn;
                const int sx = remap_core::border_interp(px, a.width, a.border);
                const uint32_t b = (sx < 0 || sy < 0) ? 0u : a.src[(size_t)sy * a.spitch + sx * cn + c];
                v |= b << (8 * q);
            }
            s_src[i] = v;
        }
    }
    __syncthreads();

    // 2. row pass over every staged row
    const int o0 = padl - ax * cn;  // byte of tap 0 of the tile's first output column: 0..3
    for (int it = threadIdx.x; it < lh * kGroups; it += kThreads) {
        const int r = it / kGroups, g = it - r * kGroups;
        const uint32_t* row = s_src + r * lwd + g;
        uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
#pragma unroll KW ? KW : 1
        for (int i = 0; i < kw; ++i) {
            const int o = o0 + i * cn;
            const uint32_t lo = row[o >> 2], hi = row[(o >> 2) + 1];
            const uint32_t d = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(o & 3));
            const uint32_t k = a.kx[i];
            acc0 += k * (d & 255u);
            acc1 += k * ((d >> 8) & 255u);
            acc2 += k * ((d >> 16) & 255u);
            acc3 += k * (d >> 24);
        }
        acc0 = acc0 < 65535u ? acc0 : 65535u;
        acc1 = acc1 < 65535u ? acc1 : 65535u;
        acc2 = acc2 < 65535u ? acc2 : 65535u;
        acc3 = acc3 < 65535u ? acc3 : 65535u;
        s_h[it] = make_uint2(acc0 | (acc1 << 16), acc2 | (acc3 << 16));
    }
    __syncthreads();

    // 3. column pass
    const bool dword_out = ((reinterpret_cast<uintptr_t>(a.dst) | (unsigned)a.dpitch) & 3) == 0;
    for (int it = threadIdx.x; it < kTileH * kGroups; it += kThreads) {
        const int ty = it / kGroups, g = it - ty * kGroups;
        const int y = y0 + ty, xb = x0 + 4 * g;
        if (y >= a.height || xb >= wb) continue;
        uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
#pragma unroll KH ? KH : 1
        for (int j = 0; j < kh; ++j) {
            const uint2 h = s_h[(ty + j) * kGroups + g];
            const uint32_t k = a.ky[j];
            acc0 += k * (h.x & 65535u);
            acc1 += k * (h.x >> 16);
            acc2 += k * (h.y & 65535u);
            acc3 += k * (h.y >> 16);
        }
        int v[4] = {(int)((acc0 + 32768u) >> 16), (int)((acc1 + 32768u) >> 16), (int)((acc2 + 32768u) >> 16),
                    (int)((acc3 + 32768u) >> 16)};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = v[q] < 255 ? v[q] : 255;
            if (a.fuse) v[q] = apply_rule(a.rule, v[q]);
        }
        uint8_t* out = a.dst + (size_t)y * a.dpitch + xb;
        if (dword_out && xb + 4 <= wb) {
            *reinterpret_cast<uint32_t*>(out) =
                (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (xb + q < wb) out[q] = (uint8_t)v[q];
        }
    }
}

// ---- threshold ---------------------------------------------------------------------------------------------------

struct ThreshArgs {
    const uint8_t* src;
    uint8_t* dst;
    int wb, height, spitch, dpitch;  // wb: bytes (8U) or floats (32F) a row
    ThreshRule rule;
    const int32_t* dev_thresh;  // Otsu: the threshold is read here; TRUNC's constant is then the threshold too
    int trunc;
    float fthresh, fmaxval;
    int type;
};

__global__ __launch_bounds__(kThreads) void thresh_u8_kernel(const ThreshArgs a)
{
    ThreshRule r = a.rule;
    if (a.dev_thresh) {
        r.ithresh = *a.dev_thresh;
        if (a.trunc) r.hi = r.ithresh;  // 0..255
    }
    const int y = blockIdx.y;
    const uint8_t* s = a.src + (size_t)y * a.spitch;
    uint8_t* d = a.dst + (size_t)y * a.dpitch;
    const bool dwords =
        ((reinterpret_cast<uintptr_t>(a.src) | reinterpret_cast<uintptr_t>(a.dst) | (unsigned)a.spitch | (unsigned)a.dpitch) & 3) == 0;
    const int x = (blockIdx.x * kThreads + threadIdx.x) * 4;
    if (x >= a.wb) return;
    if (dwords && x + 4 <= a.wb) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(s + x);
        uint32_t o = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) o |= (uint32_t)apply_rule(r, (int)((v >> (8 * q)) & 255u)) << (8 * q);
        *reinterpret_cast<uint32_t*>(d + x) = o;
    } else {
        for (int q = 0; q < 4 && x + q < a.wb; ++q) d[x + q] = (uint8_t)apply_rule(r, s[x + q]);
    }
}

// the comparisons of thresh_32f's vector body: `thresh < v` and `v <= thresh` are false for a NaN v; TRUNC is
// minps(v, thresh), thresh unless v < thresh
__global__ __launch_bounds__(kThreads) void thresh_f32_kernel(const ThreshArgs a)
{
    const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
    if (x >= a.wb) return;
    const float v = reinterpret_cast<const float*>(a.src + (size_t)y * a.spitch)[x];
    const float t = a.fthresh, m = a.fmaxval;
    float o;
    switch (a.type) {
    case TBDK_THRESH_BINARY: o = t < v ? m : 0.f; break;
    case TBDK_THRESH_BINARY_INV: o = v <= t ? m : 0.f; break;
    case TBDK_THRESH_TRUNC: o = v < t ? v : t; break;
    case TBDK_THRESH_TOZERO: o = t < v ? v : 0.f; break;
    default: o = v <= t ? v : 0.f; break;
    }
    reinterpret_cast<float*>(a.dst + (size_t)y * a.dpitch)[x] = o;
}

// 256 bins of a pitched 8-bit image, added to hist (zeroed by the caller on the stream)
__global__ __launch_bounds__(kThreads) void hist_u8_kernel(const uint8_t* src, int width, int height, int pitch,
                                                           uint32_t* hist)
{
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int y0 = blockIdx.x * 16;
    for (int y = y0; y < y0 + 16 && y < height; ++y) {
        const uint8_t* row = src + (size_t)y * pitch;
        for (int x = threadIdx.x; x < width; x += kThreads) atomicAdd(&s_hist[row[x]], 1u);
    }
    __syncthreads();
    if (s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_hist[threadIdx.x]);
}

// getThreshVal_Otsu_8u's scan (thresh.cpp:1182-1218) on one lane, in double, in the reference's operation order
// (the library is built without contraction); total: width * height as the reference's int product
__global__ void otsu_scan_kernel(const uint32_t* hist, int total, int32_t* out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double eps = (double)std::numeric_limits<float>::epsilon();
    double mu = 0, scale = 1. / total;
    for (int i = 0; i < 256; ++i) mu += i * (double)(int)hist[i];
    mu *= scale;
    double mu1 = 0, q1 = 0, max_sigma = 0;
    int max_val = 0;
    for (int i = 0; i < 256; ++i) {
        const double p_i = (int)hist[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1. - q1;
        const double lo = q2 < q1 ? q2 : q1, hi = q1 < q2 ? q2 : q1;  // std::min, std::max
        if (lo < eps || hi > 1. - eps) continue;
        mu1 = (mu1 + i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) {
            max_sigma = sigma;
            max_val = i;
        }
    }
    *out = max_val;
}

template <int KW, int KH>
void launch_blur(const BlurArgs& a, hipStream_t s)
{
    const dim3 grid((a.width * a.cn + kTileW - 1) / kTileW, (a.height + kTileH - 1) / kTileH);
    hipLaunchKernelGGL((blur_kernel<KW, KH>), grid, dim3(kThreads), 0, s, a);
}

bool rule_from(const tbdk_thresh_params* t, ThreshRule* r, double* used)
{
    blur_host::ThreshPlan p;
    if (!blur_host::thresh_plan_u8(t->thresh, t->maxval, t->type, &p)) return false;
    r->ithresh = p.ithresh;
    r->hi = p.hi_const;
    r->lo = p.lo_const;
    if (used) *used = (double)p.ithresh;
    return true;
}

bool overlaps(const void* src, int spitch, const void* dst, int dpitch, int height, int row_bytes)
{
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + (size_t)(height - 1) * spitch + row_bytes;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (size_t)(height - 1) * dpitch + row_bytes;
    return s0 < d1 && d0 < s1;
}

}  // namespace
}  // namespace tbdk

using namespace tbdk;

extern "C" {

int tbdk_gaussian_kernel_u8(int n, double sigma, uint16_t* out)
{
    if (!(sigma == sigma)) return TBDK_EINVAL;
    return blur_host::gaussian_kernel_u8(n, sigma, out) ? TBDK_OK : TBDK_EINVAL;
}

int tbdk_gaussian_blur_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int cn, int src_pitch,
                          uint8_t* dst, int dst_pitch, int kw, int kh, double sigma_x, double sigma_y,
                          int border_type, const tbdk_thresh_params* fused, void* stream)
{
    if (!ctx || !src || !dst) return TBDK_EINVAL;
    if (cn != 1 && cn != 3 && cn != 4) return TBDK_EINVAL;
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return TBDK_EINVAL;
    const int wb = width * cn;
    if (src_pitch < wb || dst_pitch < wb) return TBDK_EINVAL;
    if (border_type != TBDK_BORDER_CONSTANT && border_type != TBDK_BORDER_REPLICATE &&
        border_type != TBDK_BORDER_REFLECT && border_type != TBDK_BORDER_REFLECT_101 && border_type != TBDK_BORDER_WRAP)
        return TBDK_EINVAL;
    blur_host::BlurPlan plan;
    if (!blur_host::make_plan(width, height, kw, kh, sigma_x, sigma_y, border_type, &plan)) return TBDK_EINVAL;
    BlurArgs a;
    std::memset(&a, 0, sizeof a);
    if (fused) {
        if (!rule_from(fused, &a.rule, nullptr)) return TBDK_EINVAL;
        a.fuse = 1;
    }
    const bool same = src == dst && src_pitch == dst_pitch;
    if (plan.copy && !fused && same) return TBDK_OK;  // a copy onto itself
    const bool through = !(plan.copy && same) && overlaps(src, src_pitch, dst, dst_pitch, height, wb);

    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tpitch = (wb + 3) & ~3;
    if (through) {
        const hipError_t e = blob_scratch(ctx, &ctx->morph_buf, &ctx->morph_cap, (size_t)tpitch * height);
        if (e != hipSuccess) return map_status(e);
    }
    a.src = src;
    a.dst = through ? static_cast<uint8_t*>(ctx->morph_buf) : dst;
    a.width = width;
    a.height = height;
    a.cn = cn;
    a.spitch = src_pitch;
    a.dpitch = through ? tpitch : dst_pitch;
    a.kw = plan.kw;
    a.kh = plan.kh;
    a.border = border_type;
    for (int i = 0; i < plan.kw; ++i) a.kx[i] = plan.kx[i];
    for (int i = 0; i < plan.kh; ++i) a.ky[i] = plan.ky[i];
    const int rec = timing_begin(ctx, "blur", s);
    const int inst = (plan.kw == plan.kh && !ctx->opt_blur_generic) ? plan.kw : 0;
    switch (inst) {
    case 3: launch_blur<3, 3>(a, s); break;
    case 5: launch_blur<5, 5>(a, s); break;
    case 7: launch_blur<7, 7>(a, s); break;
    case 11: launch_blur<11, 11>(a, s); break;
    default: launch_blur<0, 0>(a, s); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && through) {  // copied out by the one-tap kernel: 256 * 256 * v + 32768 >> 16 is v
        BlurArgs c;
        std::memset(&c, 0, sizeof c);
        c.src = a.dst;
        c.dst = dst;
        c.width = width;
        c.height = height;
        c.cn = cn;
        c.spitch = tpitch;
        c.dpitch = dst_pitch;
        c.kw = c.kh = 1;
        c.border = TBDK_BORDER_REPLICATE;
        c.kx[0] = c.ky[0] = 256;
        launch_blur<0, 0>(c, s);
        e = hipGetLastError();
    }
    timing_end(ctx, rec, s);
    return map_status(e);
}

int tbdk_threshold(tbdk_ctx* ctx, const void* src, int pix, int width, int height, int cn, int src_pitch, void* dst,
                   int dst_pitch, double thresh, double maxval, int type, double* thresh_used, int32_t* otsu_dev,
                   void* stream)
{
    if (!ctx || !src || !dst) return TBDK_EINVAL;
    if (pix != TBDK_PIX_U8 && pix != TBDK_PIX_F32) return TBDK_EINVAL;
    if (width < 1 || height < 1 || width > 65535 || height > 65535 || cn < 1 || cn > 512) return TBDK_EINVAL;
    const int plain = type & TBDK_THRESH_MASK;
    if ((type & ~(TBDK_THRESH_MASK | TBDK_THRESH_OTSU)) != 0 || plain > TBDK_THRESH_TOZERO_INV) return TBDK_EINVAL;
    const bool otsu = (type & TBDK_THRESH_OTSU) != 0;
    if (otsu && (pix != TBDK_PIX_U8 || cn != 1 || !otsu_dev)) return TBDK_EINVAL;
    if (otsu && (int64_t)width * height > 0x7fffffff) return TBDK_EINVAL;  // the reference's int pixel count
    if (!(maxval == maxval) || (!otsu && !(thresh == thresh))) return TBDK_EINVAL;
    const int wb = width * cn, row_bytes = pix == TBDK_PIX_F32 ? wb * 4 : wb;
    if (src_pitch < row_bytes || dst_pitch < row_bytes) return TBDK_EINVAL;
    ThreshArgs a;
    std::memset(&a, 0, sizeof a);
    a.src = static_cast<const uint8_t*>(src);
    a.dst = static_cast<uint8_t*>(dst);
    a.wb = wb;
    a.height = height;
    a.spitch = src_pitch;
    a.dpitch = dst_pitch;
    a.type = plain;
    double used = std::numeric_limits<double>::quiet_NaN();
    if (pix == TBDK_PIX_F32) {
        if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (unsigned)src_pitch | (unsigned)dst_pitch) & 3) != 0)
            return TBDK_EINVAL;
        a.fthresh = (float)thresh;
        a.fmaxval = (float)maxval;
        used = thresh;
    } else {
        const tbdk_thresh_params t{otsu ? 0.0 : thresh, maxval, plain, 0};
        if (!rule_from(&t, &a.rule, otsu ? nullptr : &used)) return TBDK_EINVAL;
        a.trunc = plain == TBDK_THRESH_TRUNC;
    }
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* hist = nullptr;
    if (otsu) {
        const hipError_t e = blob_scratch(ctx, &ctx->morph_buf, &ctx->morph_cap, 1024);
        if (e != hipSuccess) return map_status(e);
        hist = static_cast<uint32_t*>(ctx->morph_buf);
    }
    const int rec = timing_begin(ctx, "threshold", s);
    hipError_t e = hipSuccess;
    if (otsu) {
        e = hipMemsetAsync(hist, 0, 1024, s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(hist_u8_kernel, dim3((height + 15) / 16), dim3(kThreads), 0, s, a.src, width, height,
                               src_pitch, hist);
            hipLaunchKernelGGL(otsu_scan_kernel, dim3(1), dim3(64), 0, s, hist, width * height, otsu_dev);
            a.dev_thresh = otsu_dev;
        }
    }
    if (e == hipSuccess) {
        if (pix == TBDK_PIX_F32)
            hipLaunchKernelGGL(thresh_f32_kernel, dim3((wb + kThreads - 1) / kThreads, height), dim3(kThreads), 0, s, a);
        else
            hipLaunchKernelGGL(thresh_u8_kernel, dim3((wb + 4 * kThreads - 1) / (4 * kThreads), height), dim3(kThreads),
                               0, s, a);
        e = hipGetLastError();
    }
    timing_end(ctx, rec, s);
    if (e == hipSuccess && thresh_used) *thresh_used = used;
    return map_status(e);
}

}  // extern "C"
