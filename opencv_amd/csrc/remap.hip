// remap.hip — cv::remap, cv::warpPerspective and a warp by a dense flow on
// gfx950, for 8U and 32F images of 1 to 4 channels, bit-exact with the CPU
// implementation (imgproc/src/imgwarp.cpp: RemapInvoker :1105-1280,
// remapNearest :330-428, remapBilinear :649-856, remapBicubic :860-958,
// WarpPerspectiveInvoker :2706-2797; tests/_remap_oracle.py restates it).
//
// One sampling core, templated on pixel type, channel count and interpolation,
// behind three map front ends chosen by a wave-uniform switch: remap's map
// decoding, the projective map in double with the reference's block-origin
// arithmetic, and grid + sign * flow formed in registers (the 8 B/pixel map is
// never stored).  The border mode is a kernel argument, as in warp.hip.  The
// address computation lives in remap_core.hpp, shared with the host bounds walk;
// the bicubic weights come from warp_device.hpp, shared with warp.hip.
//
// One thread per 4 destination pixels of a row: map and flow reads are
// contiguous per thread and coalesced across the wave, source taps are L1/L2
// gathers, 8-bit results leave as whole 32-bit words where the group is
// complete, aligned and nothing in it is kept.  No LDS, no scratch.
#include "tbdk_internal.hpp"

#include "remap_core.hpp"
#include "warp_device.hpp"

namespace tbdk {

namespace {

namespace rc = remap_core;
using warp_device::bicubic_tab;

static_assert(rc::kNearest == TBDK_INTER_NEAREST && rc::kLinear == TBDK_INTER_LINEAR && rc::kCubic == TBDK_INTER_CUBIC,
              "interpolation values");
static_assert(rc::kConstant == TBDK_BORDER_CONSTANT && rc::kReplicate == TBDK_BORDER_REPLICATE &&
                  rc::kReflect == TBDK_BORDER_REFLECT && rc::kWrap == TBDK_BORDER_WRAP &&
                  rc::kReflect101 == TBDK_BORDER_REFLECT_101 && rc::kTransparent == TBDK_BORDER_TRANSPARENT,
              "border values");

enum { kFrontMap32FC2 = TBDK_MAP_32FC2, kFrontMap32FC1 = TBDK_MAP_32FC1, kFrontMap16SC2 = TBDK_MAP_16SC2, kFrontFlow,
       kFrontPerspective };

struct RemapArgs {
    const uint8_t* src;
    int sw, sh, spitch;  // pitches in bytes
    uint8_t* dst;
    int dw, dh, dpitch;
    const uint8_t* map1;  // CV_32FC2 / CV_32FC1 x / CV_16SC2 / the flow
    const uint8_t* map2;  // CV_32FC1 y / CV_16UC1 fractions / null
    int pitch1, pitch2;
    int front, border;
    float sign;
    int bw0;       // warpPerspective's block width
    double m[9];   // dst -> src
    int cvi[4];    // saturate_cast<uchar>(borderValue[k])
    float cvf[4];  // saturate_cast<float>(borderValue[k])
};

template <typename T>
__device__ __forceinline__ T border_value(const RemapArgs& a, int k);
template <>
__device__ __forceinline__ uint8_t border_value<uint8_t>(const RemapArgs& a, int k)
{
    return (uint8_t)a.cvi[k];
}
template <>
__device__ __forceinline__ float border_value<float>(const RemapArgs& a, int k)
{
    return a.cvf[k];
}

__device__ __forceinline__ rc::Coord decode(const RemapArgs& a, int x, int y, bool nearest)
{
    switch (a.front) {
    case kFrontMap32FC2: {
        const float* p = reinterpret_cast<const float*>(a.map1 + (size_t)y * a.pitch1) + 2 * x;
        return rc::decode_float(p[0], p[1], nearest);
    }
    case kFrontMap32FC1:
        return rc::decode_float(reinterpret_cast<const float*>(a.map1 + (size_t)y * a.pitch1)[x],
                                reinterpret_cast<const float*>(a.map2 + (size_t)y * a.pitch2)[x], nearest);
    case kFrontMap16SC2: {
        const int16_t* p = reinterpret_cast<const int16_t*>(a.map1 + (size_t)y * a.pitch1) + 2 * x;
        const unsigned f = a.map2 ? reinterpret_cast<const uint16_t*>(a.map2 + (size_t)y * a.pitch2)[x] : 0u;
        return rc::decode_fixed(p[0], p[1], a.map2 != nullptr, f, nearest);
    }
    case kFrontFlow: {
        const float* p = reinterpret_cast<const float*>(a.map1 + (size_t)y * a.pitch1) + 2 * x;
        return rc::decode_flow(x, y, p[0], p[1], a.sign, nearest);
    }
    default:
        return rc::decode_perspective(a.m, a.bw0, a.dw, x, y, nearest);
    }
}

// a tap's CN values, or the border value where its row or column is -1
template <typename T, int CN>
__device__ __forceinline__ void load_tap(const RemapArgs& a, int y, int x, T* v)
{
#pragma unroll
    for (int k = 0; k < CN; ++k) v[k] = border_value<T>(a, k);
    if (y >= 0 && x >= 0) {
        const T* S = reinterpret_cast<const T*>(a.src + (size_t)y * a.spitch) + x * CN;
#pragma unroll
        for (int k = 0; k < CN; ++k) v[k] = S[k];
    }
}

// one destination pixel: CN values into out[], or keep
template <typename T, int CN, int INTER>
__device__ __forceinline__ bool sample_pixel(const RemapArgs& a, const rc::Coord& c, T* out)
{
    constexpr int N = rc::TapCount<INTER>::value;
    constexpr bool is8 = sizeof(T) == 1;
    int xs[N], ys[N];
    const int what = rc::make_taps<INTER>(c.sx, c.sy, a.sw, a.sh, a.border, xs, ys);
    if (what == rc::kKeep) return false;
    if (what == rc::kFill) {
#pragma unroll
        for (int k = 0; k < CN; ++k) out[k] = border_value<T>(a, k);
        return true;
    }
    if constexpr (INTER == rc::kNearest) {
        load_tap<T, CN>(a, ys[0], xs[0], out);
    } else if constexpr (INTER == rc::kLinear) {
        T v0[CN], v1[CN], v2[CN], v3[CN];
        load_tap<T, CN>(a, ys[0], xs[0], v0);
        load_tap<T, CN>(a, ys[0], xs[1], v1);
        load_tap<T, CN>(a, ys[1], xs[0], v2);
        load_tap<T, CN>(a, ys[1], xs[1], v3);
        if constexpr (is8) {  // BilinearTab_i: 15-bit weights, exact; FixedPtCast<int, uchar, 15>
            const int w0 = (32 - c.ay) * (32 - c.ax) * 32, w1 = (32 - c.ay) * c.ax * 32;
            const int w2 = c.ay * (32 - c.ax) * 32, w3 = c.ay * c.ax * 32;
#pragma unroll
            for (int k = 0; k < CN; ++k) {
                const int r = (v0[k] * w0 + v1[k] * w1 + v2[k] * w2 + v3[k] * w3 + (1 << 14)) >> 15;
                out[k] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
            }
        } else {  // BilinearTab_f: products of (1 - i/32, i/32), exact; the sum in the reference's order
            const float fx = c.ax * (1.f / 32), fy = c.ay * (1.f / 32);
            const float w0 = (1.f - fy) * (1.f - fx), w1 = (1.f - fy) * fx, w2 = fy * (1.f - fx), w3 = fy * fx;
#pragma unroll
            for (int k = 0; k < CN; ++k) out[k] = ((v0[k] * w0 + v1[k] * w1) + v2[k] * w2) + v3[k] * w3;
        }
    } else {  // bicubic, 8U: cval*ONE + sum (S - cval)*w, FixedPtCast<int, uchar, 15>
        static_assert(INTER != rc::kCubic || is8, "the 32F bicubic path is out of scope");
        int w[16], sum[CN];
        bicubic_tab(c.ay, c.ax, w);
#pragma unroll
        for (int k = 0; k < CN; ++k) sum[k] = a.cvi[k] * 32768;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (ys[r] < 0 || xs[q] < 0) continue;
                const uint8_t* S = a.src + (size_t)ys[r] * a.spitch + xs[q] * CN;
#pragma unroll
                for (int k = 0; k < CN; ++k) sum[k] += ((int)S[k] - a.cvi[k]) * w[4 * r + q];
            }
#pragma unroll
        for (int k = 0; k < CN; ++k) {
            const int r = (sum[k] + (1 << 14)) >> 15;
            out[k] = (T)(r < 0 ? 0 : (r > 255 ? 255 : r));
        }
    }
    return true;
}


constexpr int kGroup = 4;  // destination pixels per thread

template <typename T, int CN, int INTER>
__device__ __forceinline__ void remap_row_group(const RemapArgs& a)
{
    const int y = blockIdx.y;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * kGroup;
    if (x0 >= a.dw) return;
    T* D = reinterpret_cast<T*>(a.dst + (size_t)y * a.dpitch) + (size_t)x0 * CN;
    T out[kGroup * CN];
    unsigned store = 0;  // bit k: pixel k is written (inside the row and not left to BORDER_TRANSPARENT)
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
#pragma unroll
        for (int j = 0; j < CN; ++j) out[k * CN + j] = 0;
        if (x0 + k < a.dw &&
            sample_pixel<T, CN, INTER>(a, decode(a, x0 + k, y, INTER == rc::kNearest), out + k * CN))
            store |= 1u << k;
    }
    if constexpr (sizeof(T) == 1) {
        if (store == (1u << kGroup) - 1 && (reinterpret_cast<uintptr_t>(D) & 3) == 0) {
            uint32_t* D4 = reinterpret_cast<uint32_t*>(D);  // kGroup * CN bytes: CN whole words
#pragma unroll
            for (int j = 0; j < CN; ++j)
                D4[j] = (uint32_t)out[4 * j] | ((uint32_t)out[4 * j + 1] << 8) | ((uint32_t)out[4 * j + 2] << 16) |
                        ((uint32_t)out[4 * j + 3] << 24);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < kGroup; ++k)
        if (store >> k & 1) {
#pragma unroll
            for (int j = 0; j < CN; ++j) D[k * CN + j] = out[k * CN + j];
        }
}

template <typename T, int CN, int INTER>
__global__ __launch_bounds__(256) void remap_kernel(RemapArgs a)
{
    remap_row_group<T, CN, INTER>(a);
}

// warpPerspective with the matrix in device memory (tbdk_warp_perspective_dev):
// every thread reads the nine doubles, inverts them unless the caller's matrix
// already maps dst -> src (rc::invert_3x3, the host path's arithmetic) and runs
// the same sampling.  A zero *valid or a non-finite entry leaves dst untouched.
template <typename T, int CN, int INTER>
__global__ __launch_bounds__(256) void remap_persp_dev_kernel(RemapArgs a, const double* __restrict__ M,
                                                              const int32_t* __restrict__ valid, int inverse_map)
{
    if (valid && *valid == 0) return;
    double m[9];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        m[i] = M[i];
        finite = finite && isfinite(m[i]);
    }
    if (!finite) return;
    if (inverse_map) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.m[i] = m[i];
    } else {
        rc::invert_3x3(m, a.m);
    }
    remap_row_group<T, CN, INTER>(a);
}

template <typename T, int CN>
hipError_t launch_dev_cn(const RemapArgs& a, int inter, const double* M, const int32_t* valid, int inv, hipStream_t s)
{
    const dim3 grid((a.dw + kGroup * 256 - 1) / (kGroup * 256), a.dh), block(256);
    if (inter == rc::kNearest)
        hipLaunchKernelGGL((remap_persp_dev_kernel<T, CN, rc::kNearest>), grid, block, 0, s, a, M, valid, inv);
    else if (inter == rc::kLinear)
        hipLaunchKernelGGL((remap_persp_dev_kernel<T, CN, rc::kLinear>), grid, block, 0, s, a, M, valid, inv);
    else if constexpr (sizeof(T) == 1)
        hipLaunchKernelGGL((remap_persp_dev_kernel<T, CN, rc::kCubic>), grid, block, 0, s, a, M, valid, inv);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename T>
hipError_t launch_dev_t(const RemapArgs& a, int cn, int inter, const double* M, const int32_t* valid, int inv,
                        hipStream_t s)
{
    switch (cn) {
    case 1: return launch_dev_cn<T, 1>(a, inter, M, valid, inv, s);
    case 2: return launch_dev_cn<T, 2>(a, inter, M, valid, inv, s);
    case 3: return launch_dev_cn<T, 3>(a, inter, M, valid, inv, s);
    default: return launch_dev_cn<T, 4>(a, inter, M, valid, inv, s);
    }
}

template <typename T, int CN>
hipError_t launch_cn(const RemapArgs& a, int inter, hipStream_t s)
{
    const dim3 grid((a.dw + kGroup * 256 - 1) / (kGroup * 256), a.dh), block(256);
    if (inter == rc::kNearest) hipLaunchKernelGGL((remap_kernel<T, CN, rc::kNearest>), grid, block, 0, s, a);
    else if (inter == rc::kLinear) hipLaunchKernelGGL((remap_kernel<T, CN, rc::kLinear>), grid, block, 0, s, a);
    else if constexpr (sizeof(T) == 1) hipLaunchKernelGGL((remap_kernel<T, CN, rc::kCubic>), grid, block, 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename T>
hipError_t launch_t(const RemapArgs& a, int cn, int inter, hipStream_t s)
{
    switch (cn) {
    case 1: return launch_cn<T, 1>(a, inter, s);
    case 2: return launch_cn<T, 2>(a, inter, s);
    case 3: return launch_cn<T, 3>(a, inter, s);
    default: return launch_cn<T, 4>(a, inter, s);
    }
}

bool overlaps(const void* p, int64_t pn, const void* q, int64_t qn)
{
    const char *a = static_cast<const char*>(p), *b = static_cast<const char*>(q);
    return a < b + qn && b < a + pn;
}

int64_t extent(int rows, int pitch, int row_bytes) { return (int64_t)(rows - 1) * pitch + row_bytes; }

struct Image {
    const void* src;
    int pix, cn, sw, sh, spitch;
    void* dst;
    int dw, dh, dpitch;
};

// the checks the three entry points share; fills the image part of the arguments.
// Returns TBDK_OK, TBDK_EINVAL, or 1 for an empty destination (a no-op)
int prepare(const tbdk_ctx* ctx, const Image& im, int* inter, int border, const double* border_value, RemapArgs* a)
{
    if (!ctx || !border_value) return TBDK_EINVAL;
    if (im.pix != TBDK_PIX_U8 && im.pix != TBDK_PIX_F32) return TBDK_EINVAL;
    if (im.cn < 1 || im.cn > 4) return TBDK_EINVAL;
    if (*inter == TBDK_INTER_AREA) *inter = TBDK_INTER_LINEAR;  // as cv::remap does (imgwarp.cpp:1729-1730)
    if (*inter != TBDK_INTER_NEAREST && *inter != TBDK_INTER_LINEAR && *inter != TBDK_INTER_CUBIC) return TBDK_EINVAL;
    if (*inter == TBDK_INTER_CUBIC && im.pix != TBDK_PIX_U8) return TBDK_EINVAL;
    if (border < TBDK_BORDER_CONSTANT || border > TBDK_BORDER_TRANSPARENT) return TBDK_EINVAL;
    if (im.dw < 0 || im.dh < 0) return TBDK_EINVAL;
    // the reference: dst.cols < SHRT_MAX && dst.rows < SHRT_MAX && src.cols < SHRT_MAX && src.rows < SHRT_MAX
    if (im.sw <= 0 || im.sh <= 0 || im.sw >= 32767 || im.sh >= 32767 || im.dw >= 32767 || im.dh >= 32767)
        return TBDK_EINVAL;
    if (im.dw == 0 || im.dh == 0) return 1;
    if (!im.src || !im.dst) return TBDK_EINVAL;
    const int esz = im.pix == TBDK_PIX_U8 ? 1 : 4, px = esz * im.cn;
    if (im.spitch < (int64_t)im.sw * px || im.dpitch < (int64_t)im.dw * px) return TBDK_EINVAL;
    if (esz == 4 && ((reinterpret_cast<uintptr_t>(im.src) | reinterpret_cast<uintptr_t>(im.dst) | (unsigned)im.spitch |
                      (unsigned)im.dpitch) & 3))
        return TBDK_EINVAL;
    // dst == src: the reference clones src (imgwarp.cpp:1726-1727); here aliasing is an error
    if (overlaps(im.src, extent(im.sh, im.spitch, im.sw * px), im.dst, extent(im.dh, im.dpitch, im.dw * px)))
        return TBDK_EINVAL;
    a->src = static_cast<const uint8_t*>(im.src);
    a->sw = im.sw, a->sh = im.sh, a->spitch = im.spitch;
    a->dst = static_cast<uint8_t*>(im.dst);
    a->dw = im.dw, a->dh = im.dh, a->dpitch = im.dpitch;
    a->map1 = a->map2 = nullptr;
    a->pitch1 = a->pitch2 = 0;
    a->border = border;
    a->sign = 1.f;
    a->bw0 = 1;
    for (int i = 0; i < 9; ++i) a->m[i] = 0;
    for (int k = 0; k < 4; ++k) {
        const double v = border_value[k];
        // saturate_cast<uchar>(double): cvRound, then the clamp (a NaN rounds to INT_MIN)
        a->cvi[k] = !(v == v) || v <= 0 ? 0 : (v >= 255 ? 255 : (int)rint(v));
        a->cvf[k] = (float)v;
    }
    return TBDK_OK;
}

int run(tbdk_ctx* ctx, const char* name, const Image& im, const RemapArgs& a, int inter, void* stream)
{
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rec = timing_begin(ctx, name, s);
    const hipError_t e = im.pix == TBDK_PIX_U8 ? launch_t<uint8_t>(a, im.cn, inter, s) : launch_t<float>(a, im.cn, inter, s);
    timing_end(ctx, rec, s);
    return e == hipSuccess ? TBDK_OK : (e == hipErrorOutOfMemory ? TBDK_ENOMEM : TBDK_EHIP);
}

}  // namespace

// cv::invert, 3x3 CV_64F: remap_core.hpp, shared with the device-matrix kernel
void invert_3x3(const double* m, double* out) { remap_core::invert_3x3(m, out); }

}  // namespace tbdk

using namespace tbdk;

extern "C" {

int tbdk_remap(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height, int src_pitch,
               void* dst, int dst_width, int dst_height, int dst_pitch, const void* map1, int map1_pitch,
               const void* map2, int map2_pitch, int map_kind, int interpolation, int border,
               const double* border_value, void* stream)
{
    const Image im{src, pix, cn, src_width, src_height, src_pitch, dst, dst_width, dst_height, dst_pitch};
    RemapArgs a;
    int inter = interpolation;
    if (map_kind != TBDK_MAP_32FC2 && map_kind != TBDK_MAP_32FC1 && map_kind != TBDK_MAP_16SC2) return TBDK_EINVAL;
    // CV_16SC2 alone is a NEAREST map; with an interpolating mode the reference reads the shorts as floats
    if (map_kind == TBDK_MAP_16SC2 && !map2 && interpolation != TBDK_INTER_NEAREST) return TBDK_EINVAL;
    const int st = prepare(ctx, im, &inter, border, border_value, &a);
    if (st != TBDK_OK) return st < 0 ? st : TBDK_OK;
    if (!map1) return TBDK_EINVAL;
    const int64_t dbytes = extent(dst_height, dst_pitch, dst_width * cn * (pix == TBDK_PIX_U8 ? 1 : 4));
    const int row1 = dst_width * (map_kind == TBDK_MAP_32FC2 ? 8 : 4);
    const int align1 = map_kind == TBDK_MAP_16SC2 ? 1 : 3;
    if (map1_pitch < row1 || ((reinterpret_cast<uintptr_t>(map1) | (unsigned)map1_pitch) & align1)) return TBDK_EINVAL;
    if (overlaps(map1, extent(dst_height, map1_pitch, row1), dst, dbytes)) return TBDK_EINVAL;
    if (map_kind == TBDK_MAP_32FC2) map2 = nullptr;
    if (map_kind == TBDK_MAP_32FC1 && !map2) return TBDK_EINVAL;
    if (map2) {
        const int row2 = dst_width * (map_kind == TBDK_MAP_32FC1 ? 4 : 2);
        const int align2 = map_kind == TBDK_MAP_32FC1 ? 3 : 1;
        if (map2_pitch < row2 || ((reinterpret_cast<uintptr_t>(map2) | (unsigned)map2_pitch) & align2))
            return TBDK_EINVAL;
        if (overlaps(map2, extent(dst_height, map2_pitch, row2), dst, dbytes)) return TBDK_EINVAL;
    }
    a.map1 = static_cast<const uint8_t*>(map1);
    a.map2 = static_cast<const uint8_t*>(map2);
    a.pitch1 = map1_pitch;
    a.pitch2 = map2 ? map2_pitch : 0;
    a.front = map_kind;
    return run(ctx, "remap", im, a, inter, stream);
}

int tbdk_remap_flow(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height, int src_pitch,
                    void* dst, int dst_width, int dst_height, int dst_pitch, const float* flow, int flow_pitch,
                    int sign, int interpolation, int border, const double* border_value, void* stream)
{
    const Image im{src, pix, cn, src_width, src_height, src_pitch, dst, dst_width, dst_height, dst_pitch};
    RemapArgs a;
    int inter = interpolation;
    if (sign != 1 && sign != -1) return TBDK_EINVAL;
    const int st = prepare(ctx, im, &inter, border, border_value, &a);
    if (st != TBDK_OK) return st < 0 ? st : TBDK_OK;
    if (!flow || flow_pitch < (int64_t)dst_width * 8 || ((reinterpret_cast<uintptr_t>(flow) | (unsigned)flow_pitch) & 3))
        return TBDK_EINVAL;
    if (overlaps(flow, extent(dst_height, flow_pitch, dst_width * 8), dst,
                 extent(dst_height, dst_pitch, dst_width * cn * (pix == TBDK_PIX_U8 ? 1 : 4))))
        return TBDK_EINVAL;
    a.map1 = reinterpret_cast<const uint8_t*>(flow);
    a.pitch1 = flow_pitch;
    a.sign = (float)sign;
    a.front = kFrontFlow;
    return run(ctx, "remap_flow", im, a, inter, stream);
}

int tbdk_warp_perspective(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height,
                          int src_pitch, void* dst, int dst_width, int dst_height, int dst_pitch, const double* M,
                          int flags, int border, const double* border_value, void* stream)
{
    const Image im{src, pix, cn, src_width, src_height, src_pitch, dst, dst_width, dst_height, dst_pitch};
    RemapArgs a;
    int inter = flags & 7;
    if (!M || (flags & ~(7 | TBDK_WARP_INVERSE_MAP))) return TBDK_EINVAL;
    // the reference's vector and scalar bodies disagree on NaN entries: finite matrices only
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(M[i])) return TBDK_EINVAL;
    const int st = prepare(ctx, im, &inter, border, border_value, &a);
    if (st != TBDK_OK) return st < 0 ? st : TBDK_OK;
    if (flags & TBDK_WARP_INVERSE_MAP) {
        for (int i = 0; i < 9; ++i) a.m[i] = M[i];
    } else {
        invert_3x3(M, a.m);
    }
    a.bw0 = rc::perspective_block_width(dst_width, dst_height);
    a.front = kFrontPerspective;
    return run(ctx, "warp_perspective", im, a, inter, stream);
}

int tbdk_warp_perspective_dev(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height,
                              int src_pitch, void* dst, int dst_width, int dst_height, int dst_pitch, const double* M,
                              const int32_t* valid, int flags, int border, const double* border_value, void* stream)
{
    const Image im{src, pix, cn, src_width, src_height, src_pitch, dst, dst_width, dst_height, dst_pitch};
    RemapArgs a;
    int inter = flags & 7;
    if (!M || (reinterpret_cast<uintptr_t>(M) & 7) || (reinterpret_cast<uintptr_t>(valid) & 3) ||
        (flags & ~(7 | TBDK_WARP_INVERSE_MAP)))
        return TBDK_EINVAL;
    const int st = prepare(ctx, im, &inter, border, border_value, &a);
    if (st != TBDK_OK) return st < 0 ? st : TBDK_OK;
    a.bw0 = rc::perspective_block_width(dst_width, dst_height);
    a.front = kFrontPerspective;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int inv = (flags & TBDK_WARP_INVERSE_MAP) ? 1 : 0;
    const int rec = timing_begin(ctx, "warp_perspective_dev", s);
    const hipError_t e = im.pix == TBDK_PIX_U8 ? launch_dev_t<uint8_t>(a, im.cn, inter, M, valid, inv, s)
                                               : launch_dev_t<float>(a, im.cn, inter, M, valid, inv, s);
    timing_end(ctx, rec, s);
    return e == hipSuccess ? TBDK_OK : (e == hipErrorOutOfMemory ? TBDK_ENOMEM : TBDK_EHIP);
}

int tbdk_warp_perspective_invert(const double* M, double* out)
{
    if (!M || !out) return TBDK_EINVAL;
    invert_3x3(M, out);
    return TBDK_OK;
}

}  // extern "C"
