// mog2.hip — cv::BackgroundSubtractorMOG2 with a device-resident model (tbdk_mog2_*,
// include/tbdk.h; DESIGN.md §5 "MOG2").  The arithmetic is mog2_core.hpp's; this
// file is the model's layout in HBM, the three kernels and the host schedule.
//
// Layout: mode-major planes over a pixel grid whose rows are padded to a multiple
// of four pixels (wp), so a lane's kPx consecutive pixels never straddle a row and
// element kPx * g of every plane belongs to lane g:
//   weight[K][ps], variance[K][ps], mean[K][CN][ps] (float), modes_used[ps] (uint8)
// ps = wp * height rounded up to 64.  The mean's channels are planes of their own:
// three channels cost 12 bytes a mode, not the 16 of a padded float4.  Every model
// access is one load or store of kPx floats per lane (kPx bytes for modes_used).
// kPx is 2: with 4 (16-byte accesses) a lane holds twice the registers and runs
// twice the pixels one after the other, and the kernel measured 22 to 29 % slower;
// it is bound by the latency of the per-pixel code, not by bytes.
//
// A lane loads mode k's planes only if one of its pixels uses mode k, so a wave
// whose pixels all hold one or two modes moves one or two modes' planes; a plane is
// stored only by the lanes in which one of its words changed.  The slot a new mode
// goes to (index = the lane's largest count) was not loaded: it is fetched then, so
// that the neighbour's stale words in it survive as they do in the reference.
#include <cstring>
#include <new>

#include "mog2_core.hpp"
#include "tbdk_internal.hpp"

namespace tbdk {
namespace {

using mog2_core::FrameParams;

constexpr int kMog2Threads = 256;
constexpr int kPx = 2;  // consecutive pixels of a row per lane: 2 or 4 (wp is a multiple of 4)

struct Mog2Planes {
    float* weight;
    float* variance;
    float* mean;
    uint8_t* modes;
    int64_t ps;  // plane stride, elements
    int width, height, wp, gpr;  // gpr: groups of kPx pixels per row
    int ngroups;
};

struct Mog2ApplyArgs {
    Mog2Planes m;
    const uint8_t* frame;
    int pitch, f32;
    uint8_t* mask;
    int mask_pitch;
    FrameParams p;
};

// kPx consecutive floats of a plane (kPx * 4 bytes, aligned)
__device__ __forceinline__ void ld4(const float* p, float* d)
{
    if (kPx == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        d[0] = t.x, d[1] = t.y, d[kPx - 2] = t.z, d[kPx - 1] = t.w;
    } else {
        const float2 t = *reinterpret_cast<const float2*>(p);
        d[0] = t.x, d[1] = t.y;
    }
}
__device__ __forceinline__ void st4(float* p, const float* s)
{
    if (kPx == 4)
        *reinterpret_cast<float4*>(p) = make_float4(s[0], s[1], s[kPx - 2], s[kPx - 1]);
    else
        *reinterpret_cast<float2*>(p) = make_float2(s[0], s[1]);
}
// a lane's kPx mode counts
__device__ __forceinline__ void ld_modes(const uint8_t* p, int* nm)
{
    if (kPx == 4) {
        const uchar4 t = *reinterpret_cast<const uchar4*>(p);
        nm[0] = t.x, nm[1] = t.y, nm[kPx - 2] = t.z, nm[kPx - 1] = t.w;
    } else {
        const uchar2 t = *reinterpret_cast<const uchar2*>(p);
        nm[0] = t.x, nm[1] = t.y;
    }
}
__device__ __forceinline__ void st_bytes(uint8_t* p, const int* v)
{
    if (kPx == 4)
        *reinterpret_cast<uchar4*>(p) = make_uchar4((uint8_t)v[0], (uint8_t)v[1], (uint8_t)v[kPx - 2], (uint8_t)v[kPx - 1]);
    else
        *reinterpret_cast<uchar2*>(p) = make_uchar2((uint8_t)v[0], (uint8_t)v[1]);
}
__device__ __forceinline__ int max_of(const int* v)
{
    int m = v[0];
#pragma unroll
    for (int j = 1; j < kPx; ++j) m = max(m, v[j]);
    return m;
}
__device__ __forceinline__ bool differs(float a, float b) { return __float_as_uint(a) != __float_as_uint(b); }

template <int CN, int K>
__global__ __launch_bounds__(kMog2Threads) void mog2_apply_kernel(Mog2ApplyArgs a)
{
    const int g = blockIdx.x * kMog2Threads + threadIdx.x;
    if (g >= a.m.ngroups) return;
    const int y = g / a.m.gpr, x0 = (g - y * a.m.gpr) * kPx;
    const int64_t e = (int64_t)g * kPx, ps = a.m.ps;
    const int npx = min(kPx, a.m.width - x0);

    int nm[kPx];
    ld_modes(a.m.modes + e, nm);
    const int mx = max_of(nm);

    float Wv[K][kPx], Vv[K][kPx], Mv[K * CN][kPx];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k < mx) {
            ld4(a.m.weight + k * ps + e, Wv[k]);
            ld4(a.m.variance + k * ps + e, Vv[k]);
#pragma unroll
            for (int c = 0; c < CN; ++c) ld4(a.m.mean + (k * CN + c) * ps + e, Mv[k * CN + c]);
        } else {
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                Wv[k][j] = 0.f;
                Vv[k][j] = 0.f;
#pragma unroll
                for (int c = 0; c < CN; ++c) Mv[k * CN + c][j] = 0.f;
            }
        }
    }

    // the lane's samples
    float D[kPx][CN];
    const uint8_t* row = a.frame + (int64_t)y * a.pitch;
    if (a.f32) {
        const float* r = reinterpret_cast<const float*>(row) + (int64_t)x0 * CN;
#pragma unroll
        for (int j = 0; j < kPx; ++j)
#pragma unroll
            for (int c = 0; c < CN; ++c) D[j][c] = j < npx ? r[j * CN + c] : 0.f;
    } else {
        const uint8_t* r = row + (int64_t)x0 * CN;
#pragma unroll
        for (int j = 0; j < kPx; ++j)
#pragma unroll
            for (int c = 0; c < CN; ++c) D[j][c] = j < npx ? (float)r[j * CN + c] : 0.f;
    }

    unsigned cw = 0, cv = 0, cm = 0;  // planes with a changed word: bit k, bit k, bit k * CN + c
    int nm2[kPx];
    int out[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        nm2[j] = nm[j];
        out[j] = 0;
        if (j < npx) {
            float w[K], v[K], m[K * CN];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                w[k] = Wv[k][j];
                v[k] = Vv[k][j];
#pragma unroll
                for (int c = 0; c < CN; ++c) m[k * CN + c] = Mv[k * CN + c][j];
            }
            int n = nm[j];
            out[j] = mog2_core::update_pixel<CN, K>(w, v, m, &n, D[j], a.p, nullptr);
            nm2[j] = n;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                cw |= (unsigned)differs(w[k], Wv[k][j]) << k;
                cv |= (unsigned)differs(v[k], Vv[k][j]) << k;
                Wv[k][j] = w[k];
                Vv[k][j] = v[k];
#pragma unroll
                for (int c = 0; c < CN; ++c) {
                    cm |= (unsigned)differs(m[k * CN + c], Mv[k * CN + c][j]) << (k * CN + c);
                    Mv[k * CN + c][j] = m[k * CN + c];
                }
            }
        }
    }

    // a mode added at slot mx, which was not loaded: the pixels that did not add one keep the slot's words
    const int mx2 = max_of(nm2);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k == mx && mx2 > mx) {
            float o[kPx];
            ld4(a.m.weight + k * ps + e, o);
#pragma unroll
            for (int j = 0; j < kPx; ++j)
                if (!(nm2[j] > mx)) Wv[k][j] = o[j];
            ld4(a.m.variance + k * ps + e, o);
#pragma unroll
            for (int j = 0; j < kPx; ++j)
                if (!(nm2[j] > mx)) Vv[k][j] = o[j];
#pragma unroll
            for (int c = 0; c < CN; ++c) {
                ld4(a.m.mean + (k * CN + c) * ps + e, o);
#pragma unroll
                for (int j = 0; j < kPx; ++j)
                    if (!(nm2[j] > mx)) Mv[k * CN + c][j] = o[j];
                cm |= 1u << (k * CN + c);
            }
            cw |= 1u << k;
            cv |= 1u << k;
        }
    }

#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (cw >> k & 1) st4(a.m.weight + k * ps + e, Wv[k]);
        if (cv >> k & 1) st4(a.m.variance + k * ps + e, Vv[k]);
#pragma unroll
        for (int c = 0; c < CN; ++c)
            if (cm >> (k * CN + c) & 1) st4(a.m.mean + (k * CN + c) * ps + e, Mv[k * CN + c]);
    }
    bool counts_changed = false;
#pragma unroll
    for (int j = 0; j < kPx; ++j) counts_changed = counts_changed || nm2[j] != nm[j];
    if (counts_changed) st_bytes(a.m.modes + e, nm2);

    uint8_t* mrow = a.mask + (int64_t)y * a.mask_pitch + x0;
    if (npx == kPx && (reinterpret_cast<uintptr_t>(mrow) & (kPx - 1)) == 0) {
        st_bytes(mrow, out);
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (j < npx) mrow[j] = (uint8_t)out[j];
    }
}

struct Mog2BgArgs {
    Mog2Planes m;
    uint8_t* img;
    int pitch, f32, nmixtures;
    float TB;
};

// getBackgroundImage: the modes are streamed, a lane reads mode k while one of its pixels is still summing
template <int CN>
__global__ __launch_bounds__(kMog2Threads) void mog2_background_kernel(Mog2BgArgs a)
{
    const int g = blockIdx.x * kMog2Threads + threadIdx.x;
    if (g >= a.m.ngroups) return;
    const int y = g / a.m.gpr, x0 = (g - y * a.m.gpr) * kPx;
    const int64_t e = (int64_t)g * kPx, ps = a.m.ps;
    const int npx = min(kPx, a.m.width - x0);
    int nm[kPx];
    ld_modes(a.m.modes + e, nm);
    mog2_core::BgAcc<CN> acc[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) mog2_core::bg_start<CN>(acc[j]);
    for (int k = 0; k < a.nmixtures; ++k) {
        bool need = false;
#pragma unroll
        for (int j = 0; j < kPx; ++j) need = need || (acc[j].open && k < nm[j]);
        if (!need) break;
        float w[kPx], m[CN][kPx];
        ld4(a.m.weight + k * ps + e, w);
#pragma unroll
        for (int c = 0; c < CN; ++c) ld4(a.m.mean + (k * CN + c) * ps + e, m[c]);
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            if (acc[j].open && k < nm[j]) {
                float mj[CN];
#pragma unroll
                for (int c = 0; c < CN; ++c) mj[c] = m[c][j];
                mog2_core::bg_add<CN>(acc[j], w[j], mj, a.TB);
            }
        }
    }
    uint8_t* row = a.img + (int64_t)y * a.pitch;
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        if (j < npx) {
            float o[CN];
            mog2_core::bg_value<CN>(acc[j], o);
#pragma unroll
            for (int c = 0; c < CN; ++c) {
                if (a.f32)
                    reinterpret_cast<float*>(row)[(int64_t)(x0 + j) * CN + c] = o[c];
                else
                    row[(int64_t)(x0 + j) * CN + c] = mog2_core::saturate_u8(o[c]);
            }
        }
    }
}

struct Mog2ModelArgs {
    Mog2Planes m;
    int cn, nmixtures;
    float* weight;
    float* variance;
    float* mean;
    uint8_t* modes;
};

// the model in the reference's layout; one thread per pixel (tests and checkpoints, not a hot path)
__global__ __launch_bounds__(kMog2Threads) void mog2_model_kernel(Mog2ModelArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * kMog2Threads + threadIdx.x;
    if (p >= (int64_t)a.m.width * a.m.height) return;
    const int y = (int)(p / a.m.width), x = (int)(p - (int64_t)y * a.m.width);
    const int64_t e = (int64_t)y * a.m.wp + x, ps = a.m.ps;
    const int K = a.nmixtures, cn = a.cn;
    for (int k = 0; k < K; ++k) {
        if (a.weight) a.weight[p * K + k] = a.m.weight[k * ps + e];
        if (a.variance) a.variance[p * K + k] = a.m.variance[k * ps + e];
        if (a.mean)
            for (int c = 0; c < cn; ++c) a.mean[(p * K + k) * cn + c] = a.m.mean[(k * cn + c) * ps + e];
    }
    if (a.modes) a.modes[p] = a.m.modes[e];
}

template <int CN, int K>
void launch_apply_k(const Mog2ApplyArgs& a, int blocks, hipStream_t s)
{
    hipLaunchKernelGGL((mog2_apply_kernel<CN, K>), dim3(blocks), dim3(kMog2Threads), 0, s, a);
}

template <int CN>
bool launch_apply_cn(const Mog2ApplyArgs& a, int blocks, hipStream_t s)
{
    switch (a.p.nmixtures) {
    case 1: launch_apply_k<CN, 1>(a, blocks, s); return true;
    case 2: launch_apply_k<CN, 2>(a, blocks, s); return true;
    case 3: launch_apply_k<CN, 3>(a, blocks, s); return true;
    case 4: launch_apply_k<CN, 4>(a, blocks, s); return true;
    case 5: launch_apply_k<CN, 5>(a, blocks, s); return true;
    case 6: launch_apply_k<CN, 6>(a, blocks, s); return true;
    case 7: launch_apply_k<CN, 7>(a, blocks, s); return true;
    case 8: launch_apply_k<CN, 8>(a, blocks, s); return true;
    }
    return false;
}

}  // namespace
}  // namespace tbdk

using namespace tbdk;

struct tbdk_mog2 {
    tbdk_ctx* ctx = nullptr;
    tbdk_mog2_config cfg{};
    void* mem = nullptr;
    size_t mem_bytes = 0;
    Mog2Planes pl{};
    int nframes = 0;
    hipStream_t last_stream = nullptr;
};

namespace {

bool mog2_params_ok(const tbdk_mog2_config& c)
{
    return c.history >= 1 && c.shadow_value >= 0 && c.shadow_value <= 255 && c.var_threshold == c.var_threshold;
}

mog2_core::Settings mog2_settings(const tbdk_mog2_config& c)
{
    mog2_core::Settings s;
    s.history = c.history;
    s.nmixtures = c.nmixtures;
    s.detect_shadows = c.detect_shadows != 0;
    s.shadow_value = c.shadow_value;
    s.var_threshold = c.var_threshold;
    s.var_threshold_gen = c.var_threshold_gen;
    s.var_init = c.var_init;
    s.var_min = c.var_min;
    s.var_max = c.var_max;
    s.background_ratio = c.background_ratio;
    s.complexity_reduction = c.complexity_reduction;
    s.shadow_threshold = c.shadow_threshold;
    return s;
}

// a frame or image of the object's type at (ptr, pitch)
bool mog2_image_ok(const tbdk_mog2* m, const void* ptr, int pitch)
{
    if (!ptr) return false;
    const bool f32 = m->cfg.depth == TBDK_DEPTH_32F;
    const int64_t row = (int64_t)m->cfg.width * m->cfg.channels * (f32 ? 4 : 1);
    if (pitch < row) return false;
    if (f32 && ((reinterpret_cast<uintptr_t>(ptr) & 3) != 0 || (pitch & 3) != 0)) return false;
    return true;
}

}  // namespace

extern "C" {

int tbdk_mog2_config_default(int width, int height, int depth, int channels, tbdk_mog2_config* cfg)
{
    if (!cfg) return TBDK_EINVAL;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->width = width;
    cfg->height = height;
    cfg->depth = depth;
    cfg->channels = channels;
    cfg->history = 500;  // bgfg_gaussmix2.cpp:106-118
    cfg->nmixtures = 5;
    cfg->detect_shadows = 1;
    cfg->shadow_value = 127;
    cfg->var_threshold = 16.0;
    cfg->var_threshold_gen = 9.0f;
    cfg->var_init = 15.0f;
    cfg->var_min = 4.0f;
    cfg->var_max = 75.0f;
    cfg->background_ratio = 0.9f;
    cfg->complexity_reduction = 0.05f;
    cfg->shadow_threshold = 0.5f;
    return TBDK_OK;
}

int tbdk_mog2_create(tbdk_ctx* ctx, const tbdk_mog2_config* cfg, tbdk_mog2** out)
{
    if (!ctx || !cfg || !out) return TBDK_EINVAL;
    *out = nullptr;
    const tbdk_mog2_config& c = *cfg;
    if (c.width <= 0 || c.height <= 0 || c.width > 65535 || c.height > 65535) return TBDK_EINVAL;
    if (c.depth != TBDK_DEPTH_8U && c.depth != TBDK_DEPTH_32F) return TBDK_EINVAL;
    if (c.channels != 1 && c.channels != 3) return TBDK_EINVAL;
    if (c.nmixtures < 1 || c.nmixtures > mog2_core::kMaxMixtures || !mog2_params_ok(c)) return TBDK_EINVAL;
    const int wp = align_up(c.width, 4);
    const int64_t groups = (int64_t)(wp / kPx) * c.height;
    if (groups > (int64_t)1 << 29) return TBDK_EINVAL;  // group and block indices stay in int
    tbdk_mog2* m = new (std::nothrow) tbdk_mog2;
    if (!m) return TBDK_ENOMEM;
    m->ctx = ctx;
    m->cfg = c;
    Mog2Planes& p = m->pl;
    p.width = c.width;
    p.height = c.height;
    p.wp = wp;
    p.gpr = wp / kPx;
    p.ngroups = (int)groups;
    p.ps = (groups * kPx + 63) / 64 * 64;
    const size_t K = (size_t)c.nmixtures, cn = (size_t)c.channels, ps = (size_t)p.ps;
    m->mem_bytes = K * ps * 4 * (2 + cn) + ps;
    DeviceGuard g(ctx->device);
    const int rc = map_status(dev_alloc(&m->mem, m->mem_bytes, ctx->opt_alloc_fill));
    if (rc != TBDK_OK) {
        delete m;
        return rc;
    }
    p.weight = static_cast<float*>(m->mem);
    p.variance = p.weight + K * ps;
    p.mean = p.variance + K * ps;
    p.modes = reinterpret_cast<uint8_t*>(p.mean + K * cn * ps);
    *out = m;
    return TBDK_OK;
}

int tbdk_mog2_destroy(tbdk_mog2* m)
{
    if (!m) return TBDK_EINVAL;
    DeviceGuard g(m->ctx->device);
    (void)hipStreamSynchronize(m->last_stream);
    if (m->mem) (void)hipFree(m->mem);
    delete m;
    return TBDK_OK;
}

int tbdk_mog2_reset(tbdk_mog2* m)
{
    if (!m) return TBDK_EINVAL;
    m->nframes = 0;
    return TBDK_OK;
}

int tbdk_mog2_set_params(tbdk_mog2* m, const tbdk_mog2_config* cfg)
{
    if (!m || !cfg) return TBDK_EINVAL;
    const tbdk_mog2_config& c = *cfg;
    if (c.width != m->cfg.width || c.height != m->cfg.height || c.depth != m->cfg.depth ||
        c.channels != m->cfg.channels || c.nmixtures != m->cfg.nmixtures || !mog2_params_ok(c))
        return TBDK_EINVAL;
    m->cfg = c;
    return TBDK_OK;
}

int tbdk_mog2_apply(tbdk_mog2* m, const void* frame, int pitch, uint8_t* fgmask, int mask_pitch, double learning_rate,
                    void* stream)
{
    if (!m || !fgmask || mask_pitch < m->cfg.width || !(learning_rate == learning_rate)) return TBDK_EINVAL;
    if (!mog2_image_ok(m, frame, pitch)) return TBDK_EINVAL;
    tbdk_ctx* ctx = m->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int nframes = m->nframes;
    bool reinit = false;
    const double rate = mog2_core::schedule(&nframes, m->cfg.history, learning_rate, &reinit);
    Mog2ApplyArgs a;
    a.m = m->pl;
    a.frame = static_cast<const uint8_t*>(frame);
    a.pitch = pitch;
    a.f32 = m->cfg.depth == TBDK_DEPTH_32F;
    a.mask = fgmask;
    a.mask_pitch = mask_pitch;
    a.p = mog2_core::frame_params(mog2_settings(m->cfg), rate);
    const int blocks = (m->pl.ngroups + kMog2Threads - 1) / kMog2Threads;
    const int rec = timing_begin(ctx, "mog2_apply", s);
    hipError_t e = reinit ? hipMemsetAsync(m->mem, 0, m->mem_bytes, s) : hipSuccess;
    if (e == hipSuccess) {
        const bool ok = m->cfg.channels == 1 ? launch_apply_cn<1>(a, blocks, s) : launch_apply_cn<3>(a, blocks, s);
        e = ok ? hipGetLastError() : hipErrorInvalidValue;
    }
    timing_end(ctx, rec, s);
    if (e != hipSuccess) return map_status(e);
    m->nframes = nframes;
    m->last_stream = s;
    return TBDK_OK;
}

int tbdk_mog2_get_background(tbdk_mog2* m, void* img, int pitch, void* stream)
{
    if (!m || !mog2_image_ok(m, img, pitch)) return TBDK_EINVAL;
    tbdk_ctx* ctx = m->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Mog2BgArgs a;
    a.m = m->pl;
    a.img = static_cast<uint8_t*>(img);
    a.pitch = pitch;
    a.f32 = m->cfg.depth == TBDK_DEPTH_32F;
    a.nmixtures = m->cfg.nmixtures;
    a.TB = m->cfg.background_ratio;
    const int blocks = (m->pl.ngroups + kMog2Threads - 1) / kMog2Threads;
    const int rec = timing_begin(ctx, "mog2_background", s);
    // before the first apply the model is whatever the allocation held: every pixel counts as empty
    hipError_t e = m->nframes == 0 ? hipMemsetAsync(m->pl.modes, 0, (size_t)m->pl.ps, s) : hipSuccess;
    if (e == hipSuccess) {
        if (m->cfg.channels == 1)
            hipLaunchKernelGGL(mog2_background_kernel<1>, dim3(blocks), dim3(kMog2Threads), 0, s, a);
        else
            hipLaunchKernelGGL(mog2_background_kernel<3>, dim3(blocks), dim3(kMog2Threads), 0, s, a);
        e = hipGetLastError();
    }
    timing_end(ctx, rec, s);
    if (e == hipSuccess) m->last_stream = s;
    return map_status(e);
}

int tbdk_mog2_get_model(tbdk_mog2* m, float* weight, float* variance, float* mean, uint8_t* modes_used, void* stream)
{
    if (!m) return TBDK_EINVAL;
    tbdk_ctx* ctx = m->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Mog2ModelArgs a;
    a.m = m->pl;
    a.cn = m->cfg.channels;
    a.nmixtures = m->cfg.nmixtures;
    a.weight = weight;
    a.variance = variance;
    a.mean = mean;
    a.modes = modes_used;
    const int64_t px = (int64_t)m->cfg.width * m->cfg.height;
    const int blocks = (int)((px + kMog2Threads - 1) / kMog2Threads);
    const int rec = timing_begin(ctx, "mog2_model", s);
    // before the first apply the allocation is cleared, as the first apply would
    hipError_t e = m->nframes == 0 ? hipMemsetAsync(m->mem, 0, m->mem_bytes, s) : hipSuccess;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mog2_model_kernel, dim3(blocks), dim3(kMog2Threads), 0, s, a);
        e = hipGetLastError();
    }
    timing_end(ctx, rec, s);
    if (e == hipSuccess) m->last_stream = s;
    return map_status(e);
}

int tbdk_mog2_frames(tbdk_mog2* m, int* nframes)
{
    if (!m || !nframes) return TBDK_EINVAL;
    *nframes = m->nframes;
    return TBDK_OK;
}

}  // extern "C"
