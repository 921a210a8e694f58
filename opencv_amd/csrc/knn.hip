// knn.hip — cv::BackgroundSubtractorKNN (the CPU class) with a device-resident model (tbdk_knn_*,
// include/tbdk.h; DESIGN.md §5 "KNN").  The arithmetic is knn_core.hpp's; this file is the
// model's layout in HBM, the four kernels and the host schedule.
//
// Layout: sample-major planes over a pixel grid whose rows are padded to a multiple of four
// pixels (wp), so a lane's kPx consecutive pixels never straddle a row and element kPx * g of
// every plane belongs to lane g:
//   sample[3 * nN][ps]   one word a pixel: B, G, R, flag (a dword) or value, flag (two bytes)
//   index[3][ps], next[3][ps]   bytes: short, mid, long
// ps = wp * height rounded up to 64.  A wave's load of sample n is kPx words per lane, 1 KiB
// (BGR) or 512 B (gray) of consecutive memory.  The kernel is bound by these bytes, and the
// reference's early exit saves them: a lane stops loading planes when all its pixels have
// returned 1 or reached the end, a wave when all its lanes have, and the shadow pass reads
// planes only in lanes with a pixel that was not background.  Writes are a word per update.
//
// The RNG's state lives on the device, in two slots that the fills alternate between (a fill
// reads one and its last block writes the other, so no block can read what another wrote);
// the host knows which slot is current because it knows how many fills it has enqueued.  An
// object's first fill takes the configured state as a kernel argument, so creation copies
// nothing to the device and synchronises nothing.
#include <cstring>
#include <new>

#include "tbdk_internal.hpp"
// after the HIP runtime, whose 64-bit high multiply its device side uses
#include "knn_core.hpp"

namespace tbdk {
namespace {

using knn_core::FrameParams;

constexpr int kKnnThreads = 256;
constexpr int kPx = 4;           // consecutive pixels of a row per lane (wp is a multiple of 4)
constexpr int kRanduThreads = knn_core::kLanes;  // a wave per block of the fill

template <int CN>
struct WordOf {
    typedef uint32_t type;
};
template <>
struct WordOf<1> {
    typedef uint16_t type;
};

struct KnnPlanes {
    void* samples;
    uint8_t* index;   // 3 planes
    uint8_t* next;    // 3 planes
    int64_t ps;       // plane stride, elements
    int width, height, wp, gpr;  // gpr: groups of kPx pixels per row
    int ngroups;
};

struct KnnApplyArgs {
    KnnPlanes m;
    const uint8_t* frame;
    int pitch;
    uint8_t* mask;
    int mask_pitch;
    FrameParams p;
};

// a lane's kPx words of a sample plane (16 or 8 bytes, aligned)
template <int CN>
__device__ __forceinline__ void ld_words(const typename WordOf<CN>::type* p, uint32_t* d)
{
    if (CN == 3) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
    } else {
        const ushort4 t = *reinterpret_cast<const ushort4*>(p);
        d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
    }
}
// the four bytes of a lane's word of an index or next-update plane
__device__ __forceinline__ void unpack4(uint32_t w, int* d)
{
    d[0] = w & 255, d[1] = (w >> 8) & 255, d[2] = (w >> 16) & 255, d[3] = w >> 24;
}
__device__ __forceinline__ void st_bytes(uint8_t* p, const int* v)
{
    *reinterpret_cast<uchar4*>(p) = make_uchar4((uint8_t)v[0], (uint8_t)v[1], (uint8_t)v[2], (uint8_t)v[3]);
}

template <int CN>
__global__ __launch_bounds__(kKnnThreads) void knn_apply_kernel(KnnApplyArgs a)
{
    typedef typename WordOf<CN>::type Word;
    const int g = blockIdx.x * kKnnThreads + threadIdx.x;
    if (g >= a.m.ngroups) return;
    const int y = g / a.m.gpr, x0 = (g - y * a.m.gpr) * kPx;
    const int64_t e = (int64_t)g * kPx, ps = a.m.ps;
    const int npx = min(kPx, a.m.width - x0);
    Word* samples = static_cast<Word*>(a.m.samples);
    const int nN = a.p.nN, total = 3 * nN;

    uint32_t px[kPx];
    const uint8_t* r = a.frame + (int64_t)y * a.pitch + (int64_t)x0 * CN;
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        px[j] = 0;
#pragma unroll
        for (int c = 0; c < CN; ++c)
            if (j < npx) px[j] |= (uint32_t)r[j * CN + c] << (8 * c);
    }

    // what the update needs does not depend on the classification: in flight from the start
    const uint32_t pis = *reinterpret_cast<const uint32_t*>(a.m.index + e);
    const uint32_t pim = *reinterpret_cast<const uint32_t*>(a.m.index + ps + e);
    const uint32_t pil = *reinterpret_cast<const uint32_t*>(a.m.index + 2 * ps + e);
    const uint32_t pns = *reinterpret_cast<const uint32_t*>(a.m.next + e);
    const uint32_t pnm = *reinterpret_cast<const uint32_t*>(a.m.next + ps + e);
    const uint32_t pnl = *reinterpret_cast<const uint32_t*>(a.m.next + 2 * ps + e);

    // the first pass: a pixel beyond the row's end counts as decided
    knn_core::Classify cl[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        knn_core::classify_start(cl[j]);
        cl[j].background = !(j < npx);
    }
    // no pixel returns before its kNN-th sample: with kNN >= 2 the first two planes are always read, and both
    // loads are issued before either is used
    int n0 = 0;
    if (a.p.nkNN >= 2 && total >= 2) {
        uint32_t s0[kPx], s1[kPx];
        ld_words<CN>(samples + e, s0);
        ld_words<CN>(samples + ps + e, s1);
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (!cl[j].background) knn_core::classify_add<CN>(cl[j], s0[j], px[j], a.p.Tb, a.p.nkNN);
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (!cl[j].background) knn_core::classify_add<CN>(cl[j], s1[j], px[j], a.p.Tb, a.p.nkNN);
        n0 = 2;
    }
    for (int n = n0; n < total; ++n) {
        bool open = false;
#pragma unroll
        for (int j = 0; j < kPx; ++j) open = open || !cl[j].background;
        if (!open) break;
        uint32_t s[kPx];
        ld_words<CN>(samples + n * ps + e, s);
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (!cl[j].background) knn_core::classify_add<CN>(cl[j], s[j], px[j], a.p.Tb, a.p.nkNN);
    }

    // the shadow pass, where a pixel was not background
    knn_core::Shadow sh[kPx];
    bool undecided = false;
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        knn_core::shadow_start(sh[j]);
        if (cl[j].background || !a.p.detect_shadows) sh[j].verdict = 0;
        undecided = undecided || sh[j].verdict < 0;
    }
    if (undecided) {
        for (int n = 0; n < total; ++n) {
            bool open = false;
#pragma unroll
            for (int j = 0; j < kPx; ++j) open = open || sh[j].verdict < 0;
            if (!open) break;
            uint32_t s[kPx];
            ld_words<CN>(samples + n * ps + e, s);
#pragma unroll
            for (int j = 0; j < kPx; ++j)
                if (sh[j].verdict < 0) knn_core::shadow_add<CN>(sh[j], s[j], px[j], a.p.Tb, a.p.tau, a.p.nkNN, nullptr);
        }
    }

    // the update: long, mid, short, from the indices as they are before it
    int is[kPx], im[kPx], il[kPx], ns[kPx], nm[kPx], nl[kPx];
    unpack4(pis, is);
    unpack4(pim, im);
    unpack4(pil, il);
    unpack4(pns, ns);
    unpack4(pnm, nm);
    unpack4(pnl, nl);
    bool cs = false, cm = false, cg = false;
    int out[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        out[j] = 0;
        if (j < npx) {
            const bool bg = cl[j].background;
            const uint32_t include = bg || cl[j].Pbf >= a.p.nkNN;
            out[j] = knn_core::mask_value(bg ? 1 : sh[j].verdict == 2 ? 2 : 0, a.p.shadow_value);
            Word* slot_s = samples + (int64_t)is[j] * ps + e + j;
            Word* slot_m = samples + (int64_t)(nN + im[j]) * ps + e + j;
            Word* slot_l = samples + (int64_t)(2 * nN + il[j]) * ps + e + j;
            if (nl[j] == a.p.long_counter) {
                *slot_l = *slot_m;
                il[j] = knn_core::next_index(il[j], nN);
                cg = true;
            }
            if (nm[j] == a.p.mid_counter) {
                *slot_m = *slot_s;
                im[j] = knn_core::next_index(im[j], nN);
                cm = true;
            }
            if (ns[j] == a.p.short_counter) {
                *slot_s = (Word)(px[j] | include << (8 * CN));
                is[j] = knn_core::next_index(is[j], nN);
                cs = true;
            }
        }
    }
    if (cs) st_bytes(a.m.index + e, is);
    if (cm) st_bytes(a.m.index + ps + e, im);
    if (cg) st_bytes(a.m.index + 2 * ps + e, il);

    uint8_t* mrow = a.mask + (int64_t)y * a.mask_pitch + x0;
    if (npx == kPx && (reinterpret_cast<uintptr_t>(mrow) & (kPx - 1)) == 0) {
        st_bytes(mrow, out);
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (j < npx) mrow[j] = (uint8_t)out[j];
    }
}

struct KnnBgArgs {
    KnnPlanes m;
    uint8_t* img;
    int pitch, nN;
};

// getBackgroundImage: the planes are streamed while one of the lane's pixels has not met a flagged sample
template <int CN>
__global__ __launch_bounds__(kKnnThreads) void knn_background_kernel(KnnBgArgs a)
{
    typedef typename WordOf<CN>::type Word;
    const int g = blockIdx.x * kKnnThreads + threadIdx.x;
    if (g >= a.m.ngroups) return;
    const int y = g / a.m.gpr, x0 = (g - y * a.m.gpr) * kPx;
    const int64_t e = (int64_t)g * kPx, ps = a.m.ps;
    const int npx = min(kPx, a.m.width - x0);
    const Word* samples = static_cast<const Word*>(a.m.samples);
    uint32_t v[kPx];
    bool found[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        v[j] = 0;
        found[j] = !(j < npx);
    }
    for (int n = 0; n < 3 * a.nN; ++n) {
        bool open = false;
#pragma unroll
        for (int j = 0; j < kPx; ++j) open = open || !found[j];
        if (!open) break;
        uint32_t s[kPx];
        ld_words<CN>(samples + n * ps + e, s);
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            if (!found[j] && knn_core::flag_of<CN>(s[j])) {
                v[j] = s[j];
                found[j] = true;
            }
        }
    }
    uint8_t* row = a.img + (int64_t)y * a.pitch + (int64_t)x0 * CN;
#pragma unroll
    for (int j = 0; j < kPx; ++j)
        if (j < npx) {
#pragma unroll
            for (int c = 0; c < CN; ++c) row[j * CN + c] = (uint8_t)knn_core::channel(v[j], c);
        }
}

struct KnnModelArgs {
    KnnPlanes m;
    int cn, nN;
    uint8_t* samples;
    uint8_t* index3;
    uint8_t* next3;
    int32_t* counters;
    uint64_t* rng_state;
    const uint64_t* state;  // the current slot; NULL before the first fill: the state is still `seed`
    uint64_t seed;
    int32_t c0, c1, c2;
};

// the model in the reference's layout; one thread per pixel (tests and checkpoints, not a hot path)
__global__ __launch_bounds__(kKnnThreads) void knn_model_kernel(KnnModelArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;
    const int64_t npix = (int64_t)a.m.width * a.m.height;
    if (p == 0) {
        if (a.counters) a.counters[0] = a.c0, a.counters[1] = a.c1, a.counters[2] = a.c2;
        if (a.rng_state) *a.rng_state = a.state ? *a.state : a.seed;
    }
    if (p >= npix) return;
    const int y = (int)(p / a.m.width), x = (int)(p - (int64_t)y * a.m.width);
    const int64_t e = (int64_t)y * a.m.wp + x, ps = a.m.ps;
    const int nd = a.cn + 1, total = 3 * a.nN;
    if (a.samples) {
        uint8_t* o = a.samples + p * total * nd;
        for (int n = 0; n < total; ++n) {
            const uint32_t s = a.cn == 3 ? static_cast<const uint32_t*>(a.m.samples)[n * ps + e]
                                         : static_cast<const uint16_t*>(a.m.samples)[n * ps + e];
            for (int b = 0; b < nd; ++b) o[n * nd + b] = (uint8_t)(s >> (8 * b));
        }
    }
    for (int k = 0; k < 3; ++k) {
        if (a.index3) a.index3[k * npix + p] = a.m.index[k * ps + e];
        if (a.next3) a.next3[k * npix + p] = a.m.next[k * ps + e];
    }
}

struct KnnRanduArgs {
    uint8_t* plane;   // one next-update plane, rows of wp bytes
    int width, wp;
    int64_t total;    // width * height: the reference's continuous 1 x total plane
    uint32_t nblocks;
    knn_core::RanduPlan plan;
    const uint64_t* state_in;  // NULL for an object's first fill, which starts in `seed`
    uint64_t seed;
    uint64_t* state_out;
    uint64_t block_table[knn_core::kJumpBits];
    uint64_t lane_table[knn_core::kLaneBits];
};

// cv::randu over the plane: one wave per block of 1024 values, a lane's start by jump-ahead to the block and
// inside it (knn_core::randu_lane); a lane's values are consecutive, a wave's stores cover the block's 1 KiB
__global__ __launch_bounds__(kRanduThreads) void knn_randu_kernel(KnnRanduArgs a)
{
    const uint32_t b = blockIdx.x;
    const int64_t first = (int64_t)b * knn_core::kRngBlock;
    const int len = (int)min((int64_t)knn_core::kRngBlock, a.total - first);
    const int width = a.width, wp = a.wp;
    int x = -1;
    uint8_t* dst = nullptr;
    bool last = false;
    const uint64_t st = knn_core::randu_lane(a.plan, a.block_table, a.lane_table, a.state_in ? *a.state_in : a.seed, b,
                                             (int)threadIdx.x, len, &last, [&](int i, uint8_t v) {
                                                 if (x < 0) {  // the lane's first value: its row and column
                                                     const int64_t g = first + i;
                                                     const int y = (int)(g / width);
                                                     x = (int)(g - (int64_t)y * width);
                                                     dst = a.plane + (int64_t)y * wp;
                                                 }
                                                 dst[x] = v;
                                                 if (++x == width) {
                                                     x = 0;
                                                     dst += wp;
                                                 }
                                             });
    if (last && b == a.nblocks - 1) *a.state_out = st;
}

}  // namespace
}  // namespace tbdk

using namespace tbdk;

struct tbdk_knn {
    tbdk_ctx* ctx = nullptr;
    tbdk_knn_config cfg{};
    void* mem = nullptr;
    size_t model_bytes = 0;  // samples, index and next planes: what an initialisation zeroes
    KnnPlanes pl{};
    uint64_t* state = nullptr;  // two slots
    int cur = 0;                // the slot that holds the state after everything enqueued
    bool filled = false;        // false: no fill yet, the state is cfg.rng_state and no slot holds it
    knn_core::HostState host{};
    knn_core::JumpTables jump{};
    hipStream_t last_stream = nullptr;
};

namespace {

bool knn_params_ok(const tbdk_knn_config& c)
{
    return c.history >= 1 && c.shadow_value >= 0 && c.shadow_value <= 255 && c.dist2_threshold == c.dist2_threshold &&
           c.shadow_threshold == c.shadow_threshold;
}

knn_core::Settings knn_settings(const tbdk_knn_config& c)
{
    knn_core::Settings s;
    s.history = c.history;
    s.nsamples = c.nsamples;
    s.knn_samples = c.knn_samples;
    s.detect_shadows = c.detect_shadows != 0;
    s.shadow_value = c.shadow_value;
    s.dist2_threshold = c.dist2_threshold;
    s.shadow_threshold = c.shadow_threshold;
    return s;
}

hipError_t knn_clear(tbdk_knn* m, hipStream_t s) { return hipMemsetAsync(m->mem, 0, m->model_bytes, s); }

hipError_t knn_fill(tbdk_knn* m, int which, int period, hipStream_t s)
{
    KnnRanduArgs a;
    a.plane = m->pl.next + (int64_t)which * m->pl.ps;
    a.width = m->pl.width;
    a.wp = m->pl.wp;
    a.total = (int64_t)m->pl.width * m->pl.height;
    a.nblocks = (uint32_t)((a.total + knn_core::kRngBlock - 1) / knn_core::kRngBlock);
    a.plan = knn_core::randu_plan(period);
    a.state_in = m->filled ? m->state + m->cur : nullptr;
    a.seed = m->cfg.rng_state;
    a.state_out = m->state + (m->cur ^ 1);
    const bool small = a.plan.mode == knn_core::RANDU_SMALL;
    std::memcpy(a.block_table, small ? m->jump.p256 : m->jump.p1024, sizeof(a.block_table));
    std::memcpy(a.lane_table, small ? m->jump.p4 : m->jump.p16, sizeof(a.lane_table));
    const unsigned blocks = a.nblocks;
    hipLaunchKernelGGL(knn_randu_kernel, dim3(blocks), dim3(kRanduThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        m->cur ^= 1;
        m->filled = true;
    }
    return e;
}

}  // namespace

extern "C" {

int tbdk_knn_config_default(int width, int height, int channels, tbdk_knn_config* cfg)
{
    if (!cfg) return TBDK_EINVAL;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->width = width;
    cfg->height = height;
    cfg->channels = channels;
    cfg->history = 500;  // bgfg_KNN.cpp:58-65, :71-95
    cfg->nsamples = 7;
    cfg->knn_samples = 2;  // MAX(1, cvRound(0.1 * 7 * 3 + 0.40))
    cfg->detect_shadows = 1;
    cfg->shadow_value = 127;
    cfg->dist2_threshold = 400.0f;
    cfg->shadow_threshold = 0.5f;
    cfg->rng_state = 0xffffffffull;  // a fresh thread's cv::theRNG()
    return TBDK_OK;
}

int tbdk_knn_create(tbdk_ctx* ctx, const tbdk_knn_config* cfg, tbdk_knn** out)
{
    if (!ctx || !cfg || !out) return TBDK_EINVAL;
    *out = nullptr;
    const tbdk_knn_config& c = *cfg;
    if (c.width <= 0 || c.height <= 0 || c.width > 65535 || c.height > 65535) return TBDK_EINVAL;
    if (c.channels != 1 && c.channels != 3) return TBDK_EINVAL;
    if (c.nsamples < 1 || c.nsamples > knn_core::kMaxSamples || !knn_params_ok(c)) return TBDK_EINVAL;
    const int wp = align_up(c.width, 4);
    const int64_t groups = (int64_t)(wp / kPx) * c.height;
    if (groups > (int64_t)1 << 29) return TBDK_EINVAL;  // group and block indices stay in int
    tbdk_knn* m = new (std::nothrow) tbdk_knn;
    if (!m) return TBDK_ENOMEM;
    m->ctx = ctx;
    m->cfg = c;
    KnnPlanes& p = m->pl;
    p.width = c.width;
    p.height = c.height;
    p.wp = wp;
    p.gpr = wp / kPx;
    p.ngroups = (int)groups;
    p.ps = (groups * kPx + 63) / 64 * 64;
    const size_t ps = (size_t)p.ps, word = c.channels == 3 ? 4 : 2;
    const size_t sample_bytes = (size_t)3 * c.nsamples * ps * word;
    m->model_bytes = sample_bytes + 6 * ps;
    DeviceGuard g(ctx->device);
    const int rc = map_status(dev_alloc(&m->mem, m->model_bytes + 2 * sizeof(uint64_t), ctx->opt_alloc_fill));
    if (rc != TBDK_OK) {
        delete m;
        return rc;
    }
    p.samples = m->mem;
    p.index = static_cast<uint8_t*>(m->mem) + sample_bytes;
    p.next = p.index + 3 * ps;
    m->state = reinterpret_cast<uint64_t*>(p.next + 3 * ps);  // ps is a multiple of 64: aligned
    knn_core::jump_tables(&m->jump);
    *out = m;
    return TBDK_OK;
}

int tbdk_knn_destroy(tbdk_knn* m)
{
    if (!m) return TBDK_EINVAL;
    DeviceGuard g(m->ctx->device);
    (void)hipStreamSynchronize(m->last_stream);
    if (m->mem) (void)hipFree(m->mem);
    delete m;
    return TBDK_OK;
}

int tbdk_knn_reset(tbdk_knn* m)
{
    if (!m) return TBDK_EINVAL;
    m->host = knn_core::HostState{};
    return TBDK_OK;
}

int tbdk_knn_set_params(tbdk_knn* m, const tbdk_knn_config* cfg)
{
    if (!m || !cfg) return TBDK_EINVAL;
    const tbdk_knn_config& c = *cfg;
    if (c.width != m->cfg.width || c.height != m->cfg.height || c.channels != m->cfg.channels ||
        c.nsamples != m->cfg.nsamples || !knn_params_ok(c))
        return TBDK_EINVAL;
    const uint64_t seed = m->cfg.rng_state;
    m->cfg = c;
    m->cfg.rng_state = seed;  // read at creation only
    return TBDK_OK;
}

int tbdk_knn_apply(tbdk_knn* m, const uint8_t* frame, int pitch, uint8_t* fgmask, int mask_pitch, double learning_rate,
                   void* stream)
{
    if (!m || !frame || !fgmask || mask_pitch < m->cfg.width || (int64_t)pitch < (int64_t)m->cfg.width * m->cfg.channels)
        return TBDK_EINVAL;
    knn_core::FramePlan plan;
    if (!knn_core::plan_frame(m->host, m->cfg.history, m->cfg.nsamples, learning_rate, &plan)) return TBDK_EINVAL;
    tbdk_ctx* ctx = m->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    KnnApplyArgs a;
    a.m = m->pl;
    a.frame = frame;
    a.pitch = pitch;
    a.mask = fgmask;
    a.mask_pitch = mask_pitch;
    a.p = knn_core::frame_params(knn_settings(m->cfg), plan);
    const int blocks = (m->pl.ngroups + kKnnThreads - 1) / kKnnThreads;
    int rec = timing_begin(ctx, "knn_apply", s);
    hipError_t e = plan.reinit ? knn_clear(m, s) : hipSuccess;
    if (e == hipSuccess) {
        if (m->cfg.channels == 1)
            hipLaunchKernelGGL(knn_apply_kernel<1>, dim3(blocks), dim3(kKnnThreads), 0, s, a);
        else
            hipLaunchKernelGGL(knn_apply_kernel<3>, dim3(blocks), dim3(kKnnThreads), 0, s, a);
        e = hipGetLastError();
    }
    timing_end(ctx, rec, s);
    if (e != hipSuccess) return map_status(e);
    m->host = plan.after;
    m->last_stream = s;
    if (plan.fill[0] || plan.fill[1] || plan.fill[2]) {
        rec = timing_begin(ctx, "knn_randu", s);
        for (int i = 0; i < 3 && e == hipSuccess; ++i)
            if (plan.fill[i]) e = knn_fill(m, i, plan.periods[i], s);
        timing_end(ctx, rec, s);
    }
    return map_status(e);
}

int tbdk_knn_get_background(tbdk_knn* m, uint8_t* img, int pitch, void* stream)
{
    if (!m || !img || (int64_t)pitch < (int64_t)m->cfg.width * m->cfg.channels) return TBDK_EINVAL;
    tbdk_ctx* ctx = m->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    KnnBgArgs a;
    a.m = m->pl;
    a.img = img;
    a.pitch = pitch;
    a.nN = m->cfg.nsamples;
    const int blocks = (m->pl.ngroups + kKnnThreads - 1) / kKnnThreads;
    const int rec = timing_begin(ctx, "knn_background", s);
    // before the first apply the model is whatever the allocation held: it is cleared, as the first apply would
    hipError_t e = m->host.nframes == 0 ? knn_clear(m, s) : hipSuccess;
    if (e == hipSuccess) {
        if (m->cfg.channels == 1)
            hipLaunchKernelGGL(knn_background_kernel<1>, dim3(blocks), dim3(kKnnThreads), 0, s, a);
        else
            hipLaunchKernelGGL(knn_background_kernel<3>, dim3(blocks), dim3(kKnnThreads), 0, s, a);
        e = hipGetLastError();
    }
    timing_end(ctx, rec, s);
    if (e == hipSuccess) m->last_stream = s;
    return map_status(e);
}

int tbdk_knn_get_model(tbdk_knn* m, uint8_t* samples, uint8_t* index3, uint8_t* next3, int32_t* counters,
                       uint64_t* rng_state, void* stream)
{
    if (!m) return TBDK_EINVAL;
    tbdk_ctx* ctx = m->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    KnnModelArgs a;
    a.m = m->pl;
    a.cn = m->cfg.channels;
    a.nN = m->cfg.nsamples;
    a.samples = samples;
    a.index3 = index3;
    a.next3 = next3;
    a.counters = counters;
    a.rng_state = rng_state;
    a.state = m->filled ? m->state + m->cur : nullptr;
    a.seed = m->cfg.rng_state;
    a.c0 = m->host.counters[0];
    a.c1 = m->host.counters[1];
    a.c2 = m->host.counters[2];
    const int64_t px = (int64_t)m->cfg.width * m->cfg.height;
    const int blocks = (int)((px + kKnnThreads - 1) / kKnnThreads);
    const int rec = timing_begin(ctx, "knn_model", s);
    hipError_t e = m->host.nframes == 0 ? knn_clear(m, s) : hipSuccess;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(knn_model_kernel, dim3(blocks), dim3(kKnnThreads), 0, s, a);
        e = hipGetLastError();
    }
    timing_end(ctx, rec, s);
    if (e == hipSuccess) m->last_stream = s;
    return map_status(e);
}

int tbdk_knn_frames(tbdk_knn* m, int* nframes)
{
    if (!m || !nframes) return TBDK_EINVAL;
    *nframes = m->host.nframes;
    return TBDK_OK;
}

}  // extern "C"
