// klt_tracker.hip — the device-resident KLT point tracker (tbdk_klt_tracker_*;
// the loop of the reference's samples/python/lk_track.py, include/tbdk.h) and
// tbdk_mask_circles_u8.  A step enqueues, on the caller's stream: the pyramid
// build, the forward and backward PyrLK launches over max_tracks indices gated
// by the device-side live count (lk_internal's segment layout, one segment),
// the compaction, and on a detection frame the disc mask, the whole-frame
// masked GFTT (wide path allowed), cornerSubPix and the append.  The host never
// reads the count.  New kernels: klt_compact_kernel, klt_mask_circles_kernel,
// klt_append_kernel (KLT point tracker).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "tbdk_internal.hpp"

namespace tbdk {
namespace {

constexpr int kKltMaxRadius = 64;
constexpr int kKltMaxLen = 64;
constexpr int kKltMaxTracks = 65536;
constexpr int kScanThreads = 1024;  // one workgroup: the compaction's tile, the append's stride

// one copy of the track state, max_tracks entries each
struct KltState {
    int32_t* ids;
    int32_t* lens;
    float2* last;  // == hist[i][lens[i] - 1]: the contiguous point list PyrLK reads
    float2* hist;  // track_len per track, oldest first, zero beyond lens[i]
};

struct KltCompactArgs {
    KltState in, out;
    const float2* next;     // the forward pass's points
    const uint8_t* status;  // the checked status
    int32_t* count;
    const int32_t* next_id;
    tbdk_klt_tracker_stats* stats;
    int track_len, max_tracks, frame_idx;
    int track;  // 0: no previous frame, the state stays where it is (only the statistics are written)
};

// Order-preserving compaction of the tracks whose checked status is set, from
// state `in` into state `out`, each survivor with the new point appended (the
// oldest dropped beyond track_len).  One workgroup walks [0, count) in tiles of
// 1024 with a carried prefix: per tile a ballot per wave, the 16 wave sums
// through LDS, survivor t of the tile -> s_src[t]; then the tile's survivors'
// scalars, and their histories with consecutive lanes on consecutive floats of a
// row.  No atomics and one workgroup: the result does not depend on any order
// of execution.
__global__ __launch_bounds__(kScanThreads) void klt_compact_kernel(KltCompactArgs a)
{
    __shared__ int s_src[kScanThreads];
    __shared__ int s_len[kScanThreads];
    __shared__ int s_wsum[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = a.track_len;
    const int n = min(max(*a.count, 0), a.max_tracks);
    __syncthreads();  // every thread has read the count before thread 0 rewrites it
    int carry = a.track ? 0 : n;
    if (a.track) {
        for (int base = 0; base < n; base += kScanThreads) {
            const int i = base + tid;
            const bool keep = i < n && a.status[i] != 0;
            const unsigned long long b = __ballot(keep);
            if (lane == 0) s_wsum[wv] = __popcll(b);
            __syncthreads();
            int woff = 0, tot = 0;
            for (int w = 0; w < kScanThreads / 64; ++w) {
                const int c = s_wsum[w];
                woff += w < wv ? c : 0;
                tot += c;
            }
            if (keep) {
                const int t = woff + __popcll(b & ((1ull << lane) - 1ull));
                s_src[t] = i;
                s_len[t] = min(max(a.in.lens[i], 1), L);
            }
            __syncthreads();
            if (tid < tot) {
                const int i = s_src[tid], j = carry + tid;
                a.out.ids[j] = a.in.ids[i];
                a.out.lens[j] = min(s_len[tid] + 1, L);
                a.out.last[j] = a.next[i];
            }
            for (int e = tid; e < tot * L; e += kScanThreads) {
                const int t = e / L, k = e - t * L;
                const int i = s_src[t], len = s_len[t];
                const int nl = min(len + 1, L), sh = len == L ? 1 : 0;
                float2 v = make_float2(0.f, 0.f);
                if (k < nl - 1)
                    v = a.in.hist[(size_t)i * L + k + sh];
                else if (k == nl - 1)
                    v = a.next[i];
                a.out.hist[(size_t)(carry + t) * L + k] = v;
            }
            carry += tot;
            __syncthreads();  // the tile's lists are rewritten by the next one
        }
    }
    if (tid == 0) {
        *a.count = carry;
        tbdk_klt_tracker_stats st;
        st.tracks_in = n;
        st.kept = carry;
        st.detected = st.appended = st.dropped = 0;
        st.next_id = *a.next_id;
        st.frame_idx = a.frame_idx;
        *a.stats = st;
    }
}

struct KltAppendArgs {
    KltState st;
    const float2* src;
    const int32_t* src_count;  // device count of src (the GFTT row's), or nullptr: src_n points
    int src_n;                 // capacity of src, or its length
    int32_t* count;
    int32_t* next_id;
    tbdk_klt_tracker_stats* stats;
    int track_len, max_tracks;
    int detected;  // != 0: the points are a detection's (counted in stats.detected)
};

// min(found, max_tracks - count) points of src behind the live tracks, each a
// track of length 1 with the next id; one workgroup, which alone reads and
// rewrites the count, the id counter and the statistics
__global__ __launch_bounds__(kScanThreads) void klt_append_kernel(KltAppendArgs a)
{
    const int tid = threadIdx.x;
    const int L = a.track_len;
    const int n = min(max(*a.count, 0), a.max_tracks);
    const int found = a.src_count ? min(max(*a.src_count, 0), a.src_n) : a.src_n;
    const int id0 = *a.next_id;
    __syncthreads();
    const int take = min(found, a.max_tracks - n);
    for (int e = tid; e < take; e += kScanThreads) {
        a.st.ids[n + e] = id0 + e;
        a.st.lens[n + e] = 1;
        a.st.last[n + e] = a.src[e];
    }
    for (int e = tid; e < take * L; e += kScanThreads) {
        const int t = e / L, k = e - t * L;
        a.st.hist[(size_t)(n + t) * L + k] = k == 0 ? a.src[t] : make_float2(0.f, 0.f);
    }
    if (tid == 0) {
        *a.count = n + take;
        *a.next_id = id0 + take;
        tbdk_klt_tracker_stats st = *a.stats;
        if (a.detected) st.detected += found;
        st.appended += take;
        st.dropped += found - take;
        st.next_id = id0 + take;
        *a.stats = st;
    }
}

struct KltMaskArgs {
    uint8_t* mask;
    int w, h, pitch;
    const float2* pts;
    const int32_t* count;  // device count, or nullptr: n points
    int n;
    int radius, value;
    uint8_t hw[kKltMaxRadius + 1];  // half width of the circle's row at |dy| (circle_half_widths)
};

// One wave per point: the rows of its disc in turn, the lanes along a row.
// Every thread of the launch writes the same byte value, so overlapping discs
// need no ordering.  Rows and columns are clipped to the mask before any store.
__global__ __launch_bounds__(256) void klt_mask_circles_kernel(KltMaskArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int cnt = a.count ? min(max(*a.count, 0), a.n) : a.n;
    if (p >= cnt) return;
    const float2 c = a.pts[p];
    if (!(fabsf(c.x) < 1e9f) || !(fabsf(c.y) < 1e9f)) return;  // NaN, infinite or beyond int range: nothing to draw
    const int cx = (int)c.x, cy = (int)c.y, r = a.radius;      // toward zero, as the sample's np.int32 cast
    if (cx + r < 0 || cx - r >= a.w || cy + r < 0 || cy - r >= a.h) return;
    const uint8_t v = (uint8_t)a.value;
    for (int y = max(cy - r, 0); y <= min(cy + r, a.h - 1); ++y) {
        const int hw = a.hw[abs(y - cy)];
        const int x1 = min(cx + hw, a.w - 1);
        uint8_t* row = a.mask + (size_t)y * a.pitch;
        for (int x = max(cx - hw, 0) + lane; x <= x1; x += 64) row[x] = v;
    }
}

// cv::circle(img, c, radius, color, -1)'s rows (imgproc/src/drawing.cpp:1486-1628,
// Circle() with fill): per iteration of its midpoint walk rows cy -+ dy get the
// span cx -+ dx and rows cy -+ dx the span cx -+ dy; a row ends up with the widest
// span it was given.  Its clipping only cuts the spans at the image.
void circle_half_widths(int radius, uint8_t* hw)
{
    std::memset(hw, 0, kKltMaxRadius + 1);
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        hw[dy] = (uint8_t)std::max<int>(hw[dy], dx);
        hw[dx] = (uint8_t)std::max<int>(hw[dx], dy);
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

hipError_t launch_mask_circles(uint8_t* mask, int w, int h, int pitch, const float* pts,
                               const int32_t* count, int n, int radius, int value, const uint8_t* hw, hipStream_t s)
{
    KltMaskArgs a;
    a.mask = mask;
    a.w = w;
    a.h = h;
    a.pitch = pitch;
    a.pts = reinterpret_cast<const float2*>(pts);
    a.count = count;
    a.n = n;
    a.radius = radius;
    a.value = value;
    std::memcpy(a.hw, hw, sizeof(a.hw));
    hipLaunchKernelGGL(klt_mask_circles_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
}  // namespace tbdk

using namespace tbdk;

struct tbdk_klt_tracker {
    tbdk_ctx* ctx = nullptr;
    tbdk_klt_tracker_config cfg{};
    tbdk_pyr pyr[2]{};
    int cur = 0;  // the pyramid the next step builds; the other one holds the previous frame
    bool have_prev = false;
    int frame_idx = 0;
    void* mem = nullptr;  // everything below but the pyramids and the GFTT scratch
    size_t mem_bytes = 0;
    KltState st[2]{};
    int sidx = 0;  // the live copy of the state
    float2* next = nullptr;
    uint8_t* status = nullptr;
    int32_t* count = nullptr;
    int32_t* next_id = nullptr;
    int32_t* found = nullptr;  // the GFTT row's count
    tbdk_klt_tracker_stats* stats = nullptr;
    float2* corners = nullptr;  // the GFTT row, max_corners
    uint8_t* mask = nullptr;
    int mask_pitch = 0;
    GfttRoi* d_roi = nullptr;
    GfttRoi h_roi{};
    GfttPlan plan{};
    GfttScratch gftt;  // the tracker's own: the context's serves the standalone calls on other streams
    tbdk_gftt_params gp{};
    tbdk_lk_params lp{};
    tbdk_subpix_params sp{};
    uint8_t hw[kKltMaxRadius + 1]{};
    hipStream_t last_stream = nullptr;
};

namespace {

int klt_append(tbdk_klt_tracker* t, const float2* src, const int32_t* src_count, int src_n, int detected,
               hipStream_t s)
{
    KltAppendArgs a;
    a.st = t->st[t->sidx];
    a.src = src;
    a.src_count = src_count;
    a.src_n = src_n;
    a.count = t->count;
    a.next_id = t->next_id;
    a.stats = t->stats;
    a.track_len = t->cfg.track_len;
    a.max_tracks = t->cfg.max_tracks;
    a.detected = detected;
    const int rec = timing_begin(t->ctx, "klt_append", s);
    hipLaunchKernelGGL(klt_append_kernel, dim3(1), dim3(kScanThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    timing_end(t->ctx, rec, s);
    return map_status(e);
}

// the state as tbdk_klt_tracker_reset leaves it (synchronous)
int klt_clear(tbdk_klt_tracker* t)
{
    const hipError_t e = hipMemset(t->mem, 0, t->mem_bytes);
    if (e != hipSuccess) return map_status(e);
    const tbdk_klt_tracker_stats st{0, 0, 0, 0, 0, 0, -1};
    t->cur = 0;
    t->have_prev = false;
    t->frame_idx = 0;
    t->sidx = 0;
    return map_status(hipMemcpy(t->stats, &st, sizeof(st), hipMemcpyHostToDevice));
}

}  // namespace

extern "C" {

int tbdk_klt_tracker_default_config(int width, int height, tbdk_klt_tracker_config* cfg)
{
    if (!cfg) return TBDK_EINVAL;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->width = width;
    cfg->height = height;
    cfg->win = 15;  // lk_track.py:31-33
    cfg->max_level = 2;
    cfg->lk_iters = 10;
    cfg->lk_epsilon = 0.03;
    cfg->min_eig_threshold = 1e-4f;
    cfg->back_threshold = 1.0f;  // :60
    cfg->max_corners = 500;  // :35-38
    cfg->quality_level = 0.3;
    cfg->min_distance = 7;
    cfg->block_size = 7;
    cfg->use_harris = 0;
    cfg->harris_k = 0.04;
    cfg->detect_interval = 5;  // :42-43
    cfg->track_len = 10;
    cfg->mask_radius = 5;  // :78
    cfg->subpix_win = 0;
    cfg->max_tracks = 8192;
    return TBDK_OK;
}

int tbdk_klt_tracker_create(tbdk_ctx* ctx, const tbdk_klt_tracker_config* cfg, tbdk_klt_tracker** out)
{
    if (!ctx || !cfg || !out) return TBDK_EINVAL;
    *out = nullptr;
    const tbdk_klt_tracker_config& c = *cfg;
    if (c.width <= 0 || c.height <= 0 || c.width > 65535 || c.height > 65535) return TBDK_EINVAL;
    // tbdk_lk_sparse_fb's and the pyramid's
    if (c.win <= 2 || c.win > 63 || c.max_level < 0 || !(c.back_threshold > 0.f)) return TBDK_EINVAL;
    if (c.track_len < 1 || c.track_len > kKltMaxLen || c.detect_interval < 1 || c.mask_radius > kKltMaxRadius ||
        c.max_tracks < 1 || c.max_tracks > kKltMaxTracks || c.max_corners > c.max_tracks || c.subpix_win < 0)
        return TBDK_EINVAL;
    // tbdk_corner_sub_pix's
    if (c.subpix_win > 0 && (c.subpix_win > 15 || c.width < 2 * c.subpix_win + 5 || c.height < 2 * c.subpix_win + 5))
        return TBDK_EINVAL;
    tbdk_klt_tracker* t = new (std::nothrow) tbdk_klt_tracker;
    if (!t) return TBDK_ENOMEM;
    t->ctx = ctx;
    t->cfg = c;
    t->gp = tbdk_gftt_params{c.max_corners, c.quality_level, c.min_distance, c.block_size, c.use_harris, c.harris_k};
    t->lp = tbdk_lk_params{c.win, c.win, c.max_level, c.lk_iters, c.lk_epsilon, 0, c.min_eig_threshold, 0};
    t->sp = tbdk_subpix_params{c.subpix_win, c.subpix_win, -1, -1, 3, 20, 0.03};  // lkdemo.cpp:85
    circle_half_widths(std::max(c.mask_radius, 0), t->hw);
    // tbdk_gftt_rois_masked's: the parameters, and the one whole-frame ROI's layout
    const tbdk_roi roi{0, 0, c.width, c.height};
    int rc = gftt_prepare(&roi, 1, c.width, c.height, &t->gp, &t->h_roi, &t->plan);
    if (rc != TBDK_OK) {
        delete t;
        return rc;
    }
    DeviceGuard g(ctx->device);
    t->gftt.fill = ctx->opt_alloc_fill;
    rc = tbdk_pyr_create_levels(ctx, c.width, c.height, c.max_level, c.win, c.win, &t->pyr[0]);
    if (rc == TBDK_OK) rc = tbdk_pyr_create_levels(ctx, c.width, c.height, c.max_level, c.win, c.win, &t->pyr[1]);
    // GFTT scratch for the whole-frame ROI, the wide selection's and the response planes' included
    if (rc == TBDK_OK) rc = gftt_reserve(t->gftt, ctx->device, 1, t->plan.total);
    if (rc == TBDK_OK) rc = gftt_reserve_wide(t->gftt, ctx->device, 1, t->plan.total);
    if (rc == TBDK_OK && gftt_generic(&t->gp)) rc = gftt_reserve_resp(t->gftt, ctx->device, t->plan.total);
    if (rc == TBDK_OK) {
        const size_t M = (size_t)c.max_tracks, L = (size_t)c.track_len;
        t->mask_pitch = align_up(c.width, 64);
        const size_t sizes[] = {
            M * 4, M * 4, M * 8, M * L * 8,  // state 0: ids, lens, last, hist
            M * 4, M * 4, M * 8, M * L * 8,  // state 1
            M * 8, M,                        // next, status
            256,                             // count, next_id, found, stats
            (size_t)c.max_corners * 8, (size_t)t->mask_pitch * c.height, sizeof(GfttRoi)};
        size_t off[sizeof(sizes) / sizeof(sizes[0])], total = 0;
        for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
            off[i] = total;
            total += up256(sizes[i]);
        }
        rc = map_status(dev_alloc(&t->mem, total, ctx->opt_alloc_fill));
        if (rc == TBDK_OK) {
            t->mem_bytes = total;
            uint8_t* b = static_cast<uint8_t*>(t->mem);
            for (int k = 0; k < 2; ++k)
                t->st[k] = KltState{reinterpret_cast<int32_t*>(b + off[4 * k]), reinterpret_cast<int32_t*>(b + off[4 * k + 1]),
                                    reinterpret_cast<float2*>(b + off[4 * k + 2]),
                                    reinterpret_cast<float2*>(b + off[4 * k + 3])};
            t->next = reinterpret_cast<float2*>(b + off[8]);
            t->status = b + off[9];
            t->count = reinterpret_cast<int32_t*>(b + off[10]);
            t->next_id = t->count + 1;
            t->found = t->count + 2;
            t->stats = reinterpret_cast<tbdk_klt_tracker_stats*>(t->count + 8);
            t->corners = reinterpret_cast<float2*>(b + off[11]);
            t->mask = b + off[12];
            t->d_roi = reinterpret_cast<GfttRoi*>(b + off[13]);
            rc = klt_clear(t);
            if (rc == TBDK_OK)
                rc = map_status(hipMemcpy(t->d_roi, &t->h_roi, sizeof(GfttRoi), hipMemcpyHostToDevice));
        }
    }
    if (rc != TBDK_OK) {
        tbdk_klt_tracker_destroy(t);
        return rc;
    }
    *out = t;
    return TBDK_OK;
}

int tbdk_klt_tracker_destroy(tbdk_klt_tracker* t)
{
    if (!t) return TBDK_EINVAL;
    DeviceGuard g(t->ctx->device);
    (void)hipStreamSynchronize(t->last_stream);
    if (t->mem) (void)hipFree(t->mem);
    gftt_scratch_free(t->gftt);
    for (tbdk_pyr& p : t->pyr)
        if (p.storage) tbdk_pyr_destroy(t->ctx, &p);
    delete t;
    return TBDK_OK;
}

int tbdk_klt_tracker_reset(tbdk_klt_tracker* t)
{
    if (!t) return TBDK_EINVAL;
    DeviceGuard g(t->ctx->device);
    const hipError_t e = hipStreamSynchronize(t->last_stream);
    if (e != hipSuccess) return map_status(e);
    const int rc = klt_clear(t);
    // klt_clear zeroed the ROI table with the rest
    return rc != TBDK_OK ? rc : map_status(hipMemcpy(t->d_roi, &t->h_roi, sizeof(GfttRoi), hipMemcpyHostToDevice));
}

int tbdk_klt_tracker_step(tbdk_klt_tracker* t, const uint8_t* frame, int pitch, int flags, void* stream)
{
    if (!t || !frame || pitch < t->cfg.width || (flags & ~TBDK_KLT_DETECT_NOW) != 0) return TBDK_EINVAL;
    const tbdk_klt_tracker_config& c = t->cfg;
    tbdk_ctx* ctx = t->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    t->last_stream = s;
    tbdk_pyr& P = t->pyr[t->cur];
    int rc = tbdk_pyr_build(ctx, frame, pitch, &P, s);
    if (rc != TBDK_OK) return rc;
    const KltState& live = t->st[t->sidx];
    if (t->have_prev) {
        // max_tracks launch indices, one segment: index i runs iff i < count; forward, then the check
        const tbdk_pyr& Q = t->pyr[t->cur ^ 1];
        const float* pts = reinterpret_cast<const float*>(live.last);
        float* nxt = reinterpret_cast<float*>(t->next);
        rc = lk_internal(ctx, &Q, &P, pts, nxt, t->status, nullptr, nullptr, c.max_tracks, &t->lp, t->count,
                         c.max_tracks, s);
        if (rc != TBDK_OK) return rc;
        const LkBack back{nullptr, nullptr, c.back_threshold};
        rc = lk_internal(ctx, &P, &Q, pts, nxt, t->status, nullptr, nullptr, c.max_tracks, &t->lp, t->count,
                         c.max_tracks, s, nullptr, nullptr, nullptr, &back);
        if (rc != TBDK_OK) return rc;
    }
    {
        KltCompactArgs a;
        a.in = live;
        a.out = t->st[t->sidx ^ 1];
        a.next = t->next;
        a.status = t->status;
        a.count = t->count;
        a.next_id = t->next_id;
        a.stats = t->stats;
        a.track_len = c.track_len;
        a.max_tracks = c.max_tracks;
        a.frame_idx = t->frame_idx;
        a.track = t->have_prev ? 1 : 0;
        const int rec = timing_begin(ctx, "klt_compact", s);
        hipLaunchKernelGGL(klt_compact_kernel, dim3(1), dim3(kScanThreads), 0, s, a);
        const hipError_t e = hipGetLastError();
        timing_end(ctx, rec, s);
        if (e != hipSuccess) return map_status(e);
        if (t->have_prev) t->sidx ^= 1;
    }
    if (t->frame_idx % c.detect_interval == 0 || (flags & TBDK_KLT_DETECT_NOW)) {
        const KltState& cur = t->st[t->sidx];
        if (c.mask_radius >= 0) {
            const int rec = timing_begin(ctx, "klt_mask", s);
            hipError_t e = hipMemsetAsync(t->mask, 255, (size_t)t->mask_pitch * c.height, s);
            if (e == hipSuccess)
                e = launch_mask_circles(t->mask, c.width, c.height, t->mask_pitch,
                                        reinterpret_cast<const float*>(cur.last), t->count, c.max_tracks, c.mask_radius, 0,
                                        t->hw, s);
            timing_end(ctx, rec, s);
            if (e != hipSuccess) return map_status(e);
        }
        // the frame as the pyramid's level 0 holds it: the caller's buffer is not read again
        const tbdk_level& L0 = P.lv[0];
        const uint8_t* img = L0.data + (size_t)L0.pad * L0.pitch + L0.pad;
        rc = gftt_launch(ctx, t->gftt, img, L0.pitch, t->d_roi, t->plan, &t->gp, reinterpret_cast<float*>(t->corners),
                         t->found, s, nullptr, 0, &t->h_roi, c.mask_radius >= 0 ? t->mask : nullptr, t->mask_pitch,
                         TBDK_PIX_U8, true);
        if (rc != TBDK_OK) return rc;
        if (c.subpix_win > 0) {
            rc = subpix_launch(ctx, img, TBDK_PIX_U8, c.width, c.height, L0.pitch, reinterpret_cast<float*>(t->corners),
                               t->found, 1, c.max_corners, &t->sp, s);
            if (rc != TBDK_OK) return rc;
        }
        rc = klt_append(t, t->corners, t->found, c.max_corners, 1, s);
        if (rc != TBDK_OK) return rc;
    }
    t->frame_idx++;
    t->cur ^= 1;
    t->have_prev = true;
    return TBDK_OK;
}

int tbdk_klt_tracker_add_points(tbdk_klt_tracker* t, const float* device_pts, int n, void* stream)
{
    if (!t || n < 0 || (n > 0 && !device_pts)) return TBDK_EINVAL;
    if (n == 0) return TBDK_OK;
    DeviceGuard g(t->ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    t->last_stream = s;
    return klt_append(t, reinterpret_cast<const float2*>(device_pts), nullptr, n, 0, s);
}

int tbdk_klt_tracker_read(tbdk_klt_tracker* t, int32_t* ids, float* last_pts, int32_t* lens, float* hist, int cap,
                          int* n, tbdk_klt_tracker_stats* stats)
{
    if (!t || cap < 0) return TBDK_EINVAL;
    DeviceGuard g(t->ctx->device);
    hipError_t e = hipStreamSynchronize(t->last_stream);
    int32_t cnt = 0;
    if (e == hipSuccess) e = hipMemcpy(&cnt, t->count, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && stats) e = hipMemcpy(stats, t->stats, sizeof(*stats), hipMemcpyDeviceToHost);
    const KltState& st = t->st[t->sidx];
    const size_t k = (size_t)std::min<int>(std::max<int>(cnt, 0), cap), L = (size_t)t->cfg.track_len;
    if (e == hipSuccess && ids && k) e = hipMemcpy(ids, st.ids, k * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && last_pts && k) e = hipMemcpy(last_pts, st.last, k * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && lens && k) e = hipMemcpy(lens, st.lens, k * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && hist && k) e = hipMemcpy(hist, st.hist, k * L * 8, hipMemcpyDeviceToHost);
    if (n) *n = cnt;
    return map_status(e);
}

int tbdk_klt_tracker_device_state(tbdk_klt_tracker* t, const int32_t** count, const int32_t** ids,
                                  const float** last_pts, const int32_t** lens, const float** hist)
{
    if (!t) return TBDK_EINVAL;
    const KltState& st = t->st[t->sidx];
    if (count) *count = t->count;
    if (ids) *ids = st.ids;
    if (last_pts) *last_pts = reinterpret_cast<const float*>(st.last);
    if (lens) *lens = st.lens;
    if (hist) *hist = reinterpret_cast<const float*>(st.hist);
    return TBDK_OK;
}

int tbdk_mask_circles_u8(tbdk_ctx* ctx, uint8_t* mask, int width, int height, int pitch, const float* pts,
                         const int32_t* count_dev, int n, int radius, int value, void* stream)
{
    if (!ctx || n < 0 || radius < 0 || radius > kKltMaxRadius || value < 0 || value > 255) return TBDK_EINVAL;
    if (n == 0) return TBDK_OK;
    if (!mask || !pts || width <= 0 || height <= 0 || pitch < width) return TBDK_EINVAL;
    uint8_t hw[kKltMaxRadius + 1];
    circle_half_widths(radius, hw);
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rec = timing_begin(ctx, "klt_mask", s);
    const hipError_t e = launch_mask_circles(mask, width, height, pitch, pts, count_dev, n, radius, value, hw, s);
    timing_end(ctx, rec, s);
    return map_status(e);
}

}  // extern "C"
