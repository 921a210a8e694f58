// hog.hip — HOG people detector: the sample's detection step,
// cv::cuda::HOG::detectMultiScale (cudaobjdetect/src/hog.cpp), computed with the
// CPU cv::HOGDescriptor's numerics (objdetect/src/hog.cpp) so that the results
// equal the CPU detector's.  Per pyramid level:
//
//   hog_resize   resize INTER_LINEAR_EXACT (8.8 fixed point, resize.cpp:732-891)
//   hog_grad     computeGradient: gamma LUT, REFLECT_101, the 3-channel pick,
//                magnitude / fastAtan (AVX2 dispatch form), bin split (hog.cpp:239-550)
//   hog_block    one thread per (block, cell): that cell's histogram summed in the
//                reference's pixData order; the block's L2-Hys normalization in
//                its 4-lane order via LDS (hog.cpp:860-1248)
//   hog_window   one thread per window: the SVM dot product in the 4-lane float
//                order, block by block into a double (hog.cpp:1694-1766); hits are
//                appended with an atomic counter
//
// The host then sorts the hits into window order, scales them to rects, and
// groups and clips them (groupRectangles, hog.cpp:3783-3861; clipObjects).
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "tbdk_internal.hpp"

namespace tbdk {

constexpr int kHogMaxBins = 32;
constexpr int kHogMaxCells = 16;

// one pyramid level of a batched detectMultiScale: its region of the
// multi-level block buffer and its first workgroup in the batched window launch
struct HogLevelEnt {
    int64_t boff;        // floats
    int gpitch, qpitch;  // floats, bytes
    int nbx, nby, nwx, nwy;
    int level, w0;
};

struct HogScratch {
    uint8_t* level = nullptr;  // resized level image (u8, cn)
    float* grad = nullptr;     // 2 floats per pixel
    uint8_t* qangle = nullptr; // 2 bytes per pixel
    float* blocks = nullptr;
    float* svm = nullptr;
    int4* cells = nullptr;     // per-cell pixel lists: (di, dj, weight bits, 0)
    int* hits = nullptr;       // [0] count, then (level, x, y) int triples
    double* scores = nullptr;
    int64_t cap_px = 0, cap_blocks = 0, cap_svm = 0, cap_cells = 0, cap_hits = 0;
    // detectMultiScale: every level's blocks at once (one window launch for
    // all levels)
    float* mblocks = nullptr;
    HogLevelEnt* lvtab = nullptr;
    int64_t cap_mblocks = 0, cap_lvtab = 0;
    hipStream_t stream = nullptr;  // stream of the last call that used this scratch
    bool used = false;
    int block_tiled = 1;  // tbdk_ctx_set_option("hog_block_tiled"), copied by reserve()
    // host copies of what `cells` and `svm` hold (empty: unknown), so repeated
    // calls with the same detector skip the uploads and their stream sync
    std::vector<int4> cells_host;
    std::vector<float> svm_host;
    // detectMultiScale's level lanes: level k's resize -> gradient -> block
    // chain runs on lane k % nlanes; lane 0 is the caller's stream with the
    // buffers above, lanes 1.. own a stream and a level image / gradient set
    static constexpr int kMaxLanes = 4;
    hipStream_t lane_stream[kMaxLanes] = {};
    hipEvent_t fork = nullptr, join[kMaxLanes] = {};
    uint8_t* lane_level[kMaxLanes] = {};
    float* lane_grad[kMaxLanes] = {};
    uint8_t* lane_qangle[kMaxLanes] = {};
    int64_t lane_cap_px[kMaxLanes] = {};
    int fill = -1;  // the context's alloc_fill byte, copied by reserve()
};

// The scratch (cell table, level image, gradients, blocks, hits) is rewritten by
// every call. A call on another stream than the previous one first drains that
// stream, so kernels still reading the old contents never see the new ones.
static hipError_t claim(HogScratch* S, hipStream_t s)
{
    hipError_t e = hipSuccess;
    if (S->used && S->stream != s) e = hipStreamSynchronize(S->stream);
    S->stream = s;
    S->used = true;
    return e;
}

__device__ __forceinline__ int hog_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - p - 2;
    return p;
}

// ---------------------------------------------------------------------------
// resize INTER_LINEAR_EXACT (u8): interpolationLinear::getCoeffs (resize.cpp:737-761)
// per output coordinate; ufixedpoint16 horizontal, ufixedpoint32 vertical.

struct ExactCoef {
    int ofs, c0, c1;
    int mode;  // 0 inside, 1 left/top (value of 0), 2 right/bottom (value of size - 1)
};

__device__ __forceinline__ ExactCoef exact_coef(int d, double scale, int ssize)
{
    ExactCoef r;
    const double f = scale * ((double)d + 0.5) - 0.5;
    const int iv = (int)floor(f);
    r.ofs = 0, r.c0 = 256, r.c1 = 0, r.mode = 1;
    if (iv >= 0 && ssize > 1) {
        if (iv < ssize - 1) {
            r.mode = 0;
            r.ofs = iv;
            r.c1 = (int)rint((f - iv) * 256.0);
            r.c0 = 256 - r.c1;
        } else {
            r.mode = 2;
        }
    }
    return r;
}

// the reference clamps each side at the first/last index whose interpolation
// leaves the image (minofst/maxofst), then uses the edge value from there on
struct ExactAxis {
    double scale;
    int ssize, dmin, dmax;
};

__device__ __forceinline__ uint32_t exact_h(const uint8_t* S, int dx, const ExactCoef& cx, const ExactAxis& ax,
                                            int cn, int c)
{
    if (dx < ax.dmin) return (uint32_t)S[c] << 8;
    if (dx >= ax.dmax) return (uint32_t)S[(ax.ssize - 1) * cn + c] << 8;
    return (uint32_t)cx.c0 * S[cx.ofs * cn + c] + (uint32_t)cx.c1 * S[(cx.ofs + 1) * cn + c];
}

__global__ __launch_bounds__(256) void hog_resize_kernel(const uint8_t* src, int sw, int sh, int spitch, int cn,
                                                         uint8_t* dst, int dw, int dh, int dpitch, ExactAxis ax,
                                                         ExactAxis ay)
{
    const int dx = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y;
    if (dx >= dw) return;
    const ExactCoef cx = exact_coef(dx, ax.scale, sw);
    uint8_t* D = dst + (size_t)dy * dpitch + (size_t)dx * cn;
    if (dy < ay.dmin || dy >= ay.dmax) {
        const uint8_t* S = src + (size_t)(dy < ay.dmin ? 0 : sh - 1) * spitch;
        for (int c = 0; c < cn; ++c) D[c] = (uint8_t)((exact_h(S, dx, cx, ax, cn, c) + 128) >> 8);
        return;
    }
    const ExactCoef cy = exact_coef(dy, ay.scale, sh);
    const uint8_t* S0 = src + (size_t)cy.ofs * spitch;
    const uint8_t* S1 = S0 + spitch;
    for (int c = 0; c < cn; ++c) {
        const uint32_t v = exact_h(S0, dx, cx, ax, cn, c) * (uint32_t)cy.c0 + exact_h(S1, dx, cx, ax, cn, c) * (uint32_t)cy.c1;
        D[c] = (uint8_t)((v + 32768) >> 16);
    }
}

// host: minofst / maxofst of interpolationLinear for one axis
static ExactAxis exact_axis(int ssize, int dsize)
{
    ExactAxis a;
    a.scale = 1. / ((double)dsize / ssize);
    a.ssize = ssize;
    a.dmin = 0;
    a.dmax = dsize;
    for (int d = 0; d < dsize; ++d) {
        const double f = a.scale * ((double)d + 0.5) - 0.5;
        const int iv = (int)std::floor(f);
        if (iv >= 0 && ssize > 1) {
            if (iv >= ssize - 1) a.dmax = std::min(a.dmax, d);
        } else {
            a.dmin = std::max(a.dmin, d + 1);
        }
    }
    return a;
}

// ---------------------------------------------------------------------------
// computeGradient

struct HogGradArgs {
    const uint8_t* img;
    int w, h, pitch, cn;
    float* grad;
    int gpitch;  // floats
    uint8_t* qangle;
    int qpitch;  // bytes
    int nbins;
    float angle_scale;
    // cartToPolar hands each row to magnitude32f / fastAtan32f in chunks of
    // BLOCK_SIZE = 1024 (core/src/mathfuncs.cpp:285-298, precomp.hpp:269); a chunk
    // shorter than 2 x 8 lanes takes the scalar forms (mathfuncs_core.simd.hpp:131-138,
    // 202-207), so the form is chosen per pixel from its chunk's length
    int vec_min_len;
    float lut[256];
};

__device__ __forceinline__ float hog_fast_atan(float y, float x, bool vec)
{
    const float p1 = 0.9997878412794807f * (float)(180 / M_PI);
    const float p3 = -0.3258083974640975f * (float)(180 / M_PI);
    const float p5 = 0.1555786518463281f * (float)(180 / M_PI);
    const float p7 = -0.04432655554792128f * (float)(180 / M_PI);
    const float ax = fabsf(x), ay = fabsf(y);
    // v_atan_f32::compute (mathfuncs_core.simd.hpp:92-103), FMA form.  The scalar
    // atan_f32 (:50-71) of the same AVX2 unit is FMA-contracted by gcc: the same
    // chain, and "90 - poly * c" as one fused multiply-subtract, the only difference
    const float c = fminf(ax, ay) / (fmaxf(ax, ay) + (float)DBL_EPSILON);
    const float cc = c * c;
    const float poly = fmaf(fmaf(fmaf(cc, p7, p5), cc, p3), cc, p1);
    float a;
    if (ax >= ay) a = poly * c;
    else if (vec) a = 90.f - poly * c;
    else a = fmaf(-c, poly, 90.f);
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a * (float)(M_PI / 180);
}

__global__ __launch_bounds__(256) void hog_grad_kernel(HogGradArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.w) return;
    const uint8_t* P = a.img + (size_t)y * a.pitch;
    const uint8_t* Pp = a.img + (size_t)hog_reflect101(y - 1, a.h) * a.pitch;
    const uint8_t* Pn = a.img + (size_t)hog_reflect101(y + 1, a.h) * a.pitch;
    const int xl = hog_reflect101(x - 1, a.w), xr = hog_reflect101(x + 1, a.w);
    float dx, dy;
    if (a.cn == 1) {
        dx = a.lut[P[xr]] - a.lut[P[xl]];
        dy = a.lut[Pn[x]] - a.lut[Pp[x]];
    } else {
        float ddx[3], ddy[3], mag[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ddx[c] = a.lut[P[xr * a.cn + c]] - a.lut[P[xl * a.cn + c]];
            ddy[c] = a.lut[Pn[x * a.cn + c]] - a.lut[Pp[x * a.cn + c]];
            mag[c] = ddx[c] * ddx[c] + ddy[c] * ddy[c];
        }
        int k;
        if (x < (a.w & ~3)) {  // SSE2 body (hog.cpp:397-403)
            k = mag[2] > mag[1] ? 2 : 1;
            if (!(fmaxf(mag[2], mag[1]) > mag[0])) k = 0;
        } else {  // scalar tail (hog.cpp:455-477)
            k = 2;
            if (mag[k] < mag[1]) k = 1;
            if (mag[k] < mag[0]) k = 0;
        }
        dx = k == 0 ? ddx[0] : k == 1 ? ddx[1] : ddx[2];
        dy = k == 0 ? ddy[0] : k == 1 ? ddy[1] : ddy[2];
    }
    const int vec = a.w - (x & ~1023) >= a.vec_min_len;  // length of x's 1024-chunk >= 16
    const float m = sqrtf(fmaf(dx, dx, dy * dy));  // both forms: the scalar one is contracted the same way
    float ang = hog_fast_atan(dy, dx, vec) * a.angle_scale - 0.5f;
    int hidx = (int)floorf(ang);
    ang -= hidx;
    *reinterpret_cast<float2*>(a.grad + (size_t)y * a.gpitch + 2 * x) = make_float2(m * (1.f - ang), m * ang);
    if (hidx < 0) hidx += a.nbins;
    else if (hidx >= a.nbins) hidx -= a.nbins;
    const int h1 = hidx + 1 < a.nbins ? hidx + 1 : 0;
    *reinterpret_cast<uchar2*>(a.qangle + (size_t)y * a.qpitch + 2 * x) = make_uchar2((uint8_t)hidx, (uint8_t)h1);
}

// ---------------------------------------------------------------------------
// block histograms

struct HogBlockArgs {
    const float* grad;
    int gpitch;  // floats
    const uint8_t* qangle;
    int qpitch;
    int nbx, nby, csx, csy;
    int ncells, nbins, hsz;
    const int4* cells;  // ncells lists of `cell_cap` entries
    int cell_cap;
    int cell_len[kHogMaxCells];
    float thresh;
    float* blocks;
};

// the level of workgroup wg of the batched window launch
__device__ __forceinline__ int hog_level_of(const HogLevelEnt* lv, int nlv, int wg)
{
    int L = 0;
    while (L + 1 < nlv && lv[L + 1].w0 <= wg) ++L;
    return L;
}

// Each thread sums its cell's bins straight into the block's LDS histogram
// (the reference's read-both-then-write update, hog.cpp:909-911); then every
// thread of the block computes the same L2-Hys scales in normalizeBlockHistogram's
// 4-lane order and writes its own bins.
__global__ __launch_bounds__(256) void hog_block_kernel(HogBlockArgs a)
{
    extern __shared__ float lds[];
    const int per_wg = 256 / a.ncells;
    const int lb = threadIdx.x / a.ncells, cell = threadIdx.x - lb * a.ncells;
    const int nbx = a.nbx, nby = a.nby;
    const float* grad = a.grad;
    const uint8_t* qangle = a.qangle;
    const int gpitch = a.gpitch, qpitch = a.qpitch;
    float* blocks = a.blocks;
    const int b = blockIdx.x * per_wg + lb;
    const bool live = lb < per_wg && b < nbx * nby;
    float* H = lds + lb * a.hsz;
    float* hs = H + cell * a.nbins;
    if (live) {
        for (int i = 0; i < a.nbins; ++i) hs[i] = 0.f;
        const int by = b / nbx, bx = b - by * nbx;
        const int x0 = bx * a.csx, y0 = by * a.csy;
        const int4* L = a.cells + (size_t)cell * a.cell_cap;
        const int n = a.cell_len[cell];
        for (int k = 0; k < n; ++k) {
            const int4 e = L[k];
            const int yy = y0 + e.x, xx = x0 + e.y;
            const float2 g = *reinterpret_cast<const float2*>(grad + (size_t)yy * gpitch + 2 * xx);
            const uchar2 q = *reinterpret_cast<const uchar2*>(qangle + (size_t)yy * qpitch + 2 * xx);
            const float w = __int_as_float(e.z);
            const float t0 = hs[q.x] + g.x * w;
            const float t1 = hs[q.y] + g.y * w;
            hs[q.x] = t0;
            hs[q.y] = t1;
        }
    }
    __syncthreads();
    if (!live) return;
    const int sz = a.hsz;
    float ps[4];
    for (int l = 0; l < 4; ++l) ps[l] = H[l] * H[l];
    int i;
    for (i = 4; i <= sz - 4; i += 4)
        for (int l = 0; l < 4; ++l) ps[l] = ps[l] + H[i + l] * H[i + l];
    float sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    for (; i < sz; ++i) sum += H[i] * H[i];
    const float scale = 1.f / (sqrtf(sum) + (float)sz * 0.1f);
    for (int l = 0; l < 4; ++l) {
        const float v = fminf(scale * H[l], a.thresh);
        ps[l] = v * v;
    }
    for (i = 4; i <= sz - 4; i += 4)
        for (int l = 0; l < 4; ++l) {
            const float v = fminf(H[i + l] * scale, a.thresh);
            ps[l] = ps[l] + v * v;
        }
    sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    for (; i < sz; ++i) {
        const float v = fminf(H[i] * scale, a.thresh);
        sum += v * v;
    }
    const float scale2 = 1.f / (sqrtf(sum) + 1e-3f);
    float* out = blocks + (size_t)b * sz + cell * a.nbins;
    for (int k = 0; k < a.nbins; ++k) out[k] = scale2 * fminf(hs[k] * scale, a.thresh);
}

// Tiled variant for 2x2-cell blocks with 9 bins (the detectors' geometry): a
// workgroup owns 16 x 4 blocks and first stages their pixel footprint (gx, gy,
// bins) and the four cells' pixData lists into LDS, coalesced, so no per-entry
// load leaves the CU (with the lists read from L2 per entry group: 0.63 instead
// of 0.50 ms per 1080p frame).  Each thread then sums its cell's entries in
// pixData order, the reference's read-both-then-write update (hog.cpp:909-911),
// into
//   BINS_LDS = true:  its own histogram in LDS, bin-major (hs[bin * 256 + tid]),
//                     so the lanes' data-dependent bins never share a bank;
//   BINS_LDS = false: nine registers, every bin adding its entry term or +0.0f
//                     (leaves a value >= +0 unchanged; b0 != b1 for nbins >= 2).
// Pixel planes are skewed by one word per csx columns, so the 16 blocks of a
// wave (csx apart) read 16 different banks: s(y, x) = y * twp + x + x / csx.
struct HogTile {
    int bw, bh;            // block size in pixels
    int ntx;               // tiles per row of blocks
    int twp, npx;          // skewed plane pitch and plane size (words)
    int off_q;             // word offset of the bin plane (u16)
    int off_h;             // word offset of the LDS histograms (BINS_LDS)
    int off_l, lstride;    // word offset of the cell lists (int2), entries per list
};
constexpr int kHogTileBx = 16, kHogTileBy = 4;

template <bool BINS_LDS>
__global__ __launch_bounds__(256) void hog_block_tile_kernel(HogBlockArgs a, HogTile t)
{
    constexpr int NB = 9, U = 4;
    extern __shared__ float lds[];
    float* gxs = lds;
    float* gys = lds + t.npx;
    uint16_t* qs = reinterpret_cast<uint16_t*>(lds + t.off_q);
    float* hs = lds + t.off_h + threadIdx.x;
    int2* lst = reinterpret_cast<int2*>(lds + t.off_l);
    const int tid = threadIdx.x, csx = a.csx, csy = a.csy;
    const int tby = blockIdx.x / t.ntx, tbx = blockIdx.x - tby * t.ntx;
    const int bx0 = tbx * kHogTileBx, by0 = tby * kHogTileBy;
    const int px0 = bx0 * csx, py0 = by0 * csy;
    const int tw = (min(bx0 + kHogTileBx, a.nbx) - 1 - bx0) * csx + t.bw;
    const int th = (min(by0 + kHogTileBy, a.nby) - 1 - by0) * csy + t.bh;
    // the footprint, one wave per row, lanes along x
    for (int y = tid >> 6; y < th; y += 4) {
        const float* gr = a.grad + (size_t)(py0 + y) * a.gpitch + 2 * px0;
        const uint16_t* qr = reinterpret_cast<const uint16_t*>(a.qangle + (size_t)(py0 + y) * a.qpitch) + px0;
        for (int x = tid & 63; x < tw; x += 64) {
            const float2 g = *reinterpret_cast<const float2*>(gr + 2 * x);
            const int s = y * t.twp + x + x / csx;
            gxs[s] = g.x;
            gys[s] = g.y;
            qs[s] = qr[x];
        }
    }
    // the four cell lists as (skewed offset, weight bits)
    for (int i = tid; i < 4 * t.lstride; i += 256) {
        const int c = i / t.lstride, k = i - c * t.lstride;
        if (k < a.cell_cap) {
            const int4 e = a.cells[(size_t)c * a.cell_cap + k];
            lst[i] = make_int2(e.w, e.z);
        }
    }
    if (BINS_LDS)
        for (int i = 0; i < NB; ++i) hs[i * 256] = 0.f;
    __syncthreads();
    const int lb = tid >> 2, cell = tid & 3;
    const int lbx = lb & (kHogTileBx - 1), lby = lb / kHogTileBx;
    const int bx = bx0 + lbx, by = by0 + lby;
    const bool live = bx < a.nbx && by < a.nby;
    float h[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) h[i] = 0.f;
    if (live) {
        const int base = lby * csy * t.twp + lbx * csx + lbx;
        const int2* L = lst + cell * t.lstride;
        const int n = cell == 0 ? a.cell_len[0] : cell == 1 ? a.cell_len[1] : cell == 2 ? a.cell_len[2] : a.cell_len[3];
        for (int k = 0; k < n; k += U) {
            // U entries' pixels read ahead of their (ordered) updates
            uint32_t q[U];
            float a0[U], a1[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int2 e = L[min(k + u, n - 1)];
                const int s = base + e.x;
                const float w = __int_as_float(e.y);
                q[u] = qs[s];
                a0[u] = gxs[s] * w;
                a1[u] = gys[s] * w;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (k + u >= n) break;
                const uint32_t q0 = q[u] & 0xffu, q1 = q[u] >> 8;
                if (BINS_LDS) {
                    const float t0 = hs[q0 * 256] + a0[u];
                    const float t1 = hs[q1 * 256] + a1[u];
                    hs[q0 * 256] = t0;
                    hs[q1 * 256] = t1;
                } else {
#pragma unroll
                    for (int i = 0; i < NB; ++i)
                        h[i] = h[i] + (q0 == (uint32_t)i ? a0[u] : (q1 == (uint32_t)i ? a1[u] : 0.f));
                }
            }
        }
    }
    if (BINS_LDS)
#pragma unroll
        for (int i = 0; i < NB; ++i) h[i] = hs[i * 256];
    __syncthreads();  // the pixel planes become the blocks' histograms
    const int sz = 4 * NB;
    float* H = lds + lb * sz;
#pragma unroll
    for (int i = 0; i < NB; ++i) H[cell * NB + i] = h[i];
    __syncthreads();
    if (!live) return;
    // normalizeBlockHistogram, as in hog_block_kernel (sz = 36: nine 4-lane steps)
    float ps[4];
    for (int l = 0; l < 4; ++l) ps[l] = H[l] * H[l];
    for (int i = 4; i <= sz - 4; i += 4)
        for (int l = 0; l < 4; ++l) ps[l] = ps[l] + H[i + l] * H[i + l];
    float sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    const float scale = 1.f / (sqrtf(sum) + (float)sz * 0.1f);
    for (int l = 0; l < 4; ++l) {
        const float v = fminf(scale * H[l], a.thresh);
        ps[l] = v * v;
    }
    for (int i = 4; i <= sz - 4; i += 4)
        for (int l = 0; l < 4; ++l) {
            const float v = fminf(H[i + l] * scale, a.thresh);
            ps[l] = ps[l] + v * v;
        }
    sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    const float scale2 = 1.f / (sqrtf(sum) + 1e-3f);
    float* out = a.blocks + ((size_t)by * a.nbx + bx) * sz + cell * NB;
#pragma unroll
    for (int k = 0; k < NB; ++k) out[k] = scale2 * fminf(h[k] * scale, a.thresh);
}

// ---------------------------------------------------------------------------
// windows

struct HogWinArgs {
    const float* blocks;
    const float* svm;
    int nbx, csx, csy;
    int wbx, wby, bsx, bsy, hsz;
    int nwx, nwy, wsx, wsy;
    double rho, hit;
    int level;
    int* hits;  // [0] count, then triples
    double* scores;
    int cap;
    const HogLevelEnt* lv;  // nlv > 0: all levels in one launch (blocks is the multi-level buffer)
    int nlv;
};

// One wave per window, one lane per block (blocks x-major as blockData): each
// lane forms its block's contribution exactly as the reference's loop body
// (float 4-lane dot, then double t0 + t1, then the tail products), and lane 0
// adds them to rho in block order (hog.cpp:1709-1760).
constexpr int kHogWinPerWg = 4;

__global__ __launch_bounds__(256) void hog_window_kernel(HogWinArgs a)
{
    extern __shared__ double wl[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int wg = blockIdx.x, nwx = a.nwx, nwy = a.nwy, nbx = a.nbx, level = a.level;
    const float* blocks = a.blocks;
    if (a.nlv > 0) {
        const HogLevelEnt& e = a.lv[hog_level_of(a.lv, a.nlv, wg)];
        wg -= e.w0;
        nwx = e.nwx, nwy = e.nwy, nbx = e.nbx, level = e.level;
        blocks += e.boff;
    }
    const int t = wg * kHogWinPerWg + wave;
    const int nblk = a.wbx * a.wby, tail = a.hsz & 3;
    double* main_v = wl + (size_t)wave * nblk * 4;  // per block: main + up to 3 tail products
    const bool live = t < nwx * nwy;
    int x0 = 0, y0 = 0;
    if (live) {
        const int wy = t / nwx, wx = t - wy * nwx;
        x0 = wx * a.wsx, y0 = wy * a.wsy;
        for (int k = lane; k < nblk; k += 64) {
            const int j = k / a.wby, i = k - j * a.wby;
            const int bx = (x0 + j * a.bsx) / a.csx, by = (y0 + i * a.bsy) / a.csy;
            const float* v = blocks + ((size_t)by * nbx + bx) * a.hsz;
            const float* sv = a.svm + (size_t)k * a.hsz;
            float ps[4];
            int q;
            if (a.hsz == 36) {
                // the detectors' 2x2x9 blocks: nine 16-byte loads of each operand,
                // all in flight at once (both rows start 144-byte aligned)
                const float4* v4 = reinterpret_cast<const float4*>(v);
                const float4* s4 = reinterpret_cast<const float4*>(sv);
                float4 x[9], y[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) x[i] = v4[i], y[i] = s4[i];
                ps[0] = y[0].x * x[0].x, ps[1] = y[0].y * x[0].y, ps[2] = y[0].z * x[0].z, ps[3] = y[0].w * x[0].w;
#pragma unroll
                for (int i = 1; i < 9; ++i) {
                    ps[0] = ps[0] + x[i].x * y[i].x;
                    ps[1] = ps[1] + x[i].y * y[i].y;
                    ps[2] = ps[2] + x[i].z * y[i].z;
                    ps[3] = ps[3] + x[i].w * y[i].w;
                }
                q = 36;
            } else {
                for (int l = 0; l < 4; ++l) ps[l] = sv[l] * v[l];
                for (q = 4; q <= a.hsz - 4; q += 4)
                    for (int l = 0; l < 4; ++l) ps[l] = ps[l] + v[q + l] * sv[q + l];
            }
            const double t0 = ps[0] + ps[1], t1 = ps[2] + ps[3];
            main_v[4 * k] = t0 + t1;
            for (int r = 0; r < tail; ++r, ++q) main_v[4 * k + 1 + r] = (double)(v[q] * sv[q]);
        }
    }
    __syncthreads();
    if (!live || lane != 0) return;
    double s = a.rho;
    for (int k = 0; k < nblk; ++k) {
        s += main_v[4 * k];
        for (int r = 0; r < tail; ++r) s += main_v[4 * k + 1 + r];
    }
    if (s >= a.hit) {
        const int slot = atomicAdd(a.hits, 1);
        if (slot < a.cap) {
            a.hits[1 + 3 * slot] = level;
            a.hits[2 + 3 * slot] = x0;
            a.hits[3 + 3 * slot] = y0;
            a.scores[slot] = s;
        }
    }
}

// Batched window pass over 36-float blocks, one row of kHogWinTile windows per
// workgroup: the blocks those windows share (their union: 20 x 11 for the
// 48 x 96 detector, 22 x 15 for the 64 x 128 default, instead of 16 x 55 /
// 16 x 105 block reads) and the detector are staged in LDS
// once, coalesced; each wave then scores every fourth window exactly as
// hog_window_kernel does (same products, sums and order), one lane per window
// for the serial sums.
constexpr int kHogWinTile = 16;

struct HogWinTile {
    int cols, rows;        // staged block columns / rows (full tile)
    int cstep, rstep;      // window step in block columns / rows (win stride / cell grid)
    int bstepx, bstepy;    // block step inside a window (block stride / cell grid)
    int off_svm, off_d;    // float offsets of the staged detector and the per-wave doubles
};

__global__ __launch_bounds__(256) void hog_window_tile_kernel(HogWinArgs a, HogWinTile t)
{
    extern __shared__ float wt[];
    float4* B4 = reinterpret_cast<float4*>(wt);
    float4* S4 = reinterpret_cast<float4*>(wt + t.off_svm);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const HogLevelEnt& e = a.lv[hog_level_of(a.lv, a.nlv, blockIdx.x)];
    const int wg = blockIdx.x - e.w0, nwx = e.nwx, nbx = e.nbx;
    const float* blocks = a.blocks + e.boff;
    const int per_row = (nwx + kHogWinTile - 1) / kHogWinTile;
    const int wy = wg / per_row, wx0 = (wg - wy * per_row) * kHogWinTile;
    const int nwin = min(kHogWinTile, nwx - wx0);
    const int bc0 = wx0 * t.cstep, br0 = wy * t.rstep;
    const int cols = (nwin - 1) * t.cstep + (a.wbx - 1) * t.bstepx + 1;
    const int nblk = a.wbx * a.wby;
    for (int idx = tid; idx < t.rows * cols * 9; idx += 256) {
        const int r = idx / (cols * 9), rem = idx - r * cols * 9, c = rem / 9, q = rem - c * 9;
        B4[(r * t.cols + c) * 9 + q] =
            reinterpret_cast<const float4*>(blocks + ((size_t)(br0 + r) * nbx + bc0 + c) * 36)[q];
    }
    for (int idx = tid; idx < nblk * 9; idx += 256) S4[idx] = reinterpret_cast<const float4*>(a.svm)[idx];
    // wave `wave` scores windows wave, wave + 4, ... (kHogWinTile / 4 rounds); the
    // block terms of all its windows first, then one lane per window sums them
    double* main_v = reinterpret_cast<double*>(wt + t.off_d) + wave * (kHogWinTile / 4) * nblk;
    __syncthreads();  // staging done
    for (int r = 0; r < kHogWinTile / 4; ++r) {
        const int w = wave + 4 * r;
        if (w >= nwin) break;
        for (int k = lane; k < nblk; k += 64) {
            const int j = k / a.wby, i = k - j * a.wby;
            const float4* v4 = B4 + ((i * t.bstepy) * t.cols + w * t.cstep + j * t.bstepx) * 9;
            const float4* s4 = S4 + k * 9;
            float4 x[9], y[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) x[q] = v4[q], y[q] = s4[q];
            float ps[4];
            ps[0] = y[0].x * x[0].x, ps[1] = y[0].y * x[0].y, ps[2] = y[0].z * x[0].z, ps[3] = y[0].w * x[0].w;
#pragma unroll
            for (int q = 1; q < 9; ++q) {
                ps[0] = ps[0] + x[q].x * y[q].x;
                ps[1] = ps[1] + x[q].y * y[q].y;
                ps[2] = ps[2] + x[q].z * y[q].z;
                ps[3] = ps[3] + x[q].w * y[q].w;
            }
            const double t0 = ps[0] + ps[1], t1 = ps[2] + ps[3];
            main_v[r * nblk + k] = t0 + t1;
        }
    }
    __syncthreads();
    const int w = wave + 4 * lane;
    if (lane < kHogWinTile / 4 && w < nwin) {
        const double* m = main_v + lane * nblk;
        double sc = a.rho;
        for (int k = 0; k < nblk; ++k) sc += m[k];
        if (sc >= a.hit) {
            const int slot = atomicAdd(a.hits, 1);
            if (slot < a.cap) {
                a.hits[1 + 3 * slot] = e.level;
                a.hits[2 + 3 * slot] = (wx0 + w) * a.wsx;
                a.hits[3 + 3 * slot] = wy * a.wsy;
                a.scores[slot] = sc;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host side

static int cv_round_d(double v) { return (int)std::lrint(v); }

static int gcd_i(int a, int b)
{
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

static int hog_check(const tbdk_hog_params* p)
{
    if (!p) return TBDK_EINVAL;
    if (p->win_w <= 0 || p->win_h <= 0 || p->block_w <= 0 || p->block_h <= 0 || p->cell_w <= 0 || p->cell_h <= 0)
        return TBDK_EINVAL;
    if (p->block_stride_x <= 0 || p->block_stride_y <= 0 || p->win_stride_x <= 0 || p->win_stride_y <= 0)
        return TBDK_EINVAL;
    // HOG_Impl's asserts (cudaobjdetect/src/hog.cpp:252-256)
    if ((p->win_w - p->block_w) % p->block_stride_x || (p->win_h - p->block_h) % p->block_stride_y) return TBDK_EINVAL;
    if (p->block_w % p->cell_w || p->block_h % p->cell_h) return TBDK_EINVAL;
    if (p->block_w > p->win_w || p->block_h > p->win_h) return TBDK_EINVAL;
    const int ncells = (p->block_w / p->cell_w) * (p->block_h / p->cell_h);
    if (p->nbins < 2 || p->nbins > kHogMaxBins || ncells > kHogMaxCells) return TBDK_EINVAL;
    const int64_t wblocks = (int64_t)((p->win_w - p->block_w) / p->block_stride_x + 1) *
                            ((p->win_h - p->block_h) / p->block_stride_y + 1);
    if (wblocks * 4 * kHogWinPerWg * (int64_t)sizeof(double) > 64 * 1024) return TBDK_EINVAL;  // window LDS
    if (ncells * p->nbins < 4) return TBDK_EINVAL;  // normalizeBlockHistogram reads 4 lanes
    if (p->block_w * p->block_h > 64 * 64) return TBDK_EINVAL;
    return TBDK_OK;
}

static int hist_size(const tbdk_hog_params* p)
{
    return (p->block_w / p->cell_w) * (p->block_h / p->cell_h) * p->nbins;
}

static int descriptor_size(const tbdk_hog_params* p)
{
    return hist_size(p) * ((p->win_w - p->block_w) / p->block_stride_x + 1) *
           ((p->win_h - p->block_h) / p->block_stride_y + 1);
}

// HOGCache::init's pixData (hog.cpp:656-848), split per cell in pixData order:
// entry = (di, dj, gradWeight * histWeights[k]) for the k whose histOfs is the cell
static void cell_lists(const tbdk_hog_params* p, std::vector<std::vector<int4>>& lists)
{
    const int bw = p->block_w, bh = p->block_h, ncx = bw / p->cell_w, ncy = bh / p->cell_h;
    const float sigma = (float)(p->win_sigma > 0 ? p->win_sigma : (bw + bh) / 8.);
    const float scale = 1.f / (sigma * sigma * 2);
    const float fbh = bh * 0.5f, fbw = bw * 0.5f;
    std::vector<float> di(bh), dj(bw);
    for (int i = 0; i < bh; i++) {
        di[i] = i - fbh;
        di[i] *= di[i];
    }
    for (int j = 0; j < bw; j++) {
        dj[j] = j - fbw;
        dj[j] *= dj[j];
    }
    struct Pix {
        int di, dj, n, cell[4];
        float hw[4], gw;
    };
    std::vector<Pix> g1, g2, g4;
    for (int j = 0; j < bw; j++)
        for (int i = 0; i < bh; i++) {
            Pix d{};
            float cellX = (j + 0.5f) / p->cell_w - 0.5f;
            float cellY = (i + 0.5f) / p->cell_h - 0.5f;
            const int icx0 = (int)std::floor(cellX), icy0 = (int)std::floor(cellY);
            int icx1 = icx0 + 1, icy1 = icy0 + 1;
            cellX -= icx0;
            cellY -= icy0;
            const bool x0ok = (unsigned)icx0 < (unsigned)ncx, x1ok = (unsigned)icx1 < (unsigned)ncx;
            const bool y0ok = (unsigned)icy0 < (unsigned)ncy, y1ok = (unsigned)icy1 < (unsigned)ncy;
            std::vector<Pix>* grp;
            if (x0ok && x1ok) {
                if (y0ok && y1ok) {
                    grp = &g4;
                    d.n = 4;
                    d.cell[0] = icx0 * ncy + icy0, d.hw[0] = (1.f - cellX) * (1.f - cellY);
                    d.cell[1] = icx1 * ncy + icy0, d.hw[1] = cellX * (1.f - cellY);
                    d.cell[2] = icx0 * ncy + icy1, d.hw[2] = (1.f - cellX) * cellY;
                    d.cell[3] = icx1 * ncy + icy1, d.hw[3] = cellX * cellY;
                } else {
                    grp = &g2;
                    d.n = 2;
                    if (y0ok) {
                        icy1 = icy0;
                        cellY = 1.f - cellY;
                    }
                    d.cell[0] = icx0 * ncy + icy1, d.hw[0] = (1.f - cellX) * cellY;
                    d.cell[1] = icx1 * ncy + icy1, d.hw[1] = cellX * cellY;
                }
            } else {
                if (x0ok) {
                    icx1 = icx0;
                    cellX = 1.f - cellX;
                }
                if (y0ok && y1ok) {
                    grp = &g2;
                    d.n = 2;
                    d.cell[0] = icx1 * ncy + icy0, d.hw[0] = cellX * (1.f - cellY);
                    d.cell[1] = icx1 * ncy + icy1, d.hw[1] = cellX * cellY;
                } else {
                    grp = &g1;
                    d.n = 1;
                    if (y0ok) {
                        icy1 = icy0;
                        cellY = 1.f - cellY;
                    }
                    d.cell[0] = icx1 * ncy + icy1, d.hw[0] = cellX * cellY;
                }
            }
            d.di = i, d.dj = j;
            d.gw = std::exp(-(di[i] + dj[j]) * scale);
            grp->push_back(d);
        }
    lists.assign(ncx * ncy, {});
    for (const std::vector<Pix>* grp : {&g1, &g2, &g4})
        for (const Pix& d : *grp)
            for (int e = 0; e < d.n; e++) {
                float w = d.gw * d.hw[e];
                int wb;
                std::memcpy(&wb, &w, 4);
                lists[d.cell[e]].push_back(make_int4(d.di, d.dj, wb, 0));
            }
}

template <typename T>
static int grow(T** p, int64_t& cap, int64_t need, int fill)
{
    if (need <= cap) return TBDK_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    cap = 0;
    if (dev_alloc(p, sizeof(T) * (size_t)need, fill) != hipSuccess) return TBDK_ENOMEM;
    cap = need;
    return TBDK_OK;
}

struct HogPlan {
    int hsz, ncells, csx, csy, wbx, wby, dsize;
    std::vector<std::vector<int4>> lists;  // entry .w: offset in hog_block_tile_kernel's skewed tile
    int cell_cap;
    int tile_twp;
};

static void make_plan(const tbdk_hog_params* p, HogPlan& pl)
{
    pl.hsz = hist_size(p);
    pl.ncells = (p->block_w / p->cell_w) * (p->block_h / p->cell_h);
    pl.csx = gcd_i(p->win_stride_x, p->block_stride_x);
    pl.csy = gcd_i(p->win_stride_y, p->block_stride_y);
    pl.wbx = (p->win_w - p->block_w) / p->block_stride_x + 1;
    pl.wby = (p->win_h - p->block_h) / p->block_stride_y + 1;
    pl.dsize = descriptor_size(p);
    cell_lists(p, pl.lists);
    const int tw = (kHogTileBx - 1) * pl.csx + p->block_w;
    pl.tile_twp = tw + (tw - 1) / pl.csx + 1;
    for (auto& l : pl.lists)
        for (int4& e : l) e.w = e.x * pl.tile_twp + e.y + e.y / pl.csx;
    pl.cell_cap = 0;
    for (auto& l : pl.lists) pl.cell_cap = std::max(pl.cell_cap, (int)l.size());
}

static bool same_int4(const std::vector<int4>& a, const std::vector<int4>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(int4) * a.size()) == 0;
}

static hipError_t upload_plan(HogScratch* S, const HogPlan& pl, hipStream_t s)
{
    std::vector<int4> flat((size_t)pl.ncells * pl.cell_cap, make_int4(0, 0, 0, 0));
    for (int c = 0; c < pl.ncells; ++c)
        std::copy(pl.lists[c].begin(), pl.lists[c].end(), flat.begin() + (size_t)c * pl.cell_cap);
    if (same_int4(flat, S->cells_host)) return hipSuccess;
    S->cells_host.clear();
    hipError_t e = hipMemcpyAsync(S->cells, flat.data(), sizeof(int4) * flat.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // `flat` is pageable and local
    if (e == hipSuccess) S->cells_host.swap(flat);
    return e;
}

static hipError_t launch_grad(const uint8_t* img, int w, int h, int pitch, int cn, const tbdk_hog_params* p,
                              float* grad, int gpitch_f, uint8_t* qa, int qpitch, hipStream_t s)
{
    HogGradArgs a;
    a.img = img, a.w = w, a.h = h, a.pitch = pitch, a.cn = cn;
    a.grad = grad, a.gpitch = gpitch_f, a.qangle = qa, a.qpitch = qpitch;
    a.nbins = p->nbins;
    a.angle_scale = p->signed_gradient ? (float)(p->nbins / (2.0 * M_PI)) : (float)(p->nbins / M_PI);
    a.vec_min_len = 16;  // chunk length from which the 8-lane forms run
    for (int i = 0; i < 256; ++i) a.lut[i] = p->gamma_correction ? std::sqrt((float)i) : (float)i;
    hipLaunchKernelGGL(hog_grad_kernel, dim3((w + 255) / 256, h), dim3(256), 0, s, a);
    return hipGetLastError();
}

// dynamic LDS of the tiled block kernels: two workgroups per CU (the default
// geometry takes 75 KB); above 64 KB the kernels opt in once per device
constexpr size_t kHogTileLds = 80 * 1024;

// the tiled window pass opts in to the whole LDS (the 64 x 128 detector's
// tile takes ~76 KB: 22 x 15 blocks, the detector and 4 waves x 4 windows of
// doubles); the limit leaves the kernel's static LDS its room
constexpr size_t kHogWinTileLds = 160 * 1024 - 1024;

static hipError_t win_lds_opt_in()
{
    static std::atomic<unsigned long long> opted{0};
    return lds_opt_in(opted, {reinterpret_cast<const void*>(&hog_window_tile_kernel)}, kHogWinTileLds);
}

static hipError_t tile_lds_opt_in()
{
    static std::atomic<unsigned long long> opted{0};
    return lds_opt_in(opted,
                      {reinterpret_cast<const void*>(&hog_block_tile_kernel<true>),
                       reinterpret_cast<const void*>(&hog_block_tile_kernel<false>)},
                      kHogTileLds);
}

static hipError_t launch_blocks(HogScratch* S, const HogPlan& pl, const tbdk_hog_params* p, const float* grad,
                                int gpitch_f, const uint8_t* qa, int qpitch, int nbx, int nby, float* blocks,
                                hipStream_t s)
{
    HogBlockArgs a;
    a.grad = grad, a.gpitch = gpitch_f, a.qangle = qa, a.qpitch = qpitch;
    a.nbx = nbx, a.nby = nby, a.csx = pl.csx, a.csy = pl.csy;
    a.ncells = pl.ncells, a.nbins = p->nbins, a.hsz = pl.hsz;
    a.cells = S->cells;
    a.cell_cap = pl.cell_cap;
    for (int c = 0; c < kHogMaxCells; ++c) a.cell_len[c] = c < pl.ncells ? (int)pl.lists[c].size() : 0;
    a.thresh = (float)p->l2hys_threshold;
    a.blocks = blocks;
    if (S->block_tiled && pl.ncells == 4 && p->nbins == 9) {
        HogTile t;
        t.bw = p->block_w, t.bh = p->block_h;
        t.ntx = (nbx + kHogTileBx - 1) / kHogTileBx;
        t.twp = pl.tile_twp;
        t.npx = ((kHogTileBy - 1) * pl.csy + t.bh) * t.twp;
        t.off_q = 2 * t.npx;
        t.off_h = t.off_q + (t.npx + 1) / 2;
        const bool bins_lds = S->block_tiled == 1;
        t.off_l = (t.off_h + (bins_lds ? 9 * 256 : 0) + 1) & ~1;
        t.lstride = (pl.cell_cap + 31) / 32 * 32 + 4;  // the four lists' heads 8 banks apart
        const size_t words = std::max<size_t>((size_t)t.off_l + 2 * 4 * (size_t)t.lstride, 64 * 36);
        if (words * sizeof(float) <= kHogTileLds) {
            const hipError_t e = tile_lds_opt_in();
            if (e != hipSuccess) return e;
            const int nty = (nby + kHogTileBy - 1) / kHogTileBy;
            const dim3 grid(t.ntx * nty);
            if (bins_lds)
                hipLaunchKernelGGL(hog_block_tile_kernel<true>, grid, dim3(256), words * sizeof(float), s, a, t);
            else
                hipLaunchKernelGGL(hog_block_tile_kernel<false>, grid, dim3(256), words * sizeof(float), s, a, t);
            return hipGetLastError();
        }
    }
    const int per_wg = 256 / pl.ncells;
    const int nb = nbx * nby;
    const dim3 grid((nb + per_wg - 1) / per_wg);
    const size_t lds = sizeof(float) * per_wg * pl.hsz;
    hipLaunchKernelGGL(hog_block_kernel, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

// one level: gradients, blocks, windows (hits appended to S->hits)
static hipError_t run_level(tbdk_ctx* ctx, HogScratch* S, const HogPlan& pl, const tbdk_hog_params* p,
                            const uint8_t* img, int w, int h, int pitch, int cn, double rho, int level, int hit_cap,
                            hipStream_t s)
{
    const int gpf = 2 * w, qp = 2 * w;
    int rec = timing_begin(ctx, "hog_grad", s);
    hipError_t e = launch_grad(img, w, h, pitch, cn, p, S->grad, gpf, S->qangle, qp, s);
    timing_end(ctx, rec, s);
    if (e != hipSuccess) return e;
    const int nbx = (w - p->block_w) / pl.csx + 1, nby = (h - p->block_h) / pl.csy + 1;
    rec = timing_begin(ctx, "hog_block", s);
    e = launch_blocks(S, pl, p, S->grad, gpf, S->qangle, qp, nbx, nby, S->blocks, s);
    timing_end(ctx, rec, s);
    if (e != hipSuccess) return e;
    HogWinArgs a;
    a.blocks = S->blocks, a.svm = S->svm;
    a.nbx = nbx, a.csx = pl.csx, a.csy = pl.csy;
    a.wbx = pl.wbx, a.wby = pl.wby, a.bsx = p->block_stride_x, a.bsy = p->block_stride_y, a.hsz = pl.hsz;
    a.nwx = (w - p->win_w) / p->win_stride_x + 1;
    a.nwy = (h - p->win_h) / p->win_stride_y + 1;
    a.wsx = p->win_stride_x, a.wsy = p->win_stride_y;
    a.rho = rho, a.hit = p->hit_threshold, a.level = level;
    a.hits = S->hits, a.scores = S->scores, a.cap = hit_cap;
    a.lv = nullptr, a.nlv = 0;
    rec = timing_begin(ctx, "hog_window", s);
    const int nwin = a.nwx * a.nwy;
    const size_t lds = sizeof(double) * 4 * kHogWinPerWg * (size_t)(pl.wbx * pl.wby);
    hipLaunchKernelGGL(hog_window_kernel, dim3((nwin + kHogWinPerWg - 1) / kHogWinPerWg), dim3(256), lds, s, a);
    timing_end(ctx, rec, s);
    return hipGetLastError();
}

static int reserve(tbdk_ctx* ctx, int w, int h, int cn, const HogPlan& pl, int svm_len, int64_t hit_cap,
                   hipStream_t s)
{
    if (!ctx->hog) ctx->hog = new (std::nothrow) HogScratch();
    HogScratch* S = ctx->hog;
    if (!S) return TBDK_ENOMEM;
    if (claim(S, s) != hipSuccess) return TBDK_EHIP;
    S->block_tiled = ctx->opt_hog_block_tiled;
    S->fill = ctx->opt_alloc_fill;
    const int64_t px = (int64_t)w * h;
    int rc = TBDK_OK;
    if (px > S->cap_px) {
        int64_t c0 = 0, c1 = 0, c2 = 0;
        if ((rc = grow(&S->level, c0, px * 4, S->fill)) || (rc = grow(&S->grad, c1, px * 2, S->fill)) ||
            (rc = grow(&S->qangle, c2, px * 2, S->fill)))
            return rc;
        S->cap_px = px;
    }
    const int64_t nblk = ((int64_t)w / pl.csx + 1) * (h / pl.csy + 1) * pl.hsz;
    if ((rc = grow(&S->blocks, S->cap_blocks, nblk, S->fill))) return rc;
    if (svm_len > S->cap_svm) S->svm_host.clear();  // reallocated below: contents unknown
    if ((rc = grow(&S->svm, S->cap_svm, svm_len, S->fill))) return rc;
    if ((int64_t)pl.ncells * pl.cell_cap > S->cap_cells) S->cells_host.clear();
    if ((rc = grow(&S->cells, S->cap_cells, (int64_t)pl.ncells * pl.cell_cap, S->fill))) return rc;
    if (hit_cap > S->cap_hits) {
        int64_t c = 0;
        if ((rc = grow(&S->hits, c, 1 + 3 * hit_cap, S->fill)) || (rc = grow(&S->scores, S->cap_hits, hit_cap, S->fill)))
            return rc;
    }
    (void)cn;
    return TBDK_OK;
}

// groupRectangles(rects, weights, groupThreshold, eps) (hog.cpp:3783-3861) with
// partition()/SimilarRects, then clipObjects (cascadedetect.cpp:1683-1710)
static int group_and_clip(std::vector<int>& r, std::vector<double>& wt, int thr, double eps, int W, int H)
{
    int n = (int)wt.size();
    if (thr > 0 && n > 0) {
        auto similar = [&](int i, int j) {
            const int* a = &r[4 * i];
            const int* b = &r[4 * j];
            const double delta = eps * (std::min(a[2], b[2]) + std::min(a[3], b[3])) * 0.5;
            return std::abs(a[0] - b[0]) <= delta && std::abs(a[1] - b[1]) <= delta &&
                   std::abs(a[0] + a[2] - b[0] - b[2]) <= delta && std::abs(a[1] + a[3] - b[1] - b[3]) <= delta;
        };
        std::vector<int> parent(n);
        std::iota(parent.begin(), parent.end(), 0);
        auto root = [&](int i) {
            while (parent[i] != i) i = parent[i] = parent[parent[i]];
            return i;
        };
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j)
                if (similar(i, j)) {
                    const int a = root(i), b = root(j);
                    if (a != b) parent[a] = b;
                }
        std::vector<int> cls(n, -1), label(n);
        int ncls = 0;
        for (int i = 0; i < n; ++i) {
            const int rt = root(i);
            if (cls[rt] < 0) cls[rt] = ncls++;
            label[i] = cls[rt];
        }
        std::vector<double> rr(4 * (size_t)ncls, 0.0), fw(ncls, -DBL_MAX);
        std::vector<int> cnt(ncls, 0), ri(4 * (size_t)ncls);
        for (int i = 0; i < n; ++i) {
            const int c = label[i];
            for (int t = 0; t < 4; ++t) rr[4 * c + t] += r[4 * i + t];
            fw[c] = std::max(fw[c], wt[i]);
            cnt[c]++;
        }
        for (int c = 0; c < ncls; ++c) {
            const double sc = 1.0 / cnt[c];
            for (int t = 0; t < 4; ++t) ri[4 * c + t] = (int)std::lrint(rr[4 * c + t] * sc);
        }
        std::vector<int> out;
        std::vector<double> ow;
        for (int i = 0; i < ncls; ++i) {
            const int* r1 = &ri[4 * i];
            const int n1 = cnt[i];
            if (n1 <= thr) continue;
            int j;
            for (j = 0; j < ncls; ++j) {
                const int n2 = cnt[j];
                if (j == i || n2 <= thr) continue;
                const int* r2 = &ri[4 * j];
                const int dx = (int)std::lrint(r2[2] * eps), dy = (int)std::lrint(r2[3] * eps);
                if (r1[0] >= r2[0] - dx && r1[1] >= r2[1] - dy && r1[0] + r1[2] <= r2[0] + r2[2] + dx &&
                    r1[1] + r1[3] <= r2[1] + r2[3] + dy && (n2 > std::max(3, n1) || n1 < 3))
                    break;
            }
            if (j == ncls) {
                out.insert(out.end(), r1, r1 + 4);
                ow.push_back(fw[i]);
            }
        }
        r.swap(out);
        wt.swap(ow);
        n = (int)wt.size();
    }
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int x0 = std::max(r[4 * i], 0), y0 = std::max(r[4 * i + 1], 0);
        const int x1 = std::min(r[4 * i] + r[4 * i + 2], W), y1 = std::min(r[4 * i + 1] + r[4 * i + 3], H);
        if (x1 <= x0 || y1 <= y0) continue;
        r[4 * m] = x0, r[4 * m + 1] = y0, r[4 * m + 2] = x1 - x0, r[4 * m + 3] = y1 - y0;
        wt[m] = wt[i];
        ++m;
    }
    return m;
}

// shared front half of detect / detectMultiScale: checks, plan, scratch, uploads
static int prepare(tbdk_ctx* ctx, const uint8_t* img, int w, int h, int pitch, int cn, const tbdk_hog_params* p,
                   const float* svm, int svm_len, HogPlan& pl, int64_t hit_cap, hipStream_t s)
{
    if (!ctx || !img || !svm || w <= 0 || h <= 0 || (cn != 1 && cn != 3 && cn != 4) || pitch < (int64_t)w * cn)
        return TBDK_EINVAL;
    int rc = hog_check(p);
    if (rc != TBDK_OK) return rc;
    make_plan(p, pl);
    if (svm_len != pl.dsize && svm_len != pl.dsize + 1) return TBDK_EINVAL;  // checkDetectorSize (hog.cpp:106-112)
    rc = reserve(ctx, w, h, cn, pl, svm_len, hit_cap, s);
    if (rc != TBDK_OK) return rc;
    HogScratch* S = ctx->hog;
    hipError_t e = hipSuccess;
    if (S->svm_host.size() != (size_t)svm_len || std::memcmp(S->svm_host.data(), svm, sizeof(float) * svm_len) != 0) {
        S->svm_host.clear();
        e = hipMemcpyAsync(S->svm, svm, sizeof(float) * svm_len, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);  // `svm` is the caller's pageable memory
        if (e == hipSuccess) S->svm_host.assign(svm, svm + svm_len);
    }
    if (e == hipSuccess) e = upload_plan(S, pl, s);
    if (e == hipSuccess) e = hipMemsetAsync(S->hits, 0, sizeof(int), s);
    return map_status(e);
}

// the lanes' streams and events (1..n-1)
static int create_lanes(HogScratch* S, int n)
{
    if (!S->fork && hipEventCreateWithFlags(&S->fork, hipEventDisableTiming) != hipSuccess) return TBDK_EHIP;
    for (int k = 1; k < n; ++k) {
        if (!S->lane_stream[k] && hipStreamCreateWithFlags(&S->lane_stream[k], hipStreamNonBlocking) != hipSuccess)
            return TBDK_EHIP;
        if (!S->join[k] && hipEventCreateWithFlags(&S->join[k], hipEventDisableTiming) != hipSuccess)
            return TBDK_EHIP;
    }
    return TBDK_OK;
}

// lanes 1..n-1 of a multi-level call: streams, events and level buffers for
// images of up to px pixels
static int reserve_lanes(HogScratch* S, int n, int64_t px)
{
    int rc = create_lanes(S, n);
    if (rc != TBDK_OK) return rc;
    for (int k = 1; k < n; ++k) {
        if (px <= S->lane_cap_px[k]) continue;
        int64_t c0 = 0, c1 = 0, c2 = 0;
        S->lane_cap_px[k] = 0;
        if ((rc = grow(&S->lane_level[k], c0, px * 4, S->fill)) || (rc = grow(&S->lane_grad[k], c1, px * 2, S->fill)) ||
            (rc = grow(&S->lane_qangle[k], c2, px * 2, S->fill)))
            return rc;
        S->lane_cap_px[k] = px;
    }
    return TBDK_OK;
}

struct Hit {
    int level, x, y;
    double score;
};

static int fetch_hits(HogScratch* S, int64_t cap, std::vector<Hit>& out, hipStream_t s)
{
    int n = 0;
    hipError_t e = hipMemcpyAsync(&n, S->hits, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return map_status(e);
    if (n > cap) return TBDK_ENOMEM;
    std::vector<int> tri(3 * (size_t)n);
    std::vector<double> sc(n);
    if (n) {
        e = hipMemcpyAsync(tri.data(), S->hits + 1, sizeof(int) * 3 * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sc.data(), S->scores, sizeof(double) * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return map_status(e);
    }
    out.resize(n);
    for (int i = 0; i < n; ++i) out[i] = Hit{tri[3 * i], tri[3 * i + 1], tri[3 * i + 2], sc[i]};
    // window order within a level (the reference's sequential loop)
    std::sort(out.begin(), out.end(), [](const Hit& a, const Hit& b) {
        return a.level != b.level ? a.level < b.level : a.y != b.y ? a.y < b.y : a.x < b.x;
    });
    return TBDK_OK;
}

}  // namespace tbdk

using namespace tbdk;

// Called by tbdk_ctx_create: the lanes' streams exist before any stream the
// caller creates afterwards.  HIP maps streams onto a few hardware queues in
// creation order; lanes created after, e.g., a TBD loop's four streams shared
// queues with the caller's stream and overlapped nothing (1080p HOG 780 instead
// of 1130 frames/s, tools/probe_hog_after_loop.py).
void tbdk::hog_create_lanes(tbdk_ctx* ctx)
{
    if (!ctx->hog) ctx->hog = new (std::nothrow) HogScratch();
    if (ctx->hog) (void)create_lanes(ctx->hog, std::min(ctx->opt_hog_level_streams, HogScratch::kMaxLanes));
}

// every buffer over its whole capacity; the host copies of `cells` and `svm`
// forgotten, so the next call uploads both again
hipError_t tbdk::hog_debug_fill(tbdk_ctx* ctx, int byte, int64_t* bytes)
{
    HogScratch* S = ctx->hog;
    if (!S) return hipSuccess;
    S->cells_host.clear();
    S->svm_host.clear();
    std::vector<std::pair<void*, size_t>> bufs = {
        {S->level, (size_t)S->cap_px * 4},
        {S->grad, sizeof(float) * (size_t)S->cap_px * 2},
        {S->qangle, (size_t)S->cap_px * 2},
        {S->blocks, sizeof(float) * (size_t)S->cap_blocks},
        {S->svm, sizeof(float) * (size_t)S->cap_svm},
        {S->cells, sizeof(int4) * (size_t)S->cap_cells},
        {S->hits, sizeof(int) * (size_t)(1 + 3 * S->cap_hits)},
        {S->scores, sizeof(double) * (size_t)S->cap_hits},
        {S->mblocks, sizeof(float) * (size_t)S->cap_mblocks},
        {S->lvtab, sizeof(HogLevelEnt) * (size_t)S->cap_lvtab}};
    for (int k = 1; k < HogScratch::kMaxLanes; ++k) {
        bufs.push_back({S->lane_level[k], (size_t)S->lane_cap_px[k] * 4});
        bufs.push_back({S->lane_grad[k], sizeof(float) * (size_t)S->lane_cap_px[k] * 2});
        bufs.push_back({S->lane_qangle[k], (size_t)S->lane_cap_px[k] * 2});
    }
    for (const auto& b : bufs) {
        if (!b.first || !b.second) continue;
        const hipError_t e = hipMemset(b.first, byte, b.second);
        if (e != hipSuccess) return e;
        *bytes += (int64_t)b.second;
    }
    return hipSuccess;
}

void tbdk::hog_release(tbdk_ctx* ctx)
{
    HogScratch* S = ctx->hog;
    if (!S) return;
    for (void* p : {(void*)S->level, (void*)S->grad, (void*)S->qangle, (void*)S->blocks, (void*)S->svm,
                    (void*)S->cells, (void*)S->hits, (void*)S->scores, (void*)S->mblocks,
                    (void*)S->lvtab})
        if (p) (void)hipFree(p);
    for (int k = 1; k < HogScratch::kMaxLanes; ++k) {
        for (void* p : {(void*)S->lane_level[k], (void*)S->lane_grad[k], (void*)S->lane_qangle[k]})
            if (p) (void)hipFree(p);
        if (S->lane_stream[k]) (void)hipStreamDestroy(S->lane_stream[k]);
        if (S->join[k]) (void)hipEventDestroy(S->join[k]);
    }
    if (S->fork) (void)hipEventDestroy(S->fork);
    delete S;
    ctx->hog = nullptr;
}

extern "C" {

int tbdk_hog_default_params(tbdk_hog_params* p)
{
    if (!p) return TBDK_EINVAL;
    p->win_w = 64, p->win_h = 128;
    p->block_w = 16, p->block_h = 16;
    p->block_stride_x = 8, p->block_stride_y = 8;
    p->cell_w = 8, p->cell_h = 8;
    p->nbins = 9;
    p->win_sigma = -1.0;
    p->l2hys_threshold = 0.2;
    p->gamma_correction = 1;
    p->signed_gradient = 0;
    p->nlevels = 64;
    p->hit_threshold = 0.0;
    p->win_stride_x = 8, p->win_stride_y = 8;
    p->scale0 = 1.05;
    p->group_threshold = 2;
    return TBDK_OK;
}

int tbdk_hog_descriptor_size(const tbdk_hog_params* p, int* size)
{
    if (!size || hog_check(p) != TBDK_OK) return TBDK_EINVAL;
    *size = descriptor_size(p);
    return TBDK_OK;
}

int tbdk_hog_resize(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int pitch, int cn, uint8_t* dst,
                    int dst_width, int dst_height, int dst_pitch, void* stream)
{
    if (!ctx || !src || !dst || width <= 0 || height <= 0 || dst_width <= 0 || dst_height <= 0 || cn < 1 || cn > 4 ||
        pitch < (int64_t)width * cn || dst_pitch < (int64_t)dst_width * cn)
        return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    const ExactAxis ax = exact_axis(width, dst_width), ay = exact_axis(height, dst_height);
    hipLaunchKernelGGL(hog_resize_kernel, dim3((dst_width + 255) / 256, dst_height), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, width, height, pitch, cn, dst, dst_width, dst_height,
                       dst_pitch, ax, ay);
    return map_status(hipGetLastError());
}

int tbdk_hog_gradient(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int cn,
                      const tbdk_hog_params* params, float* grad, int grad_pitch, uint8_t* qangle,
                      int qangle_pitch, void* stream)
{
    if (!ctx || !img || !grad || !qangle || width <= 0 || height <= 0 || (cn != 1 && cn != 3 && cn != 4) ||
        pitch < (int64_t)width * cn || grad_pitch < (int64_t)8 * width || grad_pitch % 8 ||
        qangle_pitch < (int64_t)2 * width ||
        qangle_pitch % 2)
        return TBDK_EINVAL;
    if (hog_check(params) != TBDK_OK) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    return map_status(launch_grad(img, width, height, pitch, cn, params, grad, grad_pitch / 4, qangle, qangle_pitch,
                                  static_cast<hipStream_t>(stream)));
}

int tbdk_hog_blocks(tbdk_ctx* ctx, const float* grad, int grad_pitch, const uint8_t* qangle, int qangle_pitch,
                    int width, int height, const tbdk_hog_params* params, float* blocks, void* stream)
{
    if (!ctx || !grad || !qangle || !blocks || grad_pitch % 8 || grad_pitch < (int64_t)8 * width || qangle_pitch % 2 ||
        qangle_pitch < (int64_t)2 * width)
        return TBDK_EINVAL;
    if (hog_check(params) != TBDK_OK) return TBDK_EINVAL;
    if (width < params->block_w || height < params->block_h) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    HogPlan pl;
    make_plan(params, pl);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = reserve(ctx, 1, 1, 1, pl, 1, 1, s);
    if (rc != TBDK_OK) return rc;
    hipError_t e = upload_plan(ctx->hog, pl, s);
    if (e != hipSuccess) return map_status(e);
    const int nbx = (width - params->block_w) / pl.csx + 1, nby = (height - params->block_h) / pl.csy + 1;
    return map_status(launch_blocks(ctx->hog, pl, params, grad, grad_pitch / 4, qangle, qangle_pitch, nbx, nby,
                                    blocks, s));
}

int tbdk_hog_detect(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int cn,
                    const tbdk_hog_params* params, const float* svm, int svm_len, int32_t* xy, double* scores,
                    int max_hits, int* nhits, void* stream)
{
    if (!nhits || max_hits < 0 || (max_hits > 0 && (!xy || !scores))) return TBDK_EINVAL;
    *nhits = 0;
    if (!ctx) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HogPlan pl;
    const int64_t cap = (int64_t)(width / std::max(params ? params->win_stride_x : 1, 1) + 1) *
                        (height / std::max(params ? params->win_stride_y : 1, 1) + 1);
    int rc = prepare(ctx, img, width, height, pitch, cn, params, svm, svm_len, pl, cap, s);
    if (rc != TBDK_OK) return rc;
    if (width < params->win_w || height < params->win_h) return TBDK_OK;
    const double rho = svm_len > pl.dsize ? svm[pl.dsize] : 0;
    hipError_t e = run_level(ctx, ctx->hog, pl, params, img, width, height, pitch, cn, rho, 0, (int)cap, s);
    if (e != hipSuccess) return map_status(e);
    std::vector<Hit> hits;
    rc = fetch_hits(ctx->hog, cap, hits, s);
    if (rc != TBDK_OK) return rc;
    const int n = std::min((int)hits.size(), max_hits);
    for (int i = 0; i < n; ++i) {
        xy[2 * i] = hits[i].x;
        xy[2 * i + 1] = hits[i].y;
        scores[i] = hits[i].score;
    }
    *nhits = n;
    return (int)hits.size() > max_hits ? TBDK_ENOMEM : TBDK_OK;
}

int tbdk_hog_detect_multiscale(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int cn,
                               const tbdk_hog_params* params, const float* svm, int svm_len, int32_t* rects,
                               double* weights, int max_rects, int* nrects, void* stream)
{
    if (!nrects || max_rects < 0 || (max_rects > 0 && (!rects || !weights))) return TBDK_EINVAL;
    *nrects = 0;
    if (!ctx || !params || params->nlevels < 1) return TBDK_EINVAL;
    DeviceGuard g(ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // level scales (hog.cpp:2058-2073)
    std::vector<double> lv;
    double scale = 1.;
    for (int l = 0; l < params->nlevels; ++l) {
        lv.push_back(scale);
        if (cv_round_d(width / scale) < params->win_w || cv_round_d(height / scale) < params->win_h ||
            params->scale0 <= 1) {
            lv.pop_back();
            break;
        }
        scale *= params->scale0;
    }
    if (lv.empty()) lv.push_back(1.);
    // every window of every level can hit: size the hit list for all of them
    int64_t cap = 1;
    for (double sc : lv) {
        const int sw = cv_round_d(width / sc), sh = cv_round_d(height / sc);
        if (sw >= params->win_w && sh >= params->win_h && params->win_stride_x > 0 && params->win_stride_y > 0)
            cap += (int64_t)((sw - params->win_w) / params->win_stride_x + 1) *
                   ((sh - params->win_h) / params->win_stride_y + 1);
    }
    HogPlan pl;
    int rc = prepare(ctx, img, width, height, pitch, cn, params, svm, svm_len, pl, cap, s);
    if (rc != TBDK_OK) return rc;
    HogScratch* S = ctx->hog;
    const double rho = svm_len > pl.dsize ? svm[pl.dsize] : 0;
    // the window pass: tiled (blocks and detector staged in LDS) for 36-float
    // blocks when the tile fits, else one wave per window from L2
    HogWinTile wtile{};
    size_t wtile_lds = 0;
    bool win_tiled = false;
    if (ctx->opt_hog_window_tiled && pl.hsz == 36) {
        wtile.cstep = params->win_stride_x / pl.csx, wtile.rstep = params->win_stride_y / pl.csy;
        wtile.bstepx = params->block_stride_x / pl.csx, wtile.bstepy = params->block_stride_y / pl.csy;
        wtile.cols = (kHogWinTile - 1) * wtile.cstep + (pl.wbx - 1) * wtile.bstepx + 1;
        wtile.rows = (pl.wby - 1) * wtile.bstepy + 1;
        wtile.off_svm = wtile.rows * wtile.cols * 36;
        wtile.off_d = (wtile.off_svm + pl.wbx * pl.wby * 36 + 1) & ~1;
        wtile_lds = sizeof(float) * ((size_t)wtile.off_d + 2 * kHogWinTile * (size_t)(pl.wbx * pl.wby));
        win_tiled = wtile_lds <= kHogWinTileLds;
    }
    // every level's blocks get their own region of one buffer, so the window
    // pass runs once over all levels (small levels alone fill a fraction of the
    // device; batching the block pass as well measured 14 % slower for it)
    std::vector<HogLevelEnt> ents;
    int64_t boff = 0;
    int nwwg = 0;
    for (int l = 0; l < (int)lv.size(); ++l) {
        const int sw = cv_round_d(width / lv[l]), sh = cv_round_d(height / lv[l]);
        if (sw < params->win_w || sh < params->win_h) continue;
        HogLevelEnt en;
        en.boff = boff;
        en.gpitch = 2 * sw, en.qpitch = 2 * sw;
        en.nbx = (sw - params->block_w) / pl.csx + 1, en.nby = (sh - params->block_h) / pl.csy + 1;
        en.nwx = (sw - params->win_w) / params->win_stride_x + 1;
        en.nwy = (sh - params->win_h) / params->win_stride_y + 1;
        en.level = l, en.w0 = nwwg;
        ents.push_back(en);
        boff += (int64_t)en.nbx * en.nby * pl.hsz;
        nwwg += win_tiled ? en.nwy * ((en.nwx + kHogWinTile - 1) / kHogWinTile)
                          : (en.nwx * en.nwy + kHogWinPerWg - 1) / kHogWinPerWg;
    }
    if ((rc = grow(&S->mblocks, S->cap_mblocks, std::max<int64_t>(boff, 1), S->fill)) ||
        (rc = grow(&S->lvtab, S->cap_lvtab, std::max<int64_t>((int64_t)ents.size(), 1), S->fill)))
        return rc;
    hipError_t e = ents.empty() ? hipSuccess
                                : hipMemcpyAsync(S->lvtab, ents.data(), sizeof(HogLevelEnt) * ents.size(),
                                                 hipMemcpyHostToDevice, s);
    // the levels' chains are independent until the window pass: spread them
    // over lanes (streams) so the latency-bound launches of several levels overlap
    const int nlanes = std::max(1, std::min<int>(ctx->opt_hog_level_streams, (int)ents.size()));
    if (nlanes > 1) {
        if ((rc = reserve_lanes(S, nlanes, (int64_t)width * height)) != TBDK_OK) return rc;
        if (e == hipSuccess) e = hipEventRecord(S->fork, s);
        for (int k = 1; k < nlanes && e == hipSuccess; ++k) e = hipStreamWaitEvent(S->lane_stream[k], S->fork, 0);
    }
    for (size_t k = 0; k < ents.size() && e == hipSuccess; ++k) {
        const HogLevelEnt& en = ents[k];
        const int ln = (int)(k % nlanes);
        hipStream_t ls = ln ? S->lane_stream[ln] : s;
        uint8_t* lvl = ln ? S->lane_level[ln] : S->level;
        float* grd = ln ? S->lane_grad[ln] : S->grad;
        uint8_t* qa = ln ? S->lane_qangle[ln] : S->qangle;
        const int sw = en.gpitch / 2, sh = cv_round_d(height / lv[en.level]);
        const uint8_t* li = img;
        int lp = pitch;
        if (sw != width || sh != height) {
            const ExactAxis ax = exact_axis(width, sw), ay = exact_axis(height, sh);
            const int rec = timing_begin(ctx, "hog_resize", ls);
            hipLaunchKernelGGL(hog_resize_kernel, dim3((sw + 255) / 256, sh), dim3(256), 0, ls, img, width, height,
                               pitch, cn, lvl, sw, sh, sw * cn, ax, ay);
            timing_end(ctx, rec, ls);
            e = hipGetLastError();
            li = lvl;
            lp = sw * cn;
        }
        if (e != hipSuccess) break;
        int rec = timing_begin(ctx, "hog_grad", ls);
        e = launch_grad(li, sw, sh, lp, cn, params, grd, en.gpitch, qa, en.qpitch, ls);
        timing_end(ctx, rec, ls);
        if (e != hipSuccess) break;
        rec = timing_begin(ctx, "hog_block", ls);
        e = launch_blocks(S, pl, params, grd, en.gpitch, qa, en.qpitch, en.nbx, en.nby, S->mblocks + en.boff, ls);
        timing_end(ctx, rec, ls);
    }
    // join every lane (also on failure: later calls order behind `s` only)
    for (int k = 1; k < nlanes; ++k) {
        hipError_t j = hipEventRecord(S->join[k], S->lane_stream[k]);
        if (j == hipSuccess) j = hipStreamWaitEvent(s, S->join[k], 0);
        if (e == hipSuccess) e = j;
    }
    if (e == hipSuccess && !ents.empty()) {
        {
            HogWinArgs w;
            w.blocks = S->mblocks, w.svm = S->svm;
            w.nbx = 0, w.csx = pl.csx, w.csy = pl.csy;
            w.wbx = pl.wbx, w.wby = pl.wby, w.bsx = params->block_stride_x, w.bsy = params->block_stride_y;
            w.hsz = pl.hsz;
            w.nwx = 0, w.nwy = 0, w.wsx = params->win_stride_x, w.wsy = params->win_stride_y;
            w.rho = rho, w.hit = params->hit_threshold, w.level = 0;
            w.hits = S->hits, w.scores = S->scores, w.cap = (int)cap;
            w.lv = S->lvtab, w.nlv = (int)ents.size();
            const int rec = timing_begin(ctx, "hog_window", s);
            if (win_tiled) {
                e = wtile_lds > 64 * 1024 ? win_lds_opt_in() : hipSuccess;
                if (e != hipSuccess) return map_status(e);
                // "hog_window_tile": the tiled pass ran (tests count it; no event pair unless selected)
                timing_end(ctx, timing_begin(ctx, "hog_window_tile", s), s);
                hipLaunchKernelGGL(hog_window_tile_kernel, dim3(nwwg), dim3(256), wtile_lds, s, w, wtile);
            } else {
                const size_t lds = sizeof(double) * 4 * kHogWinPerWg * (size_t)(pl.wbx * pl.wby);
                hipLaunchKernelGGL(hog_window_kernel, dim3(nwwg), dim3(256), lds, s, w);
            }
            timing_end(ctx, rec, s);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) return map_status(e);
    std::vector<Hit> hits;
    rc = fetch_hits(S, cap, hits, s);
    if (rc != TBDK_OK) return rc;
    // HOGInvoker's rects (hog.cpp:1818-1828)
    std::vector<int> r;
    std::vector<double> wt;
    r.reserve(4 * hits.size());
    for (const Hit& h : hits) {
        const double sc = lv[h.level];
        r.push_back(cv_round_d(h.x * sc));
        r.push_back(cv_round_d(h.y * sc));
        r.push_back(cv_round_d(params->win_w * sc));
        r.push_back(cv_round_d(params->win_h * sc));
        wt.push_back(h.score);
    }
    const int n = group_and_clip(r, wt, params->group_threshold, 0.2, width, height);
    const int m = std::min(n, max_rects);
    for (int i = 0; i < m; ++i) {
        for (int t = 0; t < 4; ++t) rects[4 * i + t] = r[4 * i + t];
        weights[i] = wt[i];
    }
    *nrects = m;
    return n > max_rects ? TBDK_ENOMEM : TBDK_OK;
}

}  // extern "C"
