// ccl.hip — cv::connectedComponents / cv::connectedComponentsWithStats
// (imgproc/src/connectedcomponents.cpp) on the device, CV_32S labels.
//
// The numbering.  The reference creates provisional labels in scan order, a
// union keeps the smaller root and flattenL numbers the roots in increasing
// order, so a component's final label is 1 + the number of components whose
// first scanned element comes before its own.  LabelingWu (CCL_WU, and every
// call at connectivity 4) scans pixels in raster order; LabelingGrana
// (CCL_GRANA / CCL_DEFAULT at connectivity 8) scans 2x2 blocks in block raster
// order.  So the key of a component is the raster index of its first pixel
// (Wu) or of its first 2x2 block (Grana; a block's pixels are 8-connected to
// each other, so no two components share a block), and its label is the rank
// of its key.
//
// Phases, one kernel each, nothing but kernel boundaries between them:
//   init      parent[i] = raster index of the start of i's horizontal run
//             (within its 64-pixel wave segment; wave ballot), -1 for background;
//             key and flag planes and the stats accumulators cleared
//   merge     union-find: a run's pieces across segment boundaries, and each
//             pixel with the row above where a new overlap starts
//   compress  parent[i] = root; Wu: flag[root] = 1; Grana: atomicMin of the block
//             index into key[root], from run starts only
//   flag      Grana only: flag[key[root]] = 1 for every root
//   reduce / scan_tiles / scan   exclusive scan of the flag plane -> rank, N
//   relabel   labels = rank[key(root)] + 1; stats summed per run of equal labels
//             in a wave (closed form), per 64 x 64 tile in LDS, then global atomics
//   finish    width, height, centroids into the caller's rows l < min(N, cap)
// Unions keep the minimum, so a component's root is its first pixel in raster
// order whatever the order the atomics land in; all stats are integers, so
// their order does not matter either.  No kernel waits on another workgroup.
#include <climits>

#include "tbdk_internal.hpp"

namespace tbdk {

hipError_t blob_scratch(tbdk_ctx* ctx, void** buf, size_t* cap, size_t need);  // morph.hip

namespace {

constexpr int kRows = 4;             // rows per workgroup of the pixel kernels: 4 waves, each 64 pixels of one row
constexpr int kTileRows = 64;        // rows per workgroup of the relabel kernel
constexpr int kSlots = 128;          // labels a relabel workgroup sums in LDS
constexpr int kScanTile = 1024;      // flags per workgroup of reduce / scan
constexpr int kScanThreads = 256;

struct Acc {  // per label, cleared by init
    int32_t minx, miny, maxx, maxy, area, pad;
    unsigned long long sx, sy;
};
static_assert(sizeof(Acc) == 40, "Acc layout");

struct CcArgs {
    const uint8_t* img;
    int width, height, pitch;
    int conn8;        // 8-connectivity
    int grana;        // keys are 2x2 blocks
    int bw;           // blocks per row (grana)
    int ncs;          // 64-pixel column segments per row
    int32_t* parent;  // [width * height]
    int32_t* key;     // grana: [width * height], the first block of each root
    int32_t* flag;    // [nkeys padded to kScanTile]: 1 at the keys, then their exclusive ranks
    int64_t nkeys, nkeys_pad;
    int32_t* tiles;   // [ntiles]: flag sums, then their exclusive scan
    int ntiles;
    Acc* acc;         // [cap]
    int cap;
    int32_t* labels;
    int labels_pitch; // in int32 elements
    int32_t* stats;   // [cap][5] or null
    double* centroids;  // [cap][2] or null
    int32_t* n_labels;
};

__device__ __forceinline__ int ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Terminates: every entry of parent is at most its own index and only ever
// decreases (atomicMin), so the walk strictly descends until it meets a root.
// A stale read is still an ancestor, since entries only decrease along the
// chain; unite() re-checks through the atomicMin's return value.
__device__ __forceinline__ int find(const int32_t* parent, int i)
{
    for (int p = ld(parent + i); p != i; p = ld(parent + i)) i = p;
    return i;
}

__device__ void unite(int32_t* parent, int a, int b)
{
    for (;;) {
        a = find(parent, a);
        b = find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);  // a was a root when read: link it below b
        if (old == a) return;
        a = old;  // someone linked a first: unite what it was linked to with b
    }
}

// lane's pixel of the workgroup's 64 x kRows tile (tiles in raster order along grid x); false: outside the image
__device__ __forceinline__ bool pixel(const CcArgs& a, int* x, int* y)
{
    const int by = blockIdx.x / a.ncs, bx = blockIdx.x - by * a.ncs;
    *x = bx * 64 + (threadIdx.x & 63);
    *y = by * kRows + (threadIdx.x >> 6);
    return *x < a.width && *y < a.height;
}

__global__ __launch_bounds__(64 * kRows) void cc_init_kernel(const CcArgs a)
{
    // grid-wide clears first (every workgroup takes a slice)
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = tid; i < a.nkeys_pad; i += nthreads) a.flag[i] = 0;
    for (int64_t i = tid; i < a.cap; i += nthreads) a.acc[i] = Acc{INT_MAX, INT_MAX, INT_MIN, INT_MIN, 0, 0, 0ull, 0ull};
    int x, y;
    const bool in = pixel(a, &x, &y);
    const bool fg = in && a.img[(size_t)y * a.pitch + x] != 0;
    const unsigned long long m = __ballot(fg);
    if (!in) return;
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)y * a.width + x;
    int p = -1;
    if (fg) {
        // the lane after the highest background lane below this one starts the run
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);
        const int start = below ? 64 - __builtin_clzll(below) : 0;
        p = (int)(idx - (lane - start));
    }
    a.parent[idx] = p;
    if (a.grana) a.key[idx] = INT_MAX;
}

__global__ __launch_bounds__(64 * kRows) void cc_merge_kernel(const CcArgs a)
{
    int x, y;
    if (!pixel(a, &x, &y)) return;
    const uint8_t* row = a.img + (size_t)y * a.pitch;
    if (!row[x]) return;
    const int idx = y * a.width + x;
    const bool left = x > 0 && row[x - 1];
    // a run continues across the wave segment's edge
    if (left && (threadIdx.x & 63) == 0) unite(a.parent, idx, idx - 1);
    if (y == 0) return;
    const uint8_t* up = row - a.pitch;
    const bool u = up[x], ul = x > 0 && up[x - 1], ur = x + 1 < a.width && up[x + 1];
    if (a.conn8) {
        // A run and a run of the row above that touch are united at the leftmost
        // pixel that touches: where the left neighbour and ul are both set, the left
        // neighbour touches the same run (ul and u are one run), so the pixel is not
        // the leftmost; with u clear, ul and ur are two runs.
        if (u) {
            if (!(left && ul)) unite(a.parent, idx, idx - a.width);
        } else {
            if (ul && !left) unite(a.parent, idx, idx - a.width - 1);
            if (ur) unite(a.parent, idx, idx - a.width + 1);
        }
    } else if (u && !(left && ul)) {
        unite(a.parent, idx, idx - a.width);
    }
}

__global__ __launch_bounds__(64 * kRows) void cc_compress_kernel(const CcArgs a)
{
    int x, y;
    if (!pixel(a, &x, &y)) return;
    const int idx = y * a.width + x;
    if (ld(a.parent + idx) < 0) return;
    const int root = find(a.parent, idx);
    // other lanes may be walking through this entry: the root is an ancestor too
    __hip_atomic_store(a.parent + idx, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!a.grana) {
        if (root == idx) a.flag[idx] = 1;
    } else if (x == 0 || !a.img[(size_t)y * a.pitch + x - 1]) {
        // the first block of a component holds the start of one of its runs.  The key only decreases, so a
        // block that is not below what a (possibly stale) read shows cannot win: most run starts of a large
        // component skip the atomic, which would serialise on the root's one address
        const int blk = (y >> 1) * a.bw + (x >> 1);
        if (blk < ld(a.key + root)) atomicMin(a.key + root, blk);
    }
}

__global__ __launch_bounds__(64 * kRows) void cc_flag_kernel(const CcArgs a)
{
    int x, y;
    if (!pixel(a, &x, &y)) return;
    const int idx = y * a.width + x;
    if (a.parent[idx] == idx) a.flag[a.key[idx]] = 1;
}

// exclusive scan of v over the workgroup (blockDim.x a multiple of 64, at most 1024); *total: the sum
__device__ int block_exscan(int v, int* total)
{
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();  // wsum may still be read from a previous call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < nw; ++w) {
        if (w < wave) base += wsum[w];
        sum += wsum[w];
    }
    *total = sum;
    return base + inc - v;
}

__global__ __launch_bounds__(kScanThreads) void cc_reduce_kernel(const CcArgs a)
{
    const int4 f = reinterpret_cast<const int4*>(a.flag + (size_t)blockIdx.x * kScanTile)[threadIdx.x];
    int total;
    block_exscan(f.x + f.y + f.z + f.w, &total);
    if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
}

// one workgroup: the tile sums' exclusive scan in place, and N
__global__ __launch_bounds__(1024) void cc_scan_tiles_kernel(const CcArgs a)
{
    int carry = 0;
    for (int base = 0; base < a.ntiles; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < a.ntiles ? a.tiles[i] : 0;
        int total;
        const int ex = block_exscan(v, &total);
        if (i < a.ntiles) a.tiles[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *a.n_labels = carry + 1;
}

__global__ __launch_bounds__(kScanThreads) void cc_scan_kernel(const CcArgs a)
{
    int4* p = reinterpret_cast<int4*>(a.flag + (size_t)blockIdx.x * kScanTile) + threadIdx.x;
    const int4 f = *p;
    int total;
    const int ex = a.tiles[blockIdx.x] + block_exscan(f.x + f.y + f.z + f.w, &total);
    *p = make_int4(ex, ex + f.x, ex + f.x + f.y, ex + f.x + f.y + f.z);
}

// one run of `len` pixels of a label, starting at (x, y), added to its sums (in LDS or in global memory)
__device__ __forceinline__ void add_run(Acc* c, int x, int y, int len)
{
    atomicMin(&c->minx, x);
    atomicMax(&c->maxx, x + len - 1);
    atomicMin(&c->miny, y);
    atomicMax(&c->maxy, y);
    atomicAdd(&c->area, len);
    atomicAdd(&c->sx, (unsigned long long)len * x + (unsigned long long)len * (len - 1) / 2);
    atomicAdd(&c->sy, (unsigned long long)len * y);
}
__device__ __forceinline__ void add_acc(Acc* c, const Acc& v)
{
    atomicMin(&c->minx, v.minx);
    atomicMax(&c->maxx, v.maxx);
    atomicMin(&c->miny, v.miny);
    atomicMax(&c->maxy, v.maxy);
    atomicAdd(&c->area, v.area);
    atomicAdd(&c->sx, v.sx);
    atomicAdd(&c->sy, v.sy);
}

// A workgroup relabels a tile of 64 columns x kTileRows rows, four rows a turn.  Every label's sums over the
// tile are gathered in an LDS table first (open addressing, a few probes; a run that finds no slot goes to
// global memory directly), so that a label costs one set of global atomics per tile, not per run: the
// background and a component that spans the image are hit by every tile, and atomics on one address serialise.
__global__ __launch_bounds__(64 * kRows) void cc_relabel_kernel(const CcArgs a)
{
    __shared__ int skey[kSlots];
    __shared__ Acc sacc[kSlots];
    for (int i = threadIdx.x; i < kSlots; i += 64 * kRows) {
        skey[i] = -1;
        sacc[i] = Acc{INT_MAX, INT_MAX, INT_MIN, INT_MIN, 0, 0, 0ull, 0ull};
    }
    __syncthreads();
    const int by = blockIdx.x / a.ncs, bx = blockIdx.x - by * a.ncs;
    const int lane = threadIdx.x & 63, x = bx * 64 + lane;
    const int yend = (by + 1) * kTileRows < a.height ? (by + 1) * kTileRows : a.height;
    for (int y = by * kTileRows + (threadIdx.x >> 6); y < yend; y += kRows) {  // the same turns for a whole wave
        int label = -2;  // outside the image: a run of its own, never counted
        if (x < a.width) {
            const int root = a.parent[y * a.width + x];
            label = root < 0 ? 0 : a.flag[a.grana ? a.key[root] : root] + 1;
            a.labels[(size_t)y * a.labels_pitch + x] = label;
        }
        if (!a.acc) continue;
        // runs of equal labels within the wave (one row): the first lane of each adds the whole run
        const int prev = __shfl_up(label, 1);
        const bool head = lane == 0 || prev != label;
        const unsigned long long heads = __ballot(head);
        if (head && label >= 0 && label < a.cap) {
            const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = after ? __builtin_ctzll(after) + 1 : 64 - lane;
            const unsigned h = ((unsigned)label * 2654435761u) >> 16;
            int slot = -1;
            for (int k = 0; k < 8 && slot < 0; ++k) {
                const int s = (h + k) & (kSlots - 1);
                const int old = atomicCAS(&skey[s], -1, label);
                if (old == -1 || old == label) slot = s;
            }
            if (slot >= 0)
                add_run(&sacc[slot], x, y, len);
            else
                add_run(a.acc + label, x, y, len);
        }
    }
    if (!a.acc) return;
    __syncthreads();
    for (int i = threadIdx.x; i < kSlots; i += 64 * kRows)
        if (skey[i] >= 0) add_acc(a.acc + skey[i], sacc[i]);
}

// CCStatsOp::finish: rows l < min(N, cap); a label without a pixel (label 0 of an
// image with no background) keeps INT_MAX / the wrapped extent / 0 and gets 0/0
__global__ __launch_bounds__(256) void cc_finish_kernel(const CcArgs a)
{
    const int n = *a.n_labels < a.cap ? *a.n_labels : a.cap;
    for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
        const Acc c = a.acc[l];
        if (a.stats) {
            int32_t* r = a.stats + (size_t)l * 5;
            r[0] = c.minx;
            r[1] = c.miny;
            r[2] = (int32_t)((uint32_t)c.maxx - (uint32_t)c.minx + 1u);
            r[3] = (int32_t)((uint32_t)c.maxy - (uint32_t)c.miny + 1u);
            r[4] = c.area;
        }
        if (a.centroids) {
            const double area = (double)(uint32_t)c.area;
            a.centroids[(size_t)l * 2] = (double)c.sx / area;
            a.centroids[(size_t)l * 2 + 1] = (double)c.sy / area;
        }
    }
}

}  // namespace
}  // namespace tbdk

using namespace tbdk;

extern "C" int tbdk_connected_components(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch,
                                         int32_t* labels, int labels_pitch, int connectivity, int ccltype,
                                         int32_t* stats, double* centroids, int cap, int32_t* n_labels, void* stream)
{
    if (!ctx || !img || !labels || !n_labels) return TBDK_EINVAL;
    if (width < 1 || height < 1 || (int64_t)width * height >= ((int64_t)1 << 31) || pitch < width) return TBDK_EINVAL;
    if (labels_pitch < (int64_t)width * 4 || (labels_pitch & 3) != 0 || (reinterpret_cast<uintptr_t>(labels) & 3) != 0)
        return TBDK_EINVAL;
    if (connectivity != 4 && connectivity != 8) return TBDK_EINVAL;
    if (ccltype != TBDK_CCL_DEFAULT && ccltype != TBDK_CCL_WU && ccltype != TBDK_CCL_GRANA) return TBDK_EINVAL;
    const bool want = stats || centroids;
    if (cap < 0 || (want && cap < 1)) return TBDK_EINVAL;
    if ((reinterpret_cast<uintptr_t>(stats) & 3) != 0 || (reinterpret_cast<uintptr_t>(centroids) & 7) != 0 ||
        (reinterpret_cast<uintptr_t>(n_labels) & 3) != 0)
        return TBDK_EINVAL;

    CcArgs a{};
    a.img = img;
    a.width = width;
    a.height = height;
    a.pitch = pitch;
    a.conn8 = connectivity == 8;
    a.grana = a.conn8 && ccltype != TBDK_CCL_WU;
    a.bw = (width + 1) / 2;
    a.ncs = (width + 63) / 64;
    const int64_t px = (int64_t)width * height;
    a.nkeys = a.grana ? (int64_t)a.bw * ((height + 1) / 2) : px;
    a.nkeys_pad = (a.nkeys + kScanTile - 1) / kScanTile * kScanTile;
    a.ntiles = (int)(a.nkeys_pad / kScanTile);
    a.cap = want ? cap : 0;
    a.labels = labels;
    a.labels_pitch = labels_pitch / 4;
    a.stats = stats;
    a.centroids = centroids;
    a.n_labels = n_labels;

    // the scratch's layout: every part 256-byte aligned
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_parent = 0;
    const size_t o_key = o_parent + up((size_t)px * 4);
    const size_t o_flag = o_key + (a.grana ? up((size_t)px * 4) : 0);
    const size_t o_tiles = o_flag + up((size_t)a.nkeys_pad * 4);
    const size_t o_acc = o_tiles + up((size_t)a.ntiles * 4);
    const size_t need = o_acc + up((size_t)a.cap * sizeof(Acc));
    DeviceGuard g(ctx->device);
    hipError_t e = blob_scratch(ctx, &ctx->cc_buf, &ctx->cc_cap, need);
    if (e != hipSuccess) return map_status(e);
    char* base = static_cast<char*>(ctx->cc_buf);
    a.parent = reinterpret_cast<int32_t*>(base + o_parent);
    a.key = a.grana ? reinterpret_cast<int32_t*>(base + o_key) : nullptr;
    a.flag = reinterpret_cast<int32_t*>(base + o_flag);
    a.tiles = reinterpret_cast<int32_t*>(base + o_tiles);
    a.acc = a.cap ? reinterpret_cast<Acc*>(base + o_acc) : nullptr;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 pgrid((unsigned)((int64_t)a.ncs * ((height + kRows - 1) / kRows))), pblock(64 * kRows);
    const int rec = timing_begin(ctx, "cc", s);
    hipLaunchKernelGGL(cc_init_kernel, pgrid, pblock, 0, s, a);
    hipLaunchKernelGGL(cc_merge_kernel, pgrid, pblock, 0, s, a);
    hipLaunchKernelGGL(cc_compress_kernel, pgrid, pblock, 0, s, a);
    if (a.grana) hipLaunchKernelGGL(cc_flag_kernel, pgrid, pblock, 0, s, a);
    hipLaunchKernelGGL(cc_reduce_kernel, dim3(a.ntiles), dim3(kScanThreads), 0, s, a);
    hipLaunchKernelGGL(cc_scan_tiles_kernel, dim3(1), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(a.ntiles), dim3(kScanThreads), 0, s, a);
    const dim3 rgrid((unsigned)((int64_t)a.ncs * ((height + kTileRows - 1) / kTileRows)));
    hipLaunchKernelGGL(cc_relabel_kernel, rgrid, pblock, 0, s, a);
    if (a.cap) {
        const int blocks = a.cap < 256 * 1024 ? (a.cap + 255) / 256 : 1024;
        hipLaunchKernelGGL(cc_finish_kernel, dim3(blocks), dim3(256), 0, s, a);
    }
    e = hipGetLastError();
    timing_end(ctx, rec, s);
    return map_status(e);
}
