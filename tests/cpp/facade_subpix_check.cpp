// facade_subpix_check.cpp — compiles tbdk::cornerSubPix of the C++ facade
// (include/tbdk.hpp) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV)
//   GPU    : GFTT corners of an 8U and a 32F image refined through the facade
//            (rows with device counts, a flat list, the GpuImage form) equal the
//            C entry's (tbdk_corner_sub_pix) byte for byte, and some corner moves;
//            a two-channel view and a window of 0 throw tbdk::Error(TBDK_EINVAL)
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

namespace {

constexpr int W = 200, H = 150, MAXC = 128, NROI = 3;

template <typename T>
T* upload(const std::vector<T>& v)
{
    T* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) return nullptr;
    (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}

std::vector<float> fetch(const float* d)
{
    std::vector<float> h((size_t)NROI * MAXC * 2);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost);
    return h;
}

bool same(const std::vector<float>& a, const std::vector<float>& b) { return std::memcmp(a.data(), b.data(), a.size() * 4) == 0; }

}  // namespace

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        std::vector<uint8_t> h8((size_t)W * H);
        std::vector<float> h32((size_t)W * H);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const unsigned v = (unsigned)(x * 7 + y * 13 + ((x / 9) ^ (y / 7)) * 40) & 255u;
                const unsigned lo = (unsigned)(x * 2654435761u + y * 40503u) >> 24;
                h8[(size_t)y * W + x] = (uint8_t)v;
                h32[(size_t)y * W + x] = (float)v + (float)lo / 256.f;
            }
        uint8_t* d8 = upload(h8);
        float* d32 = upload(h32);
        const tbdk_roi rois[NROI] = {{0, 0, W, H}, {33, 20, 113, 80}, {150, 100, 1, 1}};
        float *c0, *ca, *cb;
        int32_t* dn;
        const size_t cbytes = (size_t)NROI * MAXC * 8;
        if (!d8 || !d32 || hipMalloc(&c0, cbytes) || hipMalloc(&ca, cbytes) || hipMalloc(&cb, cbytes) ||
            hipMalloc(&dn, NROI * 4))
            return 4;
        const tbdk::GpuImage i8{d8, W, H, W};
        const tbdk::GpuMatView v8{d8, W, H, W, tbdk::DEPTH_8U, 1}, v32{d32, W, H, W * 4, tbdk::DEPTH_32F, 1};
        auto det = tbdk::cuda::CornersDetector::create(ctx, MAXC, 0.05, 4.0);
        (void)hipMemset(c0, 0, cbytes);
        det->detectRois(i8, rois, NROI, c0, dn);
        int32_t hn[NROI];
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(hn, dn, sizeof hn, hipMemcpyDeviceToHost);
        std::printf("corners %d %d %d\n", hn[0], hn[1], hn[2]);
        if (hn[0] <= 0 || hn[1] <= 0 || hn[2] != 0) return 6;
        const std::vector<float> start = fetch(c0);
        tbdk::TermCriteria crit;
        crit.type = tbdk::TermCriteria::COUNT | tbdk::TermCriteria::EPS;
        crit.maxCount = 30;
        crit.epsilon = 0.01;
        const tbdk_subpix_params prm{5, 7, 1, 1, 3, 30, 0.01};
        int moved = 0;
        for (int k = 0; k < 2; ++k) {
            const tbdk::GpuMatView& v = k ? v32 : v8;
            // rows with device counts: the facade is the C entry
            (void)hipMemcpy(ca, c0, cbytes, hipMemcpyDeviceToDevice);
            (void)hipMemcpy(cb, c0, cbytes, hipMemcpyDeviceToDevice);
            tbdk::cornerSubPix(ctx, v, ca, dn, NROI, MAXC, tbdk::Size{5, 7}, tbdk::Size{1, 1}, crit);
            tbdk::check(tbdk_corner_sub_pix(ctx.get(), v.data, k ? TBDK_PIX_F32 : TBDK_PIX_U8, W, H, v.pitch, cb, dn, NROI,
                                            MAXC, &prm, nullptr),
                        "tbdk_corner_sub_pix");
            const std::vector<float> a = fetch(ca), b = fetch(cb);
            if (!same(a, b)) return 7;
            for (int r = 0; r < NROI; ++r)
                for (int i = 0; i < MAXC; ++i) {
                    const bool diff = std::memcmp(&a[((size_t)r * MAXC + i) * 2], &start[((size_t)r * MAXC + i) * 2], 8) != 0;
                    if (diff && i >= hn[r]) return 8;  // beyond a row's count nothing changes
                    moved += diff;
                }
            // the flat-list form refines row 0's first hn[0] points the same way
            (void)hipMemcpy(cb, c0, cbytes, hipMemcpyDeviceToDevice);
            tbdk::cornerSubPix(ctx, v, cb, hn[0], tbdk::Size{5, 7}, tbdk::Size{1, 1}, crit);
            const std::vector<float> f = fetch(cb);
            if (std::memcmp(f.data(), a.data(), 8 * (size_t)hn[0]) != 0) return 9;
            if (std::memcmp(f.data() + 2 * (size_t)hn[0], start.data() + 2 * (size_t)hn[0], cbytes - 8 * (size_t)hn[0]) != 0)
                return 10;
        }
        if (moved <= 0) return 11;
        // the GpuImage form with lkdemo's defaults is the 8U view's
        (void)hipMemcpy(ca, c0, cbytes, hipMemcpyDeviceToDevice);
        (void)hipMemcpy(cb, c0, cbytes, hipMemcpyDeviceToDevice);
        tbdk::cornerSubPix(ctx, i8, ca, hn[0]);
        tbdk_subpix_params dp;
        tbdk::check(tbdk_subpix_default_params(&dp), "tbdk_subpix_default_params");
        tbdk::check(tbdk_corner_sub_pix(ctx.get(), d8, TBDK_PIX_U8, W, H, W, cb, nullptr, 1, hn[0], &dp, nullptr),
                    "tbdk_corner_sub_pix");
        if (!same(fetch(ca), fetch(cb))) return 12;
        // what the call does not take
        for (int bad = 0; bad < 2; ++bad) {
            tbdk::GpuMatView v = v32;
            if (bad == 0) v.cn = 2;
            try {
                tbdk::cornerSubPix(ctx, v, ca, hn[0], bad == 0 ? tbdk::Size{5, 5} : tbdk::Size{0, 5});
                return 13;
            } catch (const tbdk::Error& e) {
                if (e.code() != TBDK_EINVAL) return 14;
            }
        }
        std::printf("moved %d\n", moved);
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 5;
    }
}
