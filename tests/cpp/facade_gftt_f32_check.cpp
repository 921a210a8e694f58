// facade_gftt_f32_check.cpp — compiles the C++ facade's corner detection on typed
// views (CornersDetector::detect / detectRois and cornerResponse on a
// GpuMatView of depth 8U, 16U or 32F, include/tbdk.hpp) against libtbdk.so.
// Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV)
//   GPU    : one 32F and one 16U image, with a mask and without: corner lists,
//            counts and response maps equal to the C entries' (tbdk_gftt_rois_px,
//            tbdk_corner_response_px), the 16U results equal to the 32F ones on the
//            converted image; a two-channel view and an unknown depth throw
//            tbdk::Error(TBDK_EINVAL)
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

namespace {

constexpr int W = 200, H = 150, MAXC = 512;

template <typename T>
T* upload(const std::vector<T>& v)
{
    T* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) return nullptr;
    (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}

struct Out {
    std::vector<float> c;
    std::vector<int32_t> n;
    bool operator==(const Out& o) const
    {
        if (n != o.n) return false;
        for (size_t r = 0; r < n.size(); ++r) {
            if (n[r] < 0) return false;
            if (std::memcmp(&c[r * 2 * MAXC], &o.c[r * 2 * MAXC], 8 * (size_t)n[r]) != 0) return false;
        }
        return true;
    }
};

Out fetch(const float* dc, const int32_t* dn, int nroi)
{
    Out o;
    o.c.resize((size_t)nroi * 2 * MAXC);
    o.n.resize(nroi);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(o.c.data(), dc, o.c.size() * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(o.n.data(), dn, o.n.size() * 4, hipMemcpyDeviceToHost);
    return o;
}

}  // namespace

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        std::vector<uint16_t> h16((size_t)W * H);
        std::vector<float> h32((size_t)W * H), h16f((size_t)W * H);
        std::vector<uint8_t> hm((size_t)W * H);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const unsigned v = (unsigned)(x * 7 + y * 13 + ((x / 9) ^ (y / 7)) * 40) & 255u;
                const unsigned lo = (unsigned)(x * 2654435761u + y * 40503u) >> 24;
                h16[(size_t)y * W + x] = (uint16_t)(v * 256u + lo);
                h16f[(size_t)y * W + x] = (float)h16[(size_t)y * W + x];
                h32[(size_t)y * W + x] = ((float)v + (float)lo / 256.f) / 255.f;
                hm[(size_t)y * W + x] = (x >= 120 || ((x / 8 + y / 8) & 1)) ? 0 : (uint8_t)(1 + (x + y) % 255);
            }
        uint16_t* d16 = upload(h16);
        float *d32 = upload(h32), *d16f = upload(h16f);
        uint8_t* dm = upload(hm);
        const tbdk_roi rois[3] = {{0, 0, W, H}, {33, 20, 113, 80}, {150, 100, 3, 3}};
        float *ca, *cb, *ma, *mb;
        int32_t *na, *nb;
        if (!d16 || !d32 || !d16f || !dm || hipMalloc(&ca, 3 * 8 * MAXC) || hipMalloc(&cb, 3 * 8 * MAXC) ||
            hipMalloc(&na, 12) || hipMalloc(&nb, 12) || hipMalloc(&ma, (size_t)W * H * 4) ||
            hipMalloc(&mb, (size_t)W * H * 4))
            return 4;
        const tbdk::GpuMatView v32{d32, W, H, W * 4, tbdk::DEPTH_32F, 1}, v16{d16, W, H, W * 2, tbdk::DEPTH_16U, 1},
            v16f{d16f, W, H, W * 4, tbdk::DEPTH_32F, 1};
        const tbdk::GpuImage mask{dm, W, H, W};
        auto det = tbdk::cuda::CornersDetector::create(ctx, MAXC, 0.05, 4.0);
        const tbdk_gftt_params prm{MAXC, 0.05, 4.0, 3, 0, 0.04};
        int total = 0;
        for (int with_mask = 0; with_mask < 2; ++with_mask) {
            Out f[3];
            const tbdk::GpuMatView* views[3] = {&v32, &v16, &v16f};
            const int pix[3] = {TBDK_PIX_F32, TBDK_PIX_U16, TBDK_PIX_F32};
            for (int k = 0; k < 3; ++k) {
                (void)hipMemset(ca, 0, 3 * 8 * MAXC);
                (void)hipMemset(cb, 0, 3 * 8 * MAXC);
                if (with_mask) det->detectRois(*views[k], mask, rois, 3, ca, na);
                else det->detectRois(*views[k], rois, 3, ca, na);
                tbdk::check(tbdk_gftt_rois_px(ctx.get(), views[k]->data, pix[k], W, H, views[k]->pitch,
                                              with_mask ? dm : nullptr, with_mask ? W : 0, rois, 3, &prm, cb, nb,
                                              nullptr),
                            "tbdk_gftt_rois_px");
                f[k] = fetch(ca, na, 3);
                if (!(f[k] == fetch(cb, nb, 3))) return 6;  // the facade is the C entry
                // the whole-image form is ROI 0
                if (with_mask) det->detect(*views[k], mask, cb, nb);
                else det->detect(*views[k], cb, nb);
                const Out whole = fetch(cb, nb, 1);
                if (whole.n[0] != f[k].n[0] || std::memcmp(whole.c.data(), f[k].c.data(), 8 * (size_t)whole.n[0]) != 0)
                    return 7;
                total += f[k].n[0];
            }
            std::printf("mask %d: corners 32F %d 16U %d\n", with_mask, f[0].n[0], f[1].n[0]);
            if (f[0].n[0] <= 0 || f[1].n[0] <= 0) return 8;
            if (!(f[1] == f[2])) return 9;  // 16U is 32F on the converted image
        }
        // response maps: facade == C entry, 16U == converted 32F
        for (int mode = 0; mode < 3; ++mode) {
            const int block = mode == 0 ? 3 : 5, harris = mode == 2;
            std::vector<float> a((size_t)W * H), b((size_t)W * H), c((size_t)W * H);
            tbdk::cuda::cornerResponse(ctx, v16, ma, W * 4, block, harris != 0, 0.04);
            tbdk::check(tbdk_corner_response_px(ctx.get(), d16, TBDK_PIX_U16, W, H, W * 2, mb, W * 4, block, harris,
                                                0.04, nullptr),
                        "tbdk_corner_response_px");
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(a.data(), ma, a.size() * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(b.data(), mb, b.size() * 4, hipMemcpyDeviceToHost);
            tbdk::cuda::cornerResponse(ctx, v16f, ma, W * 4, block, harris != 0, 0.04);
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(c.data(), ma, c.size() * 4, hipMemcpyDeviceToHost);
            if (std::memcmp(a.data(), b.data(), a.size() * 4) != 0) return 10;
            if (std::memcmp(a.data(), c.data(), a.size() * 4) != 0) return 11;
        }
        // views the detector does not take
        for (int bad = 0; bad < 2; ++bad) {
            tbdk::GpuMatView v = v32;
            if (bad == 0) v.cn = 2;
            else v.depth = 3;  // CV_16S
            try {
                det->detect(v, ca, na);
                return 12;
            } catch (const tbdk::Error& e) {
                if (e.code() != TBDK_EINVAL) return 13;
            }
            try {
                tbdk::cuda::cornerResponse(ctx, v, ma, W * 4);
                return 14;
            } catch (const tbdk::Error& e) {
                if (e.code() != TBDK_EINVAL) return 15;
            }
        }
        return total > 0 ? 0 : 16;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 5;
    }
}
