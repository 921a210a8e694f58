// gftt_mask_check.cpp — compiles the C++ facade's masked corner detection
// (CornersDetector::detect / detectRois with a mask, include/tbdk.hpp) against
// libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV)
//   GPU    : detect(image, mask, ...) on a small frame: no corner on a zero mask
//            byte, fewer corners than without the mask; a mask of another size
//            throws tbdk::Error(TBDK_EINVAL)
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        const int W = 320, H = 240, MP = W + 7, MAXC = 1024;  // mask rows MP bytes apart, from an odd offset
        std::vector<uint8_t> h((size_t)W * H), m((size_t)MP * H + 1, 0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                h[(size_t)y * W + x] = (uint8_t)((x * 7 + y * 13 + ((x / 9) ^ (y / 7)) * 40) & 255);
                m[1 + (size_t)y * MP + x] = (x >= 150 || ((x / 8 + y / 8) & 1)) ? 0 : (uint8_t)(1 + (x + y) % 255);
            }
        uint8_t *d, *dm;
        float* corners;
        int32_t* cnt;
        if (hipMalloc(&d, h.size()) || hipMalloc(&dm, m.size()) || hipMalloc(&corners, 8 * MAXC * 2) ||
            hipMalloc(&cnt, 8))
            return 4;
        (void)hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice);
        (void)hipMemcpy(dm, m.data(), m.size(), hipMemcpyHostToDevice);
        const tbdk::GpuImage img{d, W, H, W}, mask{dm + 1, W, H, MP};
        auto det = tbdk::cuda::CornersDetector::create(ctx, MAXC, 0.1, 5.0);
        det->detect(img, corners, cnt);
        det->detect(img, mask, corners + 2 * MAXC, cnt + 1);
        const tbdk_roi rois[2] = {{0, 0, 160, 120}, {100, 60, 77, 33}};
        float* rc;
        int32_t* rn;
        if (hipMalloc(&rc, 8 * MAXC * 2) || hipMalloc(&rn, 8)) return 4;
        det->detectRois(img, mask, rois, 2, rc, rn);
        if (hipDeviceSynchronize() != hipSuccess) return 5;
        int n[2] = {0, 0}, nr[2] = {0, 0};
        (void)hipMemcpy(n, cnt, 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(nr, rn, 8, hipMemcpyDeviceToHost);
        std::printf("corners %d masked %d rois %d %d\n", n[0], n[1], nr[0], nr[1]);
        if (n[0] <= 0 || n[1] <= 0 || n[1] >= n[0] || nr[0] <= 0 || nr[1] < 0) return 6;
        std::vector<float> c(2 * (size_t)n[1]);
        (void)hipMemcpy(c.data(), corners + 2 * MAXC, 8 * (size_t)n[1], hipMemcpyDeviceToHost);
        for (int i = 0; i < n[1]; ++i)
            if (m[1 + (size_t)c[2 * i + 1] * MP + (size_t)c[2 * i]] == 0) return 8;  // a corner on a masked-out pixel
        try {
            const tbdk::GpuImage small{dm, W - 1, H, MP};
            det->detect(img, small, corners, cnt);
            return 9;
        } catch (const tbdk::Error& e) {
            if (e.code() != TBDK_EINVAL) return 10;
        }
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 7;
    }
}
