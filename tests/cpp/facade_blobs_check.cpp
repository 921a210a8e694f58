// facade_blobs_check.cpp — compiles the C++ facade's getStructuringElement, erode, dilate, morphologyEx,
// connectedComponents and connectedComponentsWithStats (include/tbdk.hpp) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV); the host-side structuring elements are right
//   GPU    : facade_blobs_check gpu <mask.bin> <out.bin> <w> <h> <cap>
//            opens the w x h mask with the 3 x 3 rectangle (in place, pitched), labels the result with stats and
//            writes to out.bin: the opened mask, N (int32), the labels, cap stats rows, cap centroid rows (the
//            test compares them with the numpy restatements); a labels-only call gives the same N and labels;
//            an op that is not built throws
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const tbdk::StructuringElement cross = tbdk::getStructuringElement(tbdk::MORPH_CROSS, tbdk::Size{3, 3});
    const uint8_t want_cross[9] = {0, 1, 0, 1, 1, 1, 0, 1, 0};
    if (cross.width != 3 || cross.height != 3 || std::memcmp(cross.data.data(), want_cross, 9) != 0) return 20;
    const tbdk::StructuringElement ell = tbdk::getStructuringElement(tbdk::MORPH_ELLIPSE, tbdk::Size{5, 5});
    const uint8_t want_ell[25] = {0, 0, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0};
    if (std::memcmp(ell.data.data(), want_ell, 25) != 0) return 21;
    tbdk::Point corner;
    corner.x = corner.y = 0;
    const tbdk::StructuringElement c0 = tbdk::getStructuringElement(tbdk::MORPH_CROSS, tbdk::Size{3, 2}, corner);
    const uint8_t want_c0[6] = {1, 1, 1, 1, 0, 0};
    if (std::memcmp(c0.data.data(), want_c0, 6) != 0) return 22;
    if (tbdk_structuring_element(3, 3, 3, -1, -1, nullptr) != TBDK_EINVAL) return 23;
    if (tbdk_morph_u8(nullptr, 0, nullptr, 1, 1, 1, nullptr, 1, nullptr, 3, 3, -1, -1, 1, 0, -1, nullptr) != TBDK_EINVAL)
        return 24;
    if (tbdk_connected_components(nullptr, nullptr, 1, 1, 1, nullptr, 4, 8, -1, nullptr, nullptr, 0, nullptr, nullptr) !=
        TBDK_EINVAL)
        return 25;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        if (argc != 7) return 4;
        const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), cap = std::atoi(argv[6]);
        std::vector<uint8_t> mask((size_t)w * h);
        FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(mask.data(), 1, mask.size(), f) != mask.size()) return 5;
        std::fclose(f);
        const int pitch = w + 11, lpitch = (w + 3) * 4;
        uint8_t* dmask = nullptr;
        int32_t *dlabels = nullptr, *dlabels2 = nullptr, *dstats = nullptr, *dn = nullptr;
        double* dcent = nullptr;
        if (hipMalloc(&dmask, (size_t)pitch * h) != hipSuccess || hipMalloc(&dlabels, (size_t)lpitch * h) != hipSuccess ||
            hipMalloc(&dlabels2, (size_t)lpitch * h) != hipSuccess || hipMalloc(&dstats, (size_t)cap * 20) != hipSuccess ||
            hipMalloc(&dcent, (size_t)cap * 16) != hipSuccess || hipMalloc(&dn, 8) != hipSuccess)
            return 6;
        (void)hipMemset(dmask, 9, (size_t)pitch * h);
        (void)hipMemcpy2D(dmask, pitch, mask.data(), w, w, h, hipMemcpyHostToDevice);
        (void)hipMemset(dstats, 0x11, (size_t)cap * 20);
        (void)hipMemset(dcent, 0x11, (size_t)cap * 16);
        const tbdk::GpuImage img{dmask, w, h, pitch};
        int thrown = 0;
        try {
            tbdk::morphologyEx(ctx, img, img, 4, tbdk::StructuringElement());  // MORPH_GRADIENT is not built
        } catch (const tbdk::Error& e) {
            thrown += e.code() == TBDK_EINVAL;
        }
        if (thrown != 1) return 7;
        tbdk::morphologyEx(ctx, img, img, tbdk::MORPH_OPEN, tbdk::getStructuringElement(tbdk::MORPH_RECT, tbdk::Size{3, 3}));
        tbdk::connectedComponentsWithStats(ctx, img, tbdk::GpuLabels{dlabels, w, h, lpitch}, dstats, dcent, cap, dn);
        tbdk::connectedComponents(ctx, img, tbdk::GpuLabels{dlabels2, w, h, lpitch}, dn + 1);
        if (hipDeviceSynchronize() != hipSuccess) return 8;
        std::vector<uint8_t> pm((size_t)pitch * h);
        std::vector<int32_t> lab((size_t)(lpitch / 4) * h), lab2(lab.size()), stats((size_t)cap * 5);
        std::vector<double> cent((size_t)cap * 2);
        int32_t n[2];
        (void)hipMemcpy(pm.data(), dmask, pm.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpy(lab.data(), dlabels, lab.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(lab2.data(), dlabels2, lab2.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(stats.data(), dstats, stats.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(cent.data(), dcent, cent.size() * 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(n, dn, 8, hipMemcpyDeviceToHost);
        if (n[0] != n[1]) return 9;
        FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 10;
        for (int r = 0; r < h; ++r) {
            std::fwrite(pm.data() + (size_t)r * pitch, 1, w, o);
            for (int x = w; x < pitch; ++x)
                if (pm[(size_t)r * pitch + x] != 9) return 11;  // the mask's padding was written
        }
        std::fwrite(n, 4, 1, o);
        for (int r = 0; r < h; ++r) {
            std::fwrite(lab.data() + (size_t)r * (lpitch / 4), 4, w, o);
            if (std::memcmp(lab.data() + (size_t)r * (lpitch / 4), lab2.data() + (size_t)r * (lpitch / 4), (size_t)w * 4) != 0)
                return 12;
        }
        std::fwrite(stats.data(), 4, stats.size(), o);
        std::fwrite(cent.data(), 8, cent.size(), o);
        if (std::fclose(o) != 0) return 13;
        std::printf("facade morphology and connected components: ok\n");
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("%s\n", e.what());
        return want_gpu ? 1 : (e.code() == TBDK_ENODEV ? 0 : 2);
    }
}
