// facade_blur_check.cpp — compiles the C++ facade's getGaussianKernelU8, GaussianBlur and threshold
// (include/tbdk.hpp) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV); the host-side coefficients are right
//   GPU    : facade_blur_check gpu <mask.bin> <out.bin> <w> <h>
//            writes to out.bin: the w x h mask blurred 11 x 11 at sigma 3.5 (pitched), the same with the threshold
//            (10, 255, BINARY) fused in, tbdk::threshold of the first (in place), and the Otsu word of the blurred
//            image (int32); the test compares them with the numpy restatements.  A fused Otsu throws
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const std::vector<uint16_t> k5 = tbdk::getGaussianKernelU8(5, 0);
    const uint16_t want5[5] = {16, 64, 96, 64, 16};
    if (k5.size() != 5 || std::memcmp(k5.data(), want5, sizeof want5) != 0) return 20;
    const std::vector<uint16_t> k11 = tbdk::getGaussianKernelU8(11, 3.5);
    int sum = 0;
    for (uint16_t v : k11) sum += v;
    if (sum != 257 || k11[0] != k11[10] || k11[5] <= k11[4]) return 21;
    if (tbdk_gaussian_kernel_u8(0, 1.0, nullptr) != TBDK_EINVAL) return 22;
    if (tbdk_gaussian_blur_u8(nullptr, nullptr, 1, 1, 1, 1, nullptr, 1, 3, 3, 0, 0, 4, nullptr, nullptr) != TBDK_EINVAL)
        return 23;
    if (tbdk_threshold(nullptr, nullptr, 0, 1, 1, 1, 1, nullptr, 1, 0, 0, 0, nullptr, nullptr, nullptr) != TBDK_EINVAL)
        return 24;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        if (argc != 6) return 4;
        const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
        std::vector<uint8_t> mask((size_t)w * h);
        FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(mask.data(), 1, mask.size(), f) != mask.size()) return 5;
        std::fclose(f);
        const int pitch = w + 13;
        uint8_t *dsrc = nullptr, *da = nullptr, *db = nullptr;
        int32_t* dword = nullptr;
        if (hipMalloc(&dsrc, (size_t)pitch * h) != hipSuccess || hipMalloc(&da, (size_t)pitch * h) != hipSuccess ||
            hipMalloc(&db, (size_t)pitch * h) != hipSuccess || hipMalloc(&dword, 4) != hipSuccess)
            return 6;
        (void)hipMemset(dsrc, 9, (size_t)pitch * h);
        (void)hipMemset(da, 9, (size_t)pitch * h);
        (void)hipMemset(db, 9, (size_t)pitch * h);
        (void)hipMemcpy2D(dsrc, pitch, mask.data(), w, w, h, hipMemcpyHostToDevice);
        const tbdk::GpuImage src{dsrc, w, h, pitch}, a{da, w, h, pitch}, b{db, w, h, pitch};
        tbdk::FusedThreshold ft;
        ft.thresh = 10;
        int thrown = 0;
        try {
            tbdk::FusedThreshold otsu = ft;
            otsu.type = tbdk::THRESH_BINARY | tbdk::THRESH_OTSU;
            tbdk::GaussianBlur(ctx, src, a, tbdk::Size{11, 11}, 3.5, 3.5, TBDK_BORDER_REFLECT_101, nullptr, &otsu);
        } catch (const tbdk::Error& e) {
            thrown += e.code() == TBDK_EINVAL;
        }
        if (thrown != 1) return 7;
        tbdk::GaussianBlur(ctx, src, a, tbdk::Size{11, 11}, 3.5, 3.5);
        tbdk::GaussianBlur(ctx, src, b, tbdk::Size{11, 11}, 3.5, 3.5, TBDK_BORDER_REFLECT_101, nullptr, &ft);
        std::vector<uint8_t> pa((size_t)pitch * h), pb(pa.size()), pc(pa.size());
        if (hipDeviceSynchronize() != hipSuccess) return 8;
        (void)hipMemcpy(pa.data(), da, pa.size(), hipMemcpyDeviceToHost);
        const tbdk::GpuMatView av{da, w, h, pitch, tbdk::DEPTH_8U, 1};
        const double nan = tbdk::threshold(ctx, av, av, 0, 255, tbdk::THRESH_BINARY | tbdk::THRESH_OTSU, nullptr, dword);
        if (nan == nan) return 9;  // the value exists on the device only
        (void)hipMemcpy(da, pa.data(), pa.size(), hipMemcpyHostToDevice);
        if (tbdk::threshold(ctx, av, av, 10.7, 255, tbdk::THRESH_BINARY) != 10.0) return 10;
        if (hipDeviceSynchronize() != hipSuccess) return 11;
        int32_t word = -1;
        (void)hipMemcpy(pb.data(), db, pb.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpy(pc.data(), da, pc.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpy(&word, dword, 4, hipMemcpyDeviceToHost);
        FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 12;
        for (const std::vector<uint8_t>* p : {&pa, &pb, &pc})
            for (int r = 0; r < h; ++r) {
                std::fwrite(p->data() + (size_t)r * pitch, 1, w, o);
                for (int x = w; x < pitch; ++x)
                    if ((*p)[(size_t)r * pitch + x] != 9) return 13;  // the padding was written
            }
        std::fwrite(&word, 4, 1, o);
        if (std::fclose(o) != 0) return 14;
        std::printf("facade GaussianBlur and threshold: ok\n");
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("%s\n", e.what());
        return want_gpu ? 1 : (e.code() == TBDK_ENODEV ? 0 : 2);
    }
}
