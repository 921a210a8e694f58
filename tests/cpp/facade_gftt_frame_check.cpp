// facade_gftt_frame_check.cpp — compiles the C++ facade's whole-frame corner
// detection (include/tbdk.hpp: tbdk::cuda::CornersDetector::detect) against
// libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV)
//   GPU    : facade_gftt_frame_check gpu <frame.u8> <width> <height> <maxCorners>
//            <quality> <minDistance> <corners.f32>: detect on the frame (raw 8-bit
//            rows) gives exactly the corners of the file (float32 pairs, the list
//            the Python binding returned): same count, same positions, same order;
//            the same through a typed view, and with the context option
//            "gftt_wide" = 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

namespace {

template <typename T>
std::vector<T> slurp(const char* path)
{
    std::vector<T> v;
    if (FILE* f = std::fopen(path, "rb")) {
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        v.resize(n > 0 ? (size_t)n / sizeof(T) : 0);
        if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
        std::fclose(f);
    }
    return v;
}

}  // namespace

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        if (argc != 9) return 2;
        const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), maxc = std::atoi(argv[5]);
        const double q = std::atof(argv[6]), md = std::atof(argv[7]);
        const std::vector<uint8_t> frame = slurp<uint8_t>(argv[2]);
        const std::vector<float> want = slurp<float>(argv[8]);
        if (W <= 0 || H <= 0 || maxc <= 0 || frame.size() != (size_t)W * H || want.empty() || want.size() % 2) return 2;
        uint8_t* d8 = nullptr;
        float* dc = nullptr;
        int32_t* dn = nullptr;
        if (hipMalloc(&d8, frame.size()) || hipMalloc(&dc, (size_t)maxc * 8) || hipMalloc(&dn, 4)) return 4;
        (void)hipMemcpy(d8, frame.data(), frame.size(), hipMemcpyHostToDevice);
        auto det = tbdk::cuda::CornersDetector::create(ctx, maxc, q, md);
        const tbdk::GpuImage img{d8, W, H, W};
        const tbdk::GpuMatView view{d8, W, H, W, tbdk::DEPTH_8U, 1};
        std::vector<float> got((size_t)maxc * 2);
        for (int pass = 0; pass < 3; ++pass) {  // GpuImage, typed view, every ROI through the wide path
            (void)hipMemset(dc, 0, (size_t)maxc * 8);
            (void)hipMemset(dn, 0xFF, 4);
            if (pass == 2) tbdk::check(tbdk_ctx_set_option(ctx.get(), "gftt_wide", 1), "gftt_wide");
            if (pass == 1) det->detect(view, dc, dn);
            else det->detect(img, dc, dn);
            int32_t n = 0;
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(&n, dn, 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(got.data(), dc, (size_t)maxc * 8, hipMemcpyDeviceToHost);
            std::printf("pass %d: %d corners (expected %zu)\n", pass, n, want.size() / 2);
            if (n < 0 || (size_t)n != want.size() / 2) return 6;
            if (std::memcmp(got.data(), want.data(), want.size() * 4) != 0) return 7;
        }
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 5;
    }
}
