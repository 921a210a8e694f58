// blur_host_check.cpp — opencv_amd/csrc/blur_host.hpp (the 8.8 Gaussian coefficients, GaussianBlur's kernel-size
// rules and threshold's 8-bit parameter rules, which blur.hip plans its launches with) as a stand-alone host
// program, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_blur_host.py.
//   blur_host_check <cases.bin> <out.bin>
// cases.bin: int32 count, then per case int32 kind and
//   kind 0 (coefficients): int32 n, float64 sigma            -> int32 ok, then n uint16 if ok
//   kind 1 (plan): int32 width, height, kw, kh, border, float64 sigma_x, sigma_y
//                                                            -> int32 ok, copy, kw, kh, 31 + 31 uint16
//   kind 2 (threshold): int32 type, float64 thresh, maxval   -> int32 ok, ithresh, hi, lo, special
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../opencv_amd/csrc/blur_host.hpp"

using namespace tbdk::blur_host;

static bool get(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    int32_t count = 0;
    if (!in || !out || !get(in, &count, 4)) return 3;
    for (int32_t c = 0; c < count; ++c) {
        int32_t kind = 0;
        if (!get(in, &kind, 4)) return 4;
        if (kind == 0) {
            int32_t n = 0;
            double sigma = 0;
            if (!get(in, &n, 4) || !get(in, &sigma, 8)) return 5;
            // exactly n words: the sanitizer sees a write past them
            std::vector<uint16_t> k(n > 0 ? (size_t)n : 0);
            const int32_t ok = gaussian_kernel_u8(n, sigma, k.empty() ? nullptr : k.data());
            std::fwrite(&ok, 4, 1, out);
            if (ok) std::fwrite(k.data(), 2, k.size(), out);
        } else if (kind == 1) {
            int32_t a[5];
            double s[2];
            if (!get(in, a, 20) || !get(in, s, 16)) return 6;
            BlurPlan p;
            const int32_t ok = make_plan(a[0], a[1], a[2], a[3], s[0], s[1], a[4], &p);
            const int32_t head[4] = {ok, p.copy, p.kw, p.kh};
            std::fwrite(head, 4, 4, out);
            std::fwrite(p.kx, 2, kMaxK, out);
            std::fwrite(p.ky, 2, kMaxK, out);
        } else {
            int32_t type = 0;
            double v[2];
            if (!get(in, &type, 4) || !get(in, v, 16)) return 7;
            ThreshPlan p = {0, 0, 0};
            const int32_t ok = thresh_plan_u8(v[0], v[1], type, &p);
            const int32_t head[5] = {ok, p.ithresh, p.hi_const, p.lo_const, ok ? thresh_special(p.ithresh, type) : 0};
            std::fwrite(head, 4, 5, out);
        }
    }
    if (std::fclose(out) != 0) return 8;
    std::printf("cases %d\n", (int)count);
    return 0;
}
