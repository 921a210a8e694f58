// blobs_host_check.cpp — opencv_amd/csrc/morph_host.hpp (getStructuringElement, the anchor rule and morphOp's
// iteration rules, which morph.hip plans its launches with) as a stand-alone host program, built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_blobs_host.py.
//   blobs_host_check <cases.bin> <out.bin>
// cases.bin: int32 count, then per case int32 kind and
//   kind 0 (element): shape, kw, kh, ax, ay              -> int32 ok, then kw * kh bytes if ok
//   kind 1 (plan):    has_element, kw, kh, ax, ay, iterations, then kw * kh bytes if has_element
//                                                        -> int32 ok, copy, rect, kw, kh, ax, ay, passes, 31 row masks
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../opencv_amd/csrc/morph_host.hpp"

using namespace tbdk::morph_host;

static bool get(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    int32_t count = 0;
    if (!in || !out || !get(in, &count, 4)) return 3;
    for (int32_t c = 0; c < count; ++c) {
        int32_t kind = 0, a[6];
        if (!get(in, &kind, 4)) return 4;
        if (kind == 0) {
            if (!get(in, a, 20)) return 5;
            // exactly kw * kh bytes: the sanitizer sees a write past the element
            std::vector<uint8_t> e(a[1] > 0 && a[2] > 0 ? (size_t)a[1] * a[2] : 0);
            const int32_t ok = structuring_element(a[0], a[1], a[2], a[3], a[4], e.empty() ? nullptr : e.data());
            std::fwrite(&ok, 4, 1, out);
            if (ok) std::fwrite(e.data(), 1, e.size(), out);
        } else {
            if (!get(in, a, 24)) return 6;
            std::vector<uint8_t> e(a[0] ? (size_t)a[1] * a[2] : 0);
            if (!e.empty() && !get(in, e.data(), e.size())) return 7;
            Plan p;
            const int32_t ok = make_plan(a[0] ? e.data() : nullptr, a[1], a[2], a[3], a[4], a[5], &p);
            const int32_t head[8] = {ok, p.copy, p.rect, p.kw, p.kh, p.ax, p.ay, p.passes};
            std::fwrite(head, 4, 8, out);
            std::fwrite(p.rows, 4, kMaxSide, out);
        }
    }
    if (std::fclose(out) != 0) return 8;
    std::printf("cases %d\n", (int)count);
    return 0;
}
