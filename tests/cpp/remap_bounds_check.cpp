// remap_bounds_check.cpp — host walk of the address computation the remap
// kernels run (opencv_amd/csrc/remap_core.hpp), built with
// -fsanitize=address,undefined by tests/test_remap_bounds.py.  Host only.
//
//   remap_bounds_check <cases.bin>
//
// cases.bin holds every case of tests/_remap_cases.py (written by the test):
// per case a header of 12 int32 (front, interpolation, border, sw, sh, dw, dh,
// has map2, sign, bytes of map1, bytes of map2, 0), 9 doubles (the dst -> src
// matrix) and the raw maps.  Every destination pixel goes through decode_* and
// make_taps exactly as remap.hip's kernel calls them, for the case's own
// interpolation and border and then for every other interpolation x border, and
// every tap index must lie inside the source (or be -1 under BORDER_CONSTANT).
// Then the same for a list of hostile floats and every short on sources of 1 to
// 5 pixels, and border_interp's closed form against the reference's loop.
// Exit code 0 = pass; prints the counts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "remap_core.hpp"

namespace rc = tbdk::remap_core;

namespace {

enum { kFrontMap32FC2 = 0, kFrontMap32FC1 = 1, kFrontMap16SC2 = 2, kFrontFlow = 3, kFrontPerspective = 4 };

long long g_pixels = 0, g_taps = 0, g_keep = 0, g_fill = 0, g_outside = 0;

// cv::borderInterpolate as the reference writes it (core/src/copy.cpp)
int border_interp_loop(int p, int len, int border)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (border == rc::kReplicate) return p < 0 ? 0 : len - 1;
    if (border == rc::kReflect || border == rc::kReflect101) {
        const int delta = border == rc::kReflect101;
        if (len == 1) return 0;
        do {
            if (p < 0) p = -p - 1 + delta;
            else p = len - 1 - (p - len) - delta;
        } while ((unsigned)p >= (unsigned)len);
        return p;
    }
    if (border == rc::kWrap) {
        if (p < 0) p -= ((p - len + 1) / len) * len;
        if (p >= len) p %= len;
        return p;
    }
    return -1;
}

template <int INTER>
bool check_pixel(const rc::Coord& c, int sw, int sh, int border)
{
    constexpr int N = rc::TapCount<INTER>::value;
    if (c.sx < -32768 || c.sx > 32767 || c.sy < -32768 || c.sy > 32767 || (unsigned)c.ax > 31u || (unsigned)c.ay > 31u) {
        std::printf("coordinate out of range: %d %d %d %d\n", c.sx, c.sy, c.ax, c.ay);
        return false;
    }
    int xs[N], ys[N];
    for (int q = 0; q < N; ++q) xs[q] = ys[q] = std::numeric_limits<int>::min();
    const int what = rc::make_taps<INTER>(c.sx, c.sy, sw, sh, border, xs, ys);
    ++g_pixels;
    if (what == rc::kKeep) {
        ++g_keep;
        return border == rc::kTransparent;
    }
    if (what == rc::kFill) {
        ++g_fill;
        return border == rc::kConstant;
    }
    for (int q = 0; q < N; ++q) {
        for (int t = 0; t < 2; ++t) {
            const int v = t ? ys[q] : xs[q], len = t ? sh : sw;
            ++g_taps;
            if (v == -1 && border == rc::kConstant) continue;  // the border value stands in: no load
            if (v < 0 || v >= len) {
                std::printf("tap outside: inter %d border %d s (%d, %d) size %dx%d tap %d -> %d\n", INTER, border, c.sx,
                            c.sy, sw, sh, q, v);
                ++g_outside;
                return false;
            }
        }
    }
    return true;
}

bool check_all(const rc::Coord& c, int sw, int sh)
{
    bool ok = true;
    for (int border = 0; border < 6; ++border)
        ok = ok && check_pixel<0>(c, sw, sh, border) && check_pixel<1>(c, sw, sh, border) &&
             check_pixel<2>(c, sw, sh, border);
    return ok;
}

bool check_inter(int inter, const rc::Coord& c, int sw, int sh, int border)
{
    return inter == 0 ? check_pixel<0>(c, sw, sh, border)
                      : (inter == 1 ? check_pixel<1>(c, sw, sh, border) : check_pixel<2>(c, sw, sh, border));
}

bool walk_case(const int32_t* h, const double* m, const uint8_t* map1, const uint8_t* map2)
{
    const int front = h[0], sw = h[3], sh = h[4], dw = h[5], dh = h[6];
    int inter = h[1] == 3 ? 1 : h[1];
    const int border = h[2];
    const bool has2 = h[7] != 0;
    const float sign = (float)h[8];
    const int bw0 = rc::perspective_block_width(dw, dh);
    for (int pass = 0; pass < 2; ++pass) {  // the case's own mode, then the coordinates of both decoders in every mode
        for (int y = 0; y < dh; ++y)
            for (int x = 0; x < dw; ++x) {
                for (int nn = 0; nn < 2; ++nn) {
                    const bool nearest = pass == 0 ? inter == 0 : nn == 1;
                    if (pass == 0 && nn == 1) break;
                    rc::Coord c;
                    const size_t i = (size_t)y * dw + x;
                    if (front == kFrontMap32FC2 || front == kFrontFlow) {
                        float v[2];
                        std::memcpy(v, map1 + i * 8, 8);
                        c = front == kFrontFlow ? rc::decode_flow(x, y, v[0], v[1], sign, nearest)
                                                : rc::decode_float(v[0], v[1], nearest);
                    } else if (front == kFrontMap32FC1) {
                        float vx, vy;
                        std::memcpy(&vx, map1 + i * 4, 4);
                        std::memcpy(&vy, map2 + i * 4, 4);
                        c = rc::decode_float(vx, vy, nearest);
                    } else if (front == kFrontMap16SC2) {
                        int16_t v[2];
                        uint16_t f = 0;
                        std::memcpy(v, map1 + i * 4, 4);
                        if (has2) std::memcpy(&f, map2 + i * 2, 2);
                        c = rc::decode_fixed(v[0], v[1], has2, f, nearest);
                    } else {
                        c = rc::decode_perspective(m, bw0, dw, x, y, nearest);
                    }
                    if (pass == 0 ? !check_inter(inter, c, sw, sh, border) : !check_all(c, sw, sh)) {
                        std::printf("  at destination (%d, %d), front %d\n", x, y, front);
                        return false;
                    }
                }
            }
    }
    return true;
}

bool sweeps()
{
    // border_interp: the closed form is the reference's loop
    const int lens[] = {1, 2, 3, 4, 5, 37, 130, 1920, 32766};
    for (int len : lens)
        for (int border = 0; border < 5; ++border)
            for (int p = -33000; p <= 33000; ++p) {
                // the loop takes |p| / len turns: short sources get the near range and both far ends
                if (len < 37 && std::abs(p) > 3000 && std::abs(p) < 32700) continue;
                if (rc::border_interp(p, len, border) != border_interp_loop(p, len, border)) {
                    std::printf("border_interp(%d, %d, %d) = %d, the loop gives %d\n", p, len, border,
                                rc::border_interp(p, len, border), border_interp_loop(p, len, border));
                    return false;
                }
            }
    // hostile floats through both float decoders, every short through the fixed one
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float hostile[] = {nan, -nan, inf, -inf, 1e30f, -1e30f, 40000.f, -40000.f, 3.4e38f, -3.4e38f, 67108864.f,
                             -67108864.f, 2147483648.f, -2147483648.f, 2147483520.f, 1024.f * 32768.f, 32767.f,
                             -32768.f, 32767.5f, -32768.5f, 0.f, -0.f, 1e-40f, 0.5f, 1.f / 64, -1.f / 64};
    const int sizes[] = {1, 2, 3, 4, 5, 32766};
    for (float fx : hostile)
        for (float fy : hostile)
            for (int sw : sizes)
                for (int sh : sizes)
                    for (int nn = 0; nn < 2; ++nn)
                        if (!check_all(rc::decode_float(fx, fy, nn != 0), sw, sh) ||
                            !check_all(rc::decode_flow(32765, 7, fx, fy, -1.f, nn != 0), sw, sh))
                            return false;
    const int few[] = {1, 3, 32766};
    for (int v = -32768; v <= 32767; ++v)
        for (int sw : few)
            for (int f = 0; f < 2; ++f)
                for (int nn = 0; nn < 2; ++nn)
                    if (!check_all(rc::decode_fixed(v, -v - 1, f != 0, f ? 0xFFFFu * (unsigned)(v & 1) + 17u * (unsigned)v : 0u,
                                                    nn != 0),
                                   sw, 5))
                        return false;
    // projective maps with extreme finite entries
    const double big[] = {0.0, 1.0, -1.0, 1e-310, -1e-310, 1e300, -1e300, 1.7e308, 3e8, -1.0 / 64};
    for (double a : big)
        for (double b : big)
            for (double w : big) {
                const double m[9] = {a, b, w, b, a, -w, w, a, b};
                for (int x = 0; x < 70; x += 3)
                    for (int nn = 0; nn < 2; ++nn)
                        if (!check_all(rc::decode_perspective(m, 64, 130, x, x % 7, nn != 0), 5, 3)) return false;
            }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0;
    for (;;) {
        int32_t h[12];
        const size_t got = std::fread(h, 4, 12, f);
        if (got == 0) break;
        double m[9];
        if (got != 12 || std::fread(m, 8, 9, f) != 9 || h[9] < 0 || h[10] < 0) return 3;
        std::vector<uint8_t> map1((size_t)h[9]), map2((size_t)h[10]);
        if ((h[9] && std::fread(map1.data(), 1, map1.size(), f) != map1.size()) ||
            (h[10] && std::fread(map2.data(), 1, map2.size(), f) != map2.size()))
            return 3;
        // the maps must hold what the walk reads
        const size_t px = (size_t)h[5] * h[6];
        const size_t need1 = h[0] == kFrontPerspective ? 0 : px * (h[0] == kFrontMap32FC1 || h[0] == kFrontMap16SC2 ? 4 : 8);
        const size_t need2 = h[0] == kFrontMap32FC1 ? px * 4 : (h[0] == kFrontMap16SC2 && h[7] ? px * 2 : 0);
        if (map1.size() != need1 || map2.size() != need2) return 4;
        if (!walk_case(h, m, map1.data(), map2.data())) {
            std::printf("case %d failed\n", cases);
            return 1;
        }
        ++cases;
    }
    std::fclose(f);
    if (!sweeps()) return 1;
    std::printf("cases %d pixels %lld taps %lld kept %lld filled %lld outside %lld\n", cases, g_pixels, g_taps, g_keep,
                g_fill, g_outside);
    return g_outside == 0 ? 0 : 1;
}
