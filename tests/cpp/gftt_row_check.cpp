// The identities the GFTT eigenvalue walk's row arithmetic rests on
// (opencv_amd/csrc/gftt_row_math.hpp, the text klt_gftt.hip compiles), checked on
// the host: a stand-alone program, meant to be compiled with
// -fsanitize=address,undefined -ffp-contract=off.
//  1. sobel_row (rx = s2 - s0) equals the literal three-tap form for all 256^3
//     (s0, s1, s2), bit for bit;
//  2. over 5 x 5 neighbourhoods of 8-bit and 16-bit pixels (the nine 3 x 3
//     neighbourhoods of a box sum; random, flat, saturated, steps, single pixels,
//     checkerboards, every corner pattern of {0, max}), the gradient pair without
//     the "+ 0.f", the covariances and the min eigenvalue of their box sums equal
//     the literal form's, bit for bit; no dx, dy or e is -0, and no e is NaN or
//     infinite;
//  3. fkey(max(a, b)) == max(fkey(a), fkey(b)) over those e (and the running
//     float maximum's key equals the running key maximum).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gftt_row_math.hpp"

using namespace tbdk;

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static int fkey(float f) { return fkey_bits((int)bits(f)); }

static long long g_bad = 0;
static void fail(const char* what)
{
    if (g_bad++ < 10) std::printf("MISMATCH: %s\n", what);
}

struct Mode {
    bool u16;
    float k, k2;
    int vmax;
};

// the three cov channels of the 3 x 3 centre pixels of a 5 x 5 patch and the min
// eigenvalue of their box sums ((l + c) + r per row in double, rows from the
// top as the running column sum starts: (0 + r0) + r1, then + r2)
template <bool LIT>
static float patch_eig(const Mode& m, const float (&px)[5][5], float (&grad)[3][3][2])
{
    SobelRow sr[5][3];  // image row y, centre columns 1..3
    for (int y = 0; y < 5; ++y)
        for (int x = 0; x < 3; ++x) {
            const float s0 = px[y][x], s1 = px[y][x + 1], s2 = px[y][x + 2];
            if (m.u16) sr[y][x] = sobel_row_f32(s0, s1, s2, m.k, m.k2);
            else sr[y][x] = LIT ? sobel_row_lit(s0, s1, s2, m.k, m.k2) : sobel_row(s0, s1, s2, m.k, m.k2);
        }
    double rows[3][3];  // cov row sums, [row][channel]
    for (int y = 0; y < 3; ++y) {
        float cv[3][3];  // [channel][column]
        for (int x = 0; x < 3; ++x) {
            const Grad g = LIT ? grad_lit(sr[y][x], sr[y + 1][x], sr[y + 2][x], m.k, m.k2)
                               : grad_int(sr[y][x], sr[y + 1][x], sr[y + 2][x], m.k, m.k2);
            grad[y][x][0] = g.dx;
            grad[y][x][1] = g.dy;
            cv[0][x] = g.dx * g.dx;
            cv[1][x] = g.dx * g.dy;
            cv[2][x] = g.dy * g.dy;
        }
        for (int ch = 0; ch < 3; ++ch) rows[y][ch] = (double)cv[ch][0] + (double)cv[ch][1] + (double)cv[ch][2];
    }
    float box[3];
    for (int ch = 0; ch < 3; ++ch) box[ch] = (float)(((0.0 + rows[0][ch]) + rows[1][ch]) + rows[2][ch]);
    return min_eig(box[0], box[1], box[2]);
}

static std::vector<float> g_e;

static void check_patch(const Mode& m, const float (&px)[5][5])
{
    float ga[3][3][2], gb[3][3][2];
    const float ea = patch_eig<true>(m, px, ga), eb = patch_eig<false>(m, px, gb);
    for (int y = 0; y < 3; ++y)
        for (int x = 0; x < 3; ++x)
            for (int c = 0; c < 2; ++c) {
                if (bits(ga[y][x][c]) != bits(gb[y][x][c])) fail("dx / dy differ");
                if (bits(gb[y][x][c]) == 0x80000000u || bits(ga[y][x][c]) == 0x80000000u) fail("dx / dy is -0");
                // (the covariances are products of equal bits)
            }
    if (bits(ea) != bits(eb)) fail("e differs");
    if (bits(eb) == 0x80000000u) fail("e is -0");
    if (!(eb == eb) || eb - eb != 0.f) fail("e is NaN or infinite");
    g_e.push_back(eb);
}

static void patches(const Mode& m, std::mt19937& rng)
{
    float px[5][5];
    auto fill = [&](auto f) {
        for (int y = 0; y < 5; ++y)
            for (int x = 0; x < 5; ++x) px[y][x] = (float)f(y, x);
        check_patch(m, px);
    };
    // flat (0, 1, mid, max), steps, stripes, checkerboards, single pixels
    for (int v : {0, 1, m.vmax / 2, m.vmax - 1, m.vmax}) fill([&](int, int) { return v; });
    for (int s = 0; s <= 5; ++s)
        for (int lo : {0, 1, m.vmax - 1}) {
            fill([&](int, int x) { return x < s ? lo : m.vmax; });
            fill([&](int, int x) { return x < s ? m.vmax : lo; });
            fill([&](int y, int) { return y < s ? lo : m.vmax; });
            fill([&](int y, int) { return y < s ? m.vmax : lo; });
            fill([&](int y, int x) { return x + y < s + 2 ? lo : m.vmax; });
        }
    for (int ph = 0; ph < 2; ++ph) {
        fill([&](int y, int x) { return ((x + y + ph) & 1) ? m.vmax : 0; });
        fill([&](int, int x) { return ((x + ph) & 1) ? m.vmax : 0; });
        fill([&](int y, int) { return ((y + ph) & 1) ? m.vmax : 0; });
        fill([&](int y, int x) { return ((x + y + ph) & 1) ? 1 : 0; });
    }
    for (int py = 0; py < 5; ++py)
        for (int pxl = 0; pxl < 5; ++pxl)
            for (int v : {1, m.vmax}) {
                fill([&](int y, int x) { return y == py && x == pxl ? v : 0; });
                fill([&](int y, int x) { return y == py && x == pxl ? 0 : v; });
            }
    // every pattern of {0, max} (and {max - 1, max}) over the 3 x 3 centre, the ring 0 / max
    for (int pat = 0; pat < 512; ++pat)
        for (int ring : {0, m.vmax})
            for (int lo : {0, m.vmax - 1})
                fill([&](int y, int x) {
                    if (y < 1 || y > 3 || x < 1 || x > 3) return ring;
                    return ((pat >> ((y - 1) * 3 + (x - 1))) & 1) ? m.vmax : lo;
                });
    // random: full range, {0, max} only, low values, near-flat, near-saturated
    std::uniform_int_distribution<int> full(0, m.vmax), two(0, 1), low(0, 3);
    for (int it = 0; it < 60000; ++it) fill([&](int, int) { return full(rng); });
    for (int it = 0; it < 20000; ++it) fill([&](int, int) { return two(rng) ? m.vmax : 0; });
    for (int it = 0; it < 20000; ++it) fill([&](int, int) { return low(rng); });
    for (int it = 0; it < 20000; ++it) fill([&](int, int) { return m.vmax - low(rng); });
    for (int it = 0; it < 20000; ++it) {
        const int base = full(rng);
        fill([&](int, int) { return base + (base < m.vmax ? two(rng) : 0); });
    }
}

int main()
{
    // cornerEigenValsVecs' scale as the walk computes it (klt_gftt.hip, gftt_eig_body)
    const double s8 = 1.0 / ((double)(1 << 2) * 3 * 255.0), s16 = 1.0 / ((double)(1 << 2) * 3);
    const Mode m8{false, (float)(1.0 * s8), (float)(2.0 * s8), 255};
    const Mode m16{true, (float)(1.0 * s16), (float)(2.0 * s16), 65535};

    // 1. all 256^3 Sobel rows
    for (int a = 0; a < 256; ++a)
        for (int b = 0; b < 256; ++b)
            for (int c = 0; c < 256; ++c) {
                const SobelRow l = sobel_row_lit((float)a, (float)b, (float)c, m8.k, m8.k2);
                const SobelRow n = sobel_row((float)a, (float)b, (float)c, m8.k, m8.k2);
                if (bits(l.rx) != bits(n.rx) || bits(l.ry) != bits(n.ry)) fail("sobel_row differs");
                if (bits(n.rx) == 0x80000000u || bits(n.ry) == 0x80000000u) fail("sobel_row is -0");
            }
    std::printf("sobel rows: 16777216 checked\n");

    // 2. gradients, covariances, eigenvalues
    std::mt19937 rng(20261021u);
    patches(m8, rng);
    const size_t n8 = g_e.size();
    patches(m16, rng);
    std::printf("patches: %zu 8-bit, %zu 16-bit\n", n8, g_e.size() - n8);

    // 3. the key of a float maximum is the maximum of the keys
    std::uniform_int_distribution<size_t> pick(0, g_e.size() - 1);
    for (int it = 0; it < 2000000; ++it) {
        const float a = g_e[pick(rng)], b = g_e[pick(rng)];
        const float mx = std::fmax(a, b);
        const int ka = fkey(a), kb = fkey(b);
        if (fkey(mx) != (ka > kb ? ka : kb)) fail("fkey(max(a, b)) != max(fkey(a), fkey(b))");
    }
    float run = -INFINITY;
    int krun = INT32_MIN;
    for (float e : g_e) {
        run = std::fmax(run, e);
        const int k = fkey(e);
        krun = k > krun ? k : krun;
        if (fkey(run) != krun) {
            fail("running float maximum's key != running key maximum");
            break;
        }
    }
    bool neg = false, pos = false;
    for (float e : g_e) {
        neg |= e < 0.f;
        pos |= e > 0.f;
    }
    if (!pos) fail("no positive e in the sample");
    std::printf("eigenvalues: %zu, negative ones %s\n", g_e.size(), neg ? "present" : "absent");

    if (g_bad) {
        std::printf("gftt row check FAILED: %lld mismatches\n", g_bad);
        return 1;
    }
    std::printf("gftt row check ok\n");
    return 0;
}
