// lk_int_origin_check.cpp — the integer-origin level setup of the PyrLK kernels
// (opencv_amd/csrc/lk_int_origin.hpp, the text the kernels compile) against a
// direct restatement on the CPU: the reference's calcSharrDeriv
// (lkpyramid.cpp:55-144) of the window column, then the general setup's
// bilinear with the weights (16384, 0, 0, 0) and its packing by row pairs.
// Built by tests/test_lk_int_origin_host.py with ASan + UBSan.
//   * the two identities: (16384 I + 256) >> 9 == 32 I for every I in 0..255,
//     (16384 v + 8192) >> 14 == v for every v in [-4080, 4080];
//   * window heights 7 .. 31, odd and even, both I forms (ic / packed pairs):
//     all 512 neighbourhoods of 3 x 3 pixels from {0, 255} (tiled down the
//     column: the +-4080 extremes, the modulo-2^16 wrap of the u16 terms),
//     0/255 stripes and checkerboards, flat columns, 8000 random columns per
//     height (2 * 10^5 in all); the byte of column x + 2 and the row below the
//     window hold random values the setup must not read into its result;
//   * a lane that owns no column (factors(false)) gets zero Ix / Iy pairs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "lk_int_origin.hpp"

using namespace tbdk::lkint;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()  // splitmix64
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long g_bad = 0, g_cols = 0;
static int g_min = 0, g_max = 0;  // the derivative extremes met

constexpr int W_BITS1 = 14, RND9 = 1 << (W_BITS1 - 5 - 1), RND14 = 1 << (W_BITS1 - 1);

static uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

// px[j][c]: source row j (level row ipy - 1 + j), column x - 1 + c
template <int WH>
static void check_column(const uint8_t (&px)[WH + 3][4], const char* what)
{
    constexpr int NP = (WH + 1) / 2;
    // the restatement: calcSharrDeriv at (r, x), r < WH, from source rows r .. r+2
    int I[WH], Ix[WH], Iy[WH];
    for (int r = 0; r < WH; ++r) {
        int t0[3], t1[3];  // the vertical pass at columns x-1, x, x+1
        for (int c = 0; c < 3; ++c) {
            const int a = px[r][c], b = px[r + 1][c], d = px[r + 2][c];
            t0[c] = (a + d) * 3 + b * 10;
            t1[c] = d - a;
        }
        Ix[r] = (short)(t0[2] - t0[0]);
        Iy[r] = (short)((t1[2] + t1[0]) * 3 + t1[1] * 10);
        I[r] = px[r + 1][1];
        g_min = Ix[r] < g_min ? Ix[r] : g_min;
        g_min = Iy[r] < g_min ? Iy[r] : g_min;
        g_max = Ix[r] > g_max ? Ix[r] : g_max;
        g_max = Iy[r] > g_max ? Iy[r] : g_max;
    }
    // the general setup with iw00 = 16384, iw01 = iw10 = iw11 = 0
    int ic_ref[WH];
    uint32_t ipk_ref[NP], gx_ref[NP], gy_ref[NP];
    auto i32 = [&](int r) { return r < WH ? (I[r] * 16384 + RND9) >> (W_BITS1 - 5) : 0; };
    auto d14 = [&](const int* v, int r) { return r < WH ? (v[r] * 16384 + RND14) >> W_BITS1 : 0; };
    for (int r = 0; r < WH; ++r) ic_ref[r] = RND9 - (i32(r) << 9);
    for (int q = 0; q < NP; ++q) {
        ipk_ref[q] = pack16(i32(2 * q), i32(2 * q + 1));
        gx_ref[q] = pack16(d14(Ix, 2 * q), d14(Ix, 2 * q + 1));
        gy_ref[q] = pack16(d14(Iy, 2 * q), d14(Iy, 2 * q + 1));
    }

    uint32_t u[WH + 3];
    for (int j = 0; j < WH + 3; ++j)
        u[j] = px[j][0] | (uint32_t)px[j][1] << 8 | (uint32_t)px[j][2] << 16 | (uint32_t)px[j][3] << 24;
    int ic[WH];
    uint32_t ipk[NP], gxk[NP], gyk[NP], gxk1[NP], gyk1[NP], none[1];
    column<WH, 0>(u, factors(true), RND9, ic, none, gxk, gyk);
    column<WH, 1>(u, factors(true), RND9, nullptr, ipk, gxk1, gyk1);
    bool ok = true;
    for (int r = 0; r < WH; ++r) ok &= ic[r] == ic_ref[r];
    for (int q = 0; q < NP; ++q)
        ok &= ipk[q] == ipk_ref[q] && gxk[q] == gx_ref[q] && gyk[q] == gy_ref[q] && gxk1[q] == gx_ref[q] &&
              gyk1[q] == gy_ref[q];
    column<WH, 0>(u, factors(false), RND9, ic, none, gxk, gyk);
    for (int q = 0; q < NP; ++q) ok &= gxk[q] == 0 && gyk[q] == 0;
    ++g_cols;
    if (!ok && g_bad++ < 10) std::printf("MISMATCH WH %d (%s)\n", WH, what);
}

template <int WH>
static void fill_unread(uint8_t (&px)[WH + 3][4])
{
    for (int j = 0; j < WH + 3; ++j) px[j][3] = (uint8_t)rnd();
    for (int c = 0; c < 4; ++c) px[WH + 2][c] = (uint8_t)rnd();
}

template <int WH>
static void check_height()
{
    uint8_t px[WH + 3][4];
    for (int pat = 0; pat < 512; ++pat) {  // a 3 x 3 neighbourhood from {0, 255}, tiled down the column
        for (int j = 0; j < WH + 3; ++j)
            for (int c = 0; c < 3; ++c) px[j][c] = (pat >> (3 * (j % 3) + c)) & 1 ? 255 : 0;
        fill_unread<WH>(px);
        check_column<WH>(px, "3x3");
    }
    for (int kind = 0; kind < 12; ++kind) {  // stripes, checkerboards (cells of 1 and 2), flat
        for (int j = 0; j < WH + 3; ++j)
            for (int c = 0; c < 3; ++c) {
                const int ph = kind & 1;
                int on;
                switch (kind >> 1) {
                case 0: on = (c + ph) & 1; break;                       // vertical stripes
                case 1: on = (j + ph) & 1; break;                       // horizontal stripes
                case 2: on = (j + c + ph) & 1; break;                   // checkerboard
                case 3: on = ((j >> 1) + ph) & 1; break;                // horizontal stripes, 2 rows
                case 4: on = ((j >> 1) + c + ph) & 1; break;            // checkerboard, 2-row cells
                default: on = ph; break;                                // flat 0 / flat 255
                }
                px[j][c] = on ? 255 : 0;
            }
        fill_unread<WH>(px);
        check_column<WH>(px, "pattern");
    }
    for (int n = 0; n < 8000; ++n) {
        const int mode = n & 3;  // any byte; {0, 255}; near-saturated; smooth
        for (int j = 0; j < WH + 3; ++j)
            for (int c = 0; c < 3; ++c) {
                const uint64_t v = rnd();
                px[j][c] = mode == 0 ? (uint8_t)v : mode == 1 ? ((v & 1) ? 255 : 0)
                         : mode == 2 ? (uint8_t)((v & 1) ? 250 + (v >> 8) % 6 : (v >> 8) % 6)
                                     : (uint8_t)(100 + 8 * j + 3 * c + (v >> 8) % 5);
            }
        fill_unread<WH>(px);
        check_column<WH>(px, "random");
    }
}

template <int WH, int LAST>
struct Heights {
    static void run()
    {
        check_height<WH>();
        Heights<WH + 1, LAST>::run();
    }
};
template <int LAST>
struct Heights<LAST, LAST> {
    static void run() { check_height<LAST>(); }
};

int main()
{
    for (int I = 0; I <= 255; ++I)
        if (((16384 * I + RND9) >> 9) != 32 * I) ++g_bad;
    for (int v = -4080; v <= 4080; ++v)
        if (((16384 * v + RND14) >> 14) != v) ++g_bad;
    if (g_bad) std::printf("identity failed\n");
    Heights<7, 31>::run();
    std::printf("columns %ld, derivative range [%d, %d], mismatches %ld\n", g_cols, g_min, g_max, g_bad);
    if (g_bad || g_min != -4080 || g_max != 4080 || g_cols < 100000) return 1;
    std::printf("lk int origin ok\n");
    return 0;
}
