// knn_core_check.cpp — opencv_amd/csrc/knn_core.hpp on the host, as a stand-alone program
// (tests/test_knn_core_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer
// and -ffp-contract=off).
//
//   knn_core_check cases <cases.bin> <out.bin>
// runs BackgroundSubtractorKNN sequentially over the cases of a binary file, with the model in
// the reference's layout, and writes every mask, the requested background images, the model,
// counters and RNG state after the last frame, the branch counts and every frame's periods.
// Each fill is made twice: lane by lane (64 to a block) from jump-ahead starts, as the kernel
// makes it, and sequentially; the two must agree (exit 3 otherwise).
// cases.bin: int32 ncases; per case int32 {w, h, cn, n, history, nsamples, knn_samples,
// detect_shadows, shadow_value}, float {dist2_threshold, shadow_threshold}, uint64 rng_state,
// n doubles (learning rates), n bytes (1: background after this frame), the n frames.
// out.bin: per case the n masks, the backgrounds, samples, index3, next3, int32 counters[3],
// uint64 state, 11 int64 counts (Counts, then fills small / bits / div), n x 3 int32 periods.
//
//   knn_core_check jump <pairs>
// the jump-ahead against sequential stepping for <pairs> random (state, n), the block and lane
// forms against the same, the Montgomery product against the 128-bit remainder, the two fixed
// points, and a constructed ambiguous start; prints "jump ok <pairs>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../opencv_amd/csrc/knn_core.hpp"

using namespace tbdk::knn_core;

static void rd(FILE* f, void* p, size_t n)
{
    if (n && std::fread(p, 1, n, f) != n) {
        std::fprintf(stderr, "short read\n");
        std::exit(2);
    }
}
static void wr(FILE* f, const void* p, size_t n)
{
    if (n && std::fwrite(p, 1, n, f) != n) {
        std::fprintf(stderr, "short write\n");
        std::exit(2);
    }
}
static void fail(const char* what)
{
    std::fprintf(stderr, "%s\n", what);
    std::exit(3);
}

struct Case {
    int w, h, cn, n;
    Settings s;
    uint64_t seed;
    std::vector<double> rates;
    std::vector<unsigned char> bg;
    std::vector<unsigned char> frames;
};

// the fill as knn_randu_kernel makes it: every lane of every block from its own jump-ahead start
static uint64_t fill_by_blocks(const RanduPlan& plan, const JumpTables& jt, uint64_t state, uint8_t* arr, int64_t total)
{
    const bool small = plan.mode == RANDU_SMALL;
    const int64_t nblocks = (total + kRngBlock - 1) / kRngBlock;
    uint64_t end = state;
    int ends = 0;
    for (int64_t b = nblocks - 1; b >= 0; --b) {  // any order
        const int len = (int)(total - b * kRngBlock < kRngBlock ? total - b * kRngBlock : kRngBlock);
        uint8_t* a = arr + b * kRngBlock;
        for (int lane = kLanes - 1; lane >= 0; --lane) {
            bool last = false;
            const uint64_t st = randu_lane(plan, small ? jt.p256 : jt.p1024, small ? jt.p4 : jt.p16, state, (uint32_t)b,
                                           lane, len, &last, [a](int i, uint8_t v) { a[i] = v; });
            if (last && b == nblocks - 1) end = st, ends++;
        }
    }
    if (ends != 1) fail("not exactly one lane ends the plane");
    return end;
}

template <int CN>
static void run_case(const Case& c, const JumpTables& jt, FILE* out)
{
    const size_t px = (size_t)c.w * c.h, nd = CN + 1, per_px = 3 * (size_t)c.s.nsamples * nd;
    std::vector<uint8_t> model(px * per_px), index(3 * px), next(3 * px), mask(px), bgs, tmp(px);
    Counts cnt;
    std::memset(&cnt, 0, sizeof(cnt));
    int64_t fills[3] = {0, 0, 0};
    HostState host = {};
    uint64_t state = c.seed;
    std::vector<int32_t> periods;
    for (int t = 0; t < c.n; ++t) {
        FramePlan plan;
        if (!plan_frame(host, c.s.history, c.s.nsamples, c.rates[t], &plan)) fail("a case with an undefined rate");
        if (plan.reinit) {
            std::fill(model.begin(), model.end(), 0);
            std::fill(index.begin(), index.end(), 0);
            std::fill(next.begin(), next.end(), 0);
        }
        const FrameParams p = frame_params(c.s, plan);
        const uint8_t* fr = c.frames.data() + (size_t)t * px * CN;
        for (size_t i = 0; i < px; ++i) {
            uint8_t idx[3] = {index[i], index[px + i], index[2 * px + i]};
            const uint8_t nxt[3] = {next[i], next[px + i], next[2 * px + i]};
            mask[i] = update_pixel<CN>(model.data() + i * per_px, idx, nxt, fr + i * CN, p, &cnt);
            index[i] = idx[0], index[px + i] = idx[1], index[2 * px + i] = idx[2];
        }
        wr(out, mask.data(), px);
        for (int k = 0; k < 3; ++k) {
            periods.push_back(plan.periods[k]);
            if (!plan.fill[k]) continue;
            const RanduPlan rp = randu_plan(plan.periods[k]);
            fills[rp.mode]++;
            const uint64_t a = fill_by_blocks(rp, jt, state, next.data() + k * px, (int64_t)px);
            const uint64_t b = randu_fill(rp, state, tmp.data(), (int64_t)px);
            if (a != b || std::memcmp(tmp.data(), next.data() + k * px, px) != 0) fail("the block-wise fill differs");
            state = a;
        }
        host = plan.after;
        if (c.bg[t]) {
            const size_t at = bgs.size();
            bgs.resize(at + px * CN);
            for (size_t i = 0; i < px; ++i) background_pixel<CN>(model.data() + i * per_px, c.s.nsamples, &bgs[at + i * CN]);
        }
    }
    wr(out, bgs.data(), bgs.size());
    wr(out, model.data(), model.size());
    wr(out, index.data(), index.size());
    wr(out, next.data(), next.size());
    wr(out, host.counters, sizeof(host.counters));
    wr(out, &state, sizeof(state));
    wr(out, &cnt, sizeof(cnt));
    wr(out, fills, sizeof(fills));
    wr(out, periods.data(), periods.size() * sizeof(int32_t));
}

static int run_cases(const char* in_path, const char* out_path)
{
    FILE* in = std::fopen(in_path, "rb");
    FILE* out = std::fopen(out_path, "wb");
    if (!in || !out) return 2;
    JumpTables jt;
    jump_tables(&jt);
    int32_t ncases = 0;
    rd(in, &ncases, 4);
    for (int i = 0; i < ncases; ++i) {
        Case c;
        int32_t v[9];
        float f[2];
        rd(in, v, sizeof(v));
        rd(in, f, sizeof(f));
        rd(in, &c.seed, 8);
        c.w = v[0], c.h = v[1], c.cn = v[2], c.n = v[3];
        c.s.history = v[4], c.s.nsamples = v[5], c.s.knn_samples = v[6], c.s.detect_shadows = v[7], c.s.shadow_value = v[8];
        c.s.dist2_threshold = f[0], c.s.shadow_threshold = f[1];
        if (c.s.nsamples < 1 || c.s.nsamples > kMaxSamples || (c.cn != 1 && c.cn != 3)) return 2;
        c.rates.resize(c.n);
        c.bg.resize(c.n);
        c.frames.resize((size_t)c.n * c.w * c.h * c.cn);
        rd(in, c.rates.data(), sizeof(double) * c.n);
        rd(in, c.bg.data(), c.n);
        rd(in, c.frames.data(), c.frames.size());
        if (c.cn == 1)
            run_case<1>(c, jt, out);
        else
            run_case<3>(c, jt, out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("cases %d\n", ncases);
    return 0;
}

static uint64_t g_x = 0x243f6a8885a308d3ull;
static uint64_t rnd()
{
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}

static uint64_t step_n(uint64_t x, uint64_t n)
{
    for (; n; --n) x = rng_next(x);
    return x;
}

static int run_jump(long pairs)
{
    __extension__ typedef unsigned __int128 u128;
    JumpTables jt;
    jump_tables(&jt);
    for (long i = 0; i < pairs; ++i) {
        uint64_t x = rnd();
        switch (i & 7) {  // whole range; above m; small residues; just after a step
        case 1: x = kRngM + rnd() % (~0ull - kRngM + 1); break;
        case 2: x = rnd() % (2 * kRngSlack); break;
        case 3: x = rng_next(x); break;
        default: break;
        }
        const uint64_t n = rnd() % 4097;
        if (jump(x, n) != step_n(x, n)) fail("jump differs from stepping");
        const uint64_t a = rnd() % kRngM, b = rnd() % kRngM;
        if (montmul(a, to_mont(b)) != (uint64_t)((u128)a * b % kRngM)) fail("montmul");
        if ((i & 63) == 0) {
            const uint32_t blk = (uint32_t)(rnd() % 40), lane = (uint32_t)(rnd() % kLanes);
            if (jump_units(x, blk, 256, jt.p256, kJumpBits) != step_n(x, 256ull * blk)) fail("jump_units 256");
            if (jump_units(x, blk, 1024, jt.p1024, kJumpBits) != step_n(x, 1024ull * blk)) fail("jump_units 1024");
            if (jump_units(x, lane, 4, jt.p4, kLaneBits) != step_n(x, 4ull * lane)) fail("jump_units 4");
            if (jump_units(x, lane, 16, jt.p16, kLaneBits) != step_n(x, 16ull * lane)) fail("jump_units 16");
        }
    }
    // the product at the ends of its range
    const uint64_t ends[] = {0, 1, 2, kRngSlack, kRngM - 2, kRngM - 1};
    for (uint64_t a : ends)
        for (uint64_t b : ends)
            if (montmul(a, to_mont(b)) != (uint64_t)((u128)a * b % kRngM)) fail("montmul at the ends");
    // far blocks: against the single-step form of the same rule
    for (int k = 0; k < 64; ++k) {
        const uint64_t x = rnd();
        const uint32_t blk = (uint32_t)(rnd() >> 40);
        if (jump_units(x, blk, 1024, jt.p1024, kJumpBits) != jump(x, 1024ull * blk)) fail("jump_units far");
    }
    // the fixed points
    for (uint64_t n = 0; n < 5000; n += 1237) {
        if (jump(0, n) != 0 || jump(kRngM, n) != kRngM) fail("fixed point");
        if (jump_units(0, (uint32_t)n, 256, jt.p256, kJumpBits) != 0 ||
            jump_units(kRngM, (uint32_t)n, 1024, jt.p1024, kJumpBits) != kRngM)
            fail("fixed point by blocks");
    }
    if (rng_next(0) != 0 || rng_next(kRngM) != kRngM) fail("fixed point step");
    // an ambiguous start: the successor of this state is m + 5, whose residue 5 is also the state 5
    const uint64_t amb = 0xf83f630effffffffull;
    if (rng_next(amb) != kRngM + 5) fail("the constructed state");
    if (jump(amb, 1) != kRngM + 5) fail("ambiguous start");
    if (jump(amb, 2) != rng_next(kRngM + 5) || jump(amb, 700) != step_n(amb, 700)) fail("after the ambiguous start");
    // the same through blocks: a state whose 256th successor's residue is small cannot be built by hand, so the
    // fallback's stepping is exercised with a table that makes every residue ambiguous (all ones, in Montgomery
    // form: r = r0 = 3)
    uint64_t ones[kJumpBits];
    for (int k = 0; k < kJumpBits; ++k) ones[k] = to_mont(1);
    if (jump_units(3, 3, 256, ones, kJumpBits) != step_n(3, 768)) fail("fallback by blocks");
    std::printf("jump ok %ld\n", pairs);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "cases")) return run_cases(argv[2], argv[3]);
    if (argc == 3 && !std::strcmp(argv[1], "jump")) return run_jump(std::atol(argv[2]));
    std::fprintf(stderr, "usage: knn_core_check cases <cases.bin> <out.bin> | jump <pairs>\n");
    return 2;
}
