// mog2_core_check.cpp — opencv_amd/csrc/mog2_core.hpp on the host, as a stand-alone program
// (tests/test_mog2_core_host.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer
// and -ffp-contract=off).  It runs BackgroundSubtractorMOG2 sequentially over the cases of a
// binary file, with the model in the reference's layout, and writes every mask, the requested
// background images, the model after the last frame and the branch counts.
//
//   mog2_core_check <cases.bin> <out.bin>
//
// cases.bin: int32 ncases; per case int32 {w, h, cn, f32, n, history, nmixtures, detect_shadows,
// shadow_value}, double {var_threshold, var_threshold_gen, var_init, var_min, var_max,
// background_ratio, complexity_reduction, shadow_threshold}, n doubles (learning rates), n bytes
// (1: background after this frame), the n frames.
// out.bin: per case the n masks, the backgrounds (frame type), weight, variance, mean, modes_used,
// 11 int64 counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../opencv_amd/csrc/mog2_core.hpp"

using namespace tbdk::mog2_core;

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

struct Case {
    int w, h, cn, f32, n;
    Settings s;
    std::vector<double> rates;
    std::vector<unsigned char> bg;
    std::vector<unsigned char> frames;
};

template <int CN, int K>
static void run_case(const Case& c, FILE* out)
{
    const size_t px = (size_t)c.w * c.h;
    std::vector<float> weight(px * K), variance(px * K), mean(px * K * CN);
    std::vector<unsigned char> modes(px), mask(px);
    Counts cnt;
    std::memset(&cnt, 0, sizeof(cnt));
    const size_t fbytes = px * CN * (c.f32 ? 4 : 1);
    int nframes = 0;
    std::vector<unsigned char> bgs;
    for (int t = 0; t < c.n; ++t) {
        bool reinit = false;
        const double rate = schedule(&nframes, c.s.history, c.rates[t], &reinit);
        if (reinit) {
            std::fill(weight.begin(), weight.end(), 0.f);
            std::fill(variance.begin(), variance.end(), 0.f);
            std::fill(mean.begin(), mean.end(), 0.f);
            std::fill(modes.begin(), modes.end(), 0);
        }
        const FrameParams p = frame_params(c.s, rate);
        const unsigned char* fr = c.frames.data() + fbytes * t;
        for (size_t i = 0; i < px; ++i) {
            float d[CN];
            for (int ch = 0; ch < CN; ++ch) {
                if (c.f32)
                    std::memcpy(&d[ch], fr + (i * CN + ch) * 4, 4);
                else
                    d[ch] = (float)fr[i * CN + ch];
            }
            int nm = modes[i];
            mask[i] = update_pixel<CN, K>(&weight[i * K], &variance[i * K], &mean[i * K * CN], &nm, d, p, &cnt);
            if (nm < 0 || nm > K) {
                std::fprintf(stderr, "modes_used %d outside 0..%d\n", nm, K);
                std::exit(3);
            }
            modes[i] = (unsigned char)nm;
        }
        wr(out, mask.data(), px);
        if (c.bg[t]) {
            for (size_t i = 0; i < px; ++i) {
                float o[CN];
                background_pixel<CN>(&weight[i * K], &mean[i * K * CN], modes[i], p.TB, o);
                for (int ch = 0; ch < CN; ++ch) {
                    if (c.f32) {
                        unsigned char b[4];
                        std::memcpy(b, &o[ch], 4);
                        bgs.insert(bgs.end(), b, b + 4);
                    } else {
                        bgs.push_back(saturate_u8(o[ch]));
                    }
                }
            }
        }
    }
    wr(out, bgs.data(), bgs.size());
    wr(out, weight.data(), weight.size() * 4);
    wr(out, variance.data(), variance.size() * 4);
    wr(out, mean.data(), mean.size() * 4);
    wr(out, modes.data(), modes.size());
    wr(out, &cnt, sizeof(cnt));
}

template <int CN>
static void run_cn(const Case& c, FILE* out)
{
    switch (c.s.nmixtures) {
    case 1: run_case<CN, 1>(c, out); break;
    case 2: run_case<CN, 2>(c, out); break;
    case 3: run_case<CN, 3>(c, out); break;
    case 4: run_case<CN, 4>(c, out); break;
    case 5: run_case<CN, 5>(c, out); break;
    case 6: run_case<CN, 6>(c, out); break;
    case 7: run_case<CN, 7>(c, out); break;
    case 8: run_case<CN, 8>(c, out); break;
    default: std::fprintf(stderr, "nmixtures %d\n", c.s.nmixtures); std::exit(2);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int ncases = 0;
    rd(in, &ncases, 4);
    for (int k = 0; k < ncases; ++k) {
        Case c;
        int hdr[9];
        double par[8];
        rd(in, hdr, sizeof(hdr));
        rd(in, par, sizeof(par));
        c.w = hdr[0], c.h = hdr[1], c.cn = hdr[2], c.f32 = hdr[3], c.n = hdr[4];
        if (c.w < 1 || c.h < 1 || (c.cn != 1 && c.cn != 3) || c.n < 0) return 2;
        c.s.history = hdr[5];
        c.s.nmixtures = hdr[6];
        c.s.detect_shadows = hdr[7];
        c.s.shadow_value = hdr[8];
        c.s.var_threshold = par[0];
        c.s.var_threshold_gen = (float)par[1];
        c.s.var_init = (float)par[2];
        c.s.var_min = (float)par[3];
        c.s.var_max = (float)par[4];
        c.s.background_ratio = (float)par[5];
        c.s.complexity_reduction = (float)par[6];
        c.s.shadow_threshold = (float)par[7];
        c.rates.resize(c.n);
        c.bg.resize(c.n);
        rd(in, c.rates.data(), sizeof(double) * c.n);
        rd(in, c.bg.data(), c.n);
        c.frames.resize((size_t)c.w * c.h * c.cn * (c.f32 ? 4 : 1) * c.n);
        rd(in, c.frames.data(), c.frames.size());
        if (c.cn == 1)
            run_cn<1>(c, out);
        else
            run_cn<3>(c, out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("cases %d\n", ncases);
    return 0;
}
