// homography_core_check.cpp — the sequential findHomography built from
// opencv_amd/csrc/homography_core.hpp alone, for the host (no HIP, no library),
// meant to be compiled with -fsanitize=address,undefined -ffp-contract=off.
//
//   homography_core_check <cases.bin>
//
// cases.bin (written by tests/test_homography_core_host.py), little-endian:
//   int32 ncases, then per case
//   int32 n, method, max_iters; double threshold, confidence; float src[2n], dst[2n]
// Prints per case:
//   case <i> valid <v> ninliers <k> iters <t> nsub <s> margin <min distance of num/denom from k + 0.5>
//   H0 <9 doubles as hex words>     the result with refine = 0
//   H <9 doubles as hex words>      the refined result
//   mask <n characters 0/1>
//   subsets <4 * nsub indices>
//   hyps <FNV-1a 64 over the bits of every hypothesis' H, a zero word for a failed one>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../opencv_amd/csrc/homography_core.hpp"

namespace hc = tbdk::homography_core;

struct Pairs {
    const hc::Pt *src, *dst;
    hc::Pt M(int i) const { return src[i]; }
    hc::Pt m(int i) const { return dst[i]; }
};

struct Indexed {
    const hc::Pt *src, *dst;
    int idx[4];
    hc::Pt M(int i) const { return src[idx[i]]; }
    hc::Pt m(int i) const { return dst[idx[i]]; }
};

struct SeqSums {
    Pairs p;
    int n;
    double operator()(const double* h, bool jac, hc::LmSums* cur) const
    {
        hc::LmSums s;
        hc::lm_zero(&s);
        for (int i = 0; i < n; ++i) hc::lm_point(h, p.M(i), p.m(i), jac, &s);
        if (jac) *cur = s;
        return s.S;
    }
};

static uint64_t fnv(uint64_t h, const void* p, size_t n)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static void print_h(const char* name, const double* H)
{
    std::printf("%s", name);
    for (int i = 0; i < 9; ++i) {
        uint64_t w;
        std::memcpy(&w, &H[i], 8);
        std::printf(" %016" PRIx64, w);
    }
    std::printf("\n");
}

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t ncases = 0;
    if (!f || !rd(f, &ncases, 4)) return 2;
    for (int ci = 0; ci < ncases; ++ci) {
        int32_t hdr[3];
        double par[2];
        if (!rd(f, hdr, sizeof hdr) || !rd(f, par, sizeof par)) return 2;
        const int n = hdr[0], method = hdr[1], max_iters = hdr[2];
        const double thr = par[0] <= 0 ? 3. : par[0], conf = par[1];
        std::vector<hc::Pt> src(n), dst(n);
        if (!rd(f, src.data(), sizeof(hc::Pt) * n) || !rd(f, dst.data(), sizeof(hc::Pt) * n)) return 2;
        std::vector<double> wsbuf(hc::kWsDoubles);
        const hc::Ws ws{wsbuf.data(), 1};
        const Pairs all{src.data(), dst.data()};
        std::vector<unsigned char> mask(n, 0);
        std::vector<int> subsets;
        double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, H0[9], margin = 1;
        uint64_t hyps = 14695981039346656037ull;
        int valid = 0, iters = 0, ninl = 0;
        bool have = false;
        if (n >= 4 && (method == 0 || n == 4)) {
            have = hc::run_kernel(all, n, ws, H);
            if (have) mask.assign(n, 1);
        } else if (n > 4) {
            tbdk::RansacRng rng;
            int niters = max_iters > 1 ? max_iters : 1, max_good = 0;
            const float t = hc::inlier_bound(thr);
            std::vector<unsigned char> cur(n);
            for (; iters < niters; ++iters) {
                Indexed sub{src.data(), dst.data(), {0, 0, 0, 0}};
                if (!hc::get_subset(all, n, rng, &sub.idx[0], &sub.idx[1], &sub.idx[2], &sub.idx[3])) break;
                subsets.insert(subsets.end(), sub.idx, sub.idx + 4);
                double model[9];
                if (!hc::run_kernel(sub, 4, ws, model)) {
                    const uint64_t z = 0;
                    hyps = fnv(hyps, &z, 8);
                    continue;
                }
                hyps = fnv(hyps, model, sizeof model);
                const hc::ModelF mf = hc::model_f(model);
                int good = 0;
                for (int i = 0; i < n; ++i) good += cur[i] = hc::is_inlier(mf, t, src[i], dst[i]);
                if (good > (max_good > 3 ? max_good : 3)) {
                    mask = cur;
                    std::memcpy(H, model, sizeof H);
                    max_good = good;
                    double mg;
                    niters = hc::update_num_iters(conf, (double)(n - good) / n, niters, &mg);
                    if (mg < margin) margin = mg;
                }
            }
            have = max_good > 0;
            if (!have) mask.assign(n, 0);
        }
        std::memcpy(H0, H, sizeof H);
        if (have) {
            valid = 1;
            std::vector<hc::Pt> s, d;
            for (int i = 0; i < n; ++i)
                if (mask[i]) s.push_back(src[i]), d.push_back(dst[i]);
            ninl = (int)s.size();
            if (n > 4 && ninl > 0) {
                const Pairs inl{s.data(), d.data()};
                if (method != 0) hc::run_kernel(inl, ninl, ws, H);
                std::memcpy(H0, H, sizeof H);
                hc::LmSums cur;
                hc::lm_refine(SeqSums{inl, ninl}, ws, &cur, H);
            }
        }
        std::printf("case %d valid %d ninliers %d iters %d nsub %d margin %.9g\n", ci, valid, ninl, iters,
                    (int)subsets.size() / 4, margin);
        print_h("H0", H0);
        print_h("H", H);
        std::printf("mask ");
        for (int i = 0; i < n; ++i) std::putchar('0' + mask[i]);
        std::printf("\nsubsets");
        for (int v : subsets) std::printf(" %d", v);
        std::printf("\nhyps %016" PRIx64 "\n", hyps);
    }
    std::fclose(f);
    return 0;
}
