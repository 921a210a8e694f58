// affine2d_core_check.cpp — the sequential estimateAffine2D / estimateAffinePartial2D
// built from opencv_amd/csrc/affine2d_core.hpp alone, for the host (no HIP, no
// library), meant to be compiled with -fsanitize=address,undefined
// -ffp-contract=off.
//
//   affine2d_core_check <cases.bin>
//
// cases.bin (written by tests/test_affine2d_core_host.py), little-endian:
//   int32 ncases, then per case
//   int32 n, model, method, max_iters, refine_iters; double threshold, confidence; float src[2n], dst[2n]
// A set of more than 4096 pairs is answered as the library answers it (npoints -1).
// Prints per case:
//   case <i> valid <v> npoints <n or -1> ninliers <k> iters <t> nsub <s> margin <min distance of num/denom from k + 0.5>
//   M0 <6 doubles as hex words>     the result with refine_iters = 0
//   M <6 doubles as hex words>      the refined result
//   mask <n characters 0/1>
//   subsets <modelPoints * nsub indices>
//   hyps <FNV-1a 64 over the bits of every hypothesis' M, a NaN as 0x7ff8000000000000>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../opencv_amd/csrc/affine2d_core.hpp"

namespace ac = tbdk::affine2d_core;
namespace hc = tbdk::homography_core;

struct Pairs {
    const hc::Pt *src, *dst;
    hc::Pt M(int i) const { return src[i]; }
    hc::Pt m(int i) const { return dst[i]; }
};

template <int N>
struct SeqStep {
    Pairs p;
    int n;
    hc::Ws ws;
    double sums(const double* h, bool jac, ac::LmSums<N>* cur) const
    {
        ac::LmSums<N> s;
        ac::lm_zero(&s);
        for (int i = 0; i < n; ++i) ac::lm_point<N>(h, p.M(i), p.m(i), jac, &s);
        if (jac) *cur = s;
        return s.S;
    }
    void solve(const ac::LmSums<N>* cur, const double* D, double lambda, double* d) const
    {
        ac::lm_solve<N>(ws, cur, D, lambda, d);
    }
    double inv_diag_max(const ac::LmSums<N>* cur, const double* D) const { return ac::lm_inv_diag_max<N>(ws, cur, D); }
};

static uint64_t fnv(uint64_t h, const void* p, size_t n)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static uint64_t fnv_model(uint64_t h, const double* M)
{
    for (int i = 0; i < 6; ++i) {
        uint64_t w;
        std::memcpy(&w, &M[i], 8);
        if (std::isnan(M[i])) w = 0x7ff8000000000000ull;
        h = fnv(h, &w, 8);
    }
    return h;
}

static void print_m(const char* name, const double* M)
{
    std::printf("%s", name);
    for (int i = 0; i < 6; ++i) {
        uint64_t w;
        std::memcpy(&w, &M[i], 8);
        std::printf(" %016" PRIx64, w);
    }
    std::printf("\n");
}

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

template <int MP>
static void run_case(int ci, int n_all, int method, int max_iters, int refine_iters, double thr, double conf,
                     const std::vector<hc::Pt>& src, const std::vector<hc::Pt>& dst)
{
    constexpr int N = MP == 3 ? 6 : 4;
    const bool over = n_all > 4096;
    const int n = over ? 0 : n_all;
    std::vector<double> wsbuf(hc::kWsDoubles);
    const hc::Ws ws{wsbuf.data(), 1};
    const Pairs all{src.data(), dst.data()};
    std::vector<unsigned char> mask(n_all, 0);
    std::vector<int> subsets;
    double M[6] = {1, 0, 0, 0, 1, 0}, M0[6], margin = 1;
    uint64_t hyps = 14695981039346656037ull;
    int iters = 0, ninl = 0;
    bool have = false;
    const bool lmeds = method == ac::kLmeds;
    if (n == MP) {
        const int idx[3] = {0, 1, 2};
        ac::run_kernel<MP>(all, idx, M);
        have = true;
        for (int i = 0; i < n; ++i) mask[i] = 1;
        ninl = n;
    } else if (n > MP) {
        tbdk::RansacRng rng;
        float t = ac::inlier_bound(thr);
        double mg;
        int niters = lmeds ? ac::lmeds_num_iters(conf, MP, max_iters, &mg) : (max_iters > 1 ? max_iters : 1);
        if (lmeds && mg < margin) margin = mg;
        int max_good = 0;
        double min_median = DBL_MAX;
        std::vector<float> err(n);
        for (; iters < niters; ++iters) {
            int idx[3] = {0, 0, 0};
            if (!ac::get_subset<MP>(all, n, rng, lmeds ? ac::kMaxAttemptsLmeds : ac::kMaxAttemptsRansac, idx)) break;
            subsets.insert(subsets.end(), idx, idx + MP);
            double model[6];
            ac::run_kernel<MP>(all, idx, model);
            hyps = fnv_model(hyps, model);
            const ac::ModelF mf = ac::model_f(model);
            if (!lmeds) {
                int good = 0;
                for (int i = 0; i < n; ++i) good += ac::is_inlier(mf, t, src[i], dst[i]);
                if (good > (max_good > MP - 1 ? max_good : MP - 1)) {
                    std::memcpy(M, model, sizeof M);
                    max_good = good;
                    niters = ac::update_num_iters(conf, (double)(n - good) / n, MP, niters, &mg);
                    if (mg < margin) margin = mg;
                }
            } else {
                for (int i = 0; i < n; ++i) err[i] = ac::reproj_error(mf, src[i], dst[i]);
                const unsigned bits = ac::rank_select(
                    [&](unsigned msk, unsigned want) {
                        int c = 0;
                        for (int i = 0; i < n; ++i) {
                            unsigned b;
                            std::memcpy(&b, &err[i], 4);
                            c += (b & msk) == want;
                        }
                        return c;
                    },
                    n / 2);
                float medf;
                std::memcpy(&medf, &bits, 4);
                const double median = medf;
                if (median < min_median) {
                    min_median = median;
                    std::memcpy(M, model, sizeof M);
                }
            }
        }
        if (!lmeds) {
            have = max_good > 0;
        } else if (min_median < DBL_MAX) {
            t = ac::inlier_bound(ac::lmeds_sigma(min_median, n, MP));
            have = true;
        }
        if (have) {
            const ac::ModelF mf = ac::model_f(M);
            for (int i = 0; i < n; ++i) ninl += mask[i] = ac::is_inlier(mf, t, src[i], dst[i]);
            have = ninl >= MP;
        }
        if (!have) {
            ninl = 0;
            mask.assign(n_all, 0);
            const double id[6] = {1, 0, 0, 0, 1, 0};
            std::memcpy(M, id, sizeof M);
        }
    }
    std::memcpy(M0, M, sizeof M);
    if (have && n > MP && refine_iters > 0) {
        std::vector<hc::Pt> s, d;
        for (int i = 0; i < n; ++i)
            if (mask[i]) s.push_back(src[i]), d.push_back(dst[i]);
        const SeqStep<N> step{Pairs{s.data(), d.data()}, (int)s.size(), ws};
        ac::LmSums<N> cur;
        if (MP == 3) {
            ac::lm_refine<N>(step, &cur, refine_iters, M);
        } else {
            double h[4];
            ac::partial_pack(M, h);
            ac::lm_refine<N>(step, &cur, refine_iters, h);
            ac::partial_unpack(h, M);
        }
    }
    std::printf("case %d valid %d npoints %d ninliers %d iters %d nsub %d margin %.9g\n", ci, (int)have,
                over ? -1 : n_all, ninl, iters, (int)subsets.size() / MP, margin);
    print_m("M0", M0);
    print_m("M", M);
    std::printf("mask ");
    for (int i = 0; i < n_all; ++i) std::putchar('0' + mask[i]);
    std::printf("\nsubsets");
    for (int v : subsets) std::printf(" %d", v);
    std::printf("\nhyps %016" PRIx64 "\n", hyps);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t ncases = 0;
    if (!f || !rd(f, &ncases, 4)) return 2;
    for (int ci = 0; ci < ncases; ++ci) {
        int32_t hdr[5];
        double par[2];
        if (!rd(f, hdr, sizeof hdr) || !rd(f, par, sizeof par)) return 2;
        const int n = hdr[0];
        std::vector<hc::Pt> src(n), dst(n);
        if (!rd(f, src.data(), sizeof(hc::Pt) * n) || !rd(f, dst.data(), sizeof(hc::Pt) * n)) return 2;
        if (hdr[1] == ac::kPartial)
            run_case<2>(ci, n, hdr[2], hdr[3], hdr[4], par[0], par[1], src, dst);
        else
            run_case<3>(ci, n, hdr[2], hdr[3], hdr[4], par[0], par[1], src, dst);
    }
    std::fclose(f);
    return 0;
}
