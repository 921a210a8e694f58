// facade_fb_check.cpp — SparsePyrLKOpticalFlow::calcChecked of the C++ facade
// (include/tbdk.hpp) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV)
//   GPU    : calcChecked equals calc forward, calc backward from the tracked
//            points, and the comparison done here on the host
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const int W = 320, H = 240;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        // a blocky texture, moved by (3, 2) in the second frame; a flat patch covers
        // part of the second frame, so some points are lost or come back elsewhere
        std::vector<uint8_t> f0((size_t)W * H), f1((size_t)W * H);
        auto tex = [](int x, int y) {
            unsigned v = (unsigned)(x / 5) * 2654435761u ^ (unsigned)(y / 4) * 40503u;
            v ^= v >> 13;
            return (uint8_t)(64 + (v * 2246822519u >> 25) + ((x * 3 + y * 5) & 31));
        };
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                f0[(size_t)y * W + x] = tex(x, y);
                const bool patch = x >= 120 && x < 200 && y >= 80 && y < 150;
                f1[(size_t)y * W + x] = patch ? (uint8_t)128 : tex(x - 3, y - 2);
            }
        std::vector<float> pts;
        for (int y = 6; y < H; y += 13)
            for (int x = 5; x < W; x += 11) {
                pts.push_back((float)x + 0.25f);
                pts.push_back((float)y + 0.5f);
            }
        const int n = (int)pts.size() / 2;
        uint8_t *d0, *d1, *st, *stf, *stb;
        float *p0, *p1, *p1c, *pb, *err, *errc, *fbe;
        if (hipMalloc(&d0, f0.size()) || hipMalloc(&d1, f1.size()) || hipMalloc(&st, n) || hipMalloc(&stf, n) ||
            hipMalloc(&stb, n) || hipMalloc(&p0, 8 * n) || hipMalloc(&p1, 8 * n) || hipMalloc(&p1c, 8 * n) ||
            hipMalloc(&pb, 8 * n) || hipMalloc(&err, 4 * n) || hipMalloc(&errc, 4 * n) || hipMalloc(&fbe, 4 * n))
            return 4;
        (void)hipMemcpy(d0, f0.data(), f0.size(), hipMemcpyHostToDevice);
        (void)hipMemcpy(d1, f1.data(), f1.size(), hipMemcpyHostToDevice);
        (void)hipMemcpy(p0, pts.data(), 8 * n, hipMemcpyHostToDevice);
        const tbdk::GpuImage a{d0, W, H, W}, b{d1, W, H, W};
        const float thr = 0.5f;
        auto lk = tbdk::cuda::SparsePyrLKOpticalFlow::create(ctx, {21, 21}, 2, 30);
        lk->calcChecked(a, b, p0, p1c, st, n, thr, errc, fbe);
        lk->calc(a, b, p0, p1, stf, err, n);
        lk->calc(b, a, p1, pb, stb, nullptr, n);
        (void)hipDeviceSynchronize();
        std::vector<uint8_t> hst(n), hstf(n), hstb(n);
        std::vector<float> hp1(2 * n), hp1c(2 * n), hpb(2 * n), herr(n), herrc(n), hfbe(n);
        (void)hipMemcpy(hst.data(), st, n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hstf.data(), stf, n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hstb.data(), stb, n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hp1.data(), p1, 8 * n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hp1c.data(), p1c, 8 * n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hpb.data(), pb, 8 * n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(herr.data(), err, 4 * n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(herrc.data(), errc, 4 * n, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hfbe.data(), fbe, 4 * n, hipMemcpyDeviceToHost);
        if (std::memcmp(hp1.data(), hp1c.data(), 8 * n) || std::memcmp(herr.data(), herrc.data(), 4 * n)) return 5;
        int kept = 0, lostf = 0, lostb = 0, far = 0;
        for (int i = 0; i < n; ++i) {
            float d = std::numeric_limits<float>::infinity();
            if (hstf[i] && hstb[i])
                d = std::fmax(std::fabs(pts[2 * i] - hpb[2 * i]), std::fabs(pts[2 * i + 1] - hpb[2 * i + 1]));
            const uint8_t want = hstf[i] && hstb[i] && d < thr;
            if (hst[i] != want) return 6;
            if (std::memcmp(&hfbe[i], &d, 4)) return 7;
            kept += want;
            lostf += !hstf[i];
            lostb += hstf[i] && !hstb[i];
            far += hstf[i] && hstb[i] && !(d < thr);
        }
        std::printf("%d points: %d kept, %d lost forward, %d lost backward, %d too far\n", n, kept, lostf, lostb, far);
        if (kept == 0 || kept == n) return 8;  // the check must have had something to do
        bool threw = false;
        try {
            lk->calcChecked(a, b, p0, p1c, st, n, 0.f);
        } catch (const tbdk::Error& e) {
            threw = e.code() == TBDK_EINVAL;
        }
        return threw ? 0 : 9;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 7;
    }
}
