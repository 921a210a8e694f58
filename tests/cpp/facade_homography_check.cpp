// facade_homography_check.cpp — compiles tbdk::findHomography and
// tbdk::warpPerspectiveDeviceMatrix of the C++ facade (include/tbdk.hpp) against
// libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV); the default parameters are
//            the reference's
//   GPU    : on pairs under an exact homography the facade call equals the C
//            entry bit for bit and recovers the matrix; the warp by the device
//            matrix equals the warp by the downloaded one byte for byte, queued
//            behind findHomography with no synchronisation; bad parameters
//            return TBDK_EINVAL
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

namespace {

template <typename T>
T* upload(const std::vector<T>& v)
{
    T* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) return nullptr;
    (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}

template <typename T>
std::vector<T> fetch(const T* d, size_t n)
{
    std::vector<T> h(n);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost);
    return h;
}

}  // namespace

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    tbdk_homography_params p;
    if (tbdk_homography_default_params(&p) != TBDK_OK || p.method != TBDK_HOMOGRAPHY_RANSAC || p.reproj_threshold != 3.0 ||
        p.max_iters != 2000 || p.confidence != 0.995 || p.refine != 1)
        return 20;
    if (tbdk_homography_default_params(nullptr) != TBDK_EINVAL) return 21;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        constexpr int N = 40, SW = 97, SH = 61, DW = 70, DH = 33;
        const double T[9] = {1.01, 0.02, 3.0, -0.015, 0.99, -2.0, 2e-5, -1e-5, 1.0};
        std::vector<float> hs(2 * N), hd(2 * N);
        for (int i = 0; i < N; ++i) {
            const double x = 5.0 + 13.0 * (i % 8) + 0.37 * i, y = 4.0 + 11.0 * (i / 8) + 0.11 * i;
            const double w = T[6] * x + T[7] * y + T[8];
            hs[2 * i] = (float)x, hs[2 * i + 1] = (float)y;
            hd[2 * i] = (float)((T[0] * x + T[1] * y + T[2]) / w), hd[2 * i + 1] = (float)((T[3] * x + T[4] * y + T[5]) / w);
        }
        hd[6] += 25.f;  // one outlier
        const std::vector<int32_t> hoff = {0, N};
        float *ds = upload(hs), *dd = upload(hd);
        int32_t* doff = upload(hoff);
        std::vector<tbdk_homography> hz(2);
        std::memset(hz.data(), 0, sizeof(tbdk_homography) * 2);
        tbdk_homography* dout = upload(hz);
        std::vector<uint8_t> hm(2 * N, 7);
        uint8_t* dmask = upload(hm);
        std::vector<uint8_t> himg((size_t)SW * SH), hfill((size_t)DW * DH, 9);
        for (size_t i = 0; i < himg.size(); ++i) himg[i] = (uint8_t)((i * 2654435761u) >> 24);
        uint8_t *dimg = upload(himg), *da = upload(hfill), *db = upload(hfill);
        if (!ds || !dd || !doff || !dout || !dmask || !dimg || !da || !db) return 4;
        // the facade, then the warp by its device matrix, nothing in between
        tbdk::findHomography(ctx, ds, dd, nullptr, doff, 1, dout, tbdk::RANSAC, 3.0, dmask);
        const tbdk::GpuMatView src{dimg, SW, SH, SW, tbdk::DEPTH_8U, 1};
        tbdk::GpuMatView a{da, DW, DH, DW, tbdk::DEPTH_8U, 1}, b{db, DW, DH, DW, tbdk::DEPTH_8U, 1};
        tbdk::warpPerspectiveDeviceMatrix(ctx, src, a, dout[0].h, &dout[0].valid);
        // the C entry into the second slot
        if (tbdk_find_homography(ctx.get(), ds, dd, nullptr, doff, 1, &p, dout + 1, dmask + N, nullptr) != TBDK_OK) return 5;
        const std::vector<tbdk_homography> out = fetch(dout, 2);
        if (std::memcmp(&out[0], &out[1], sizeof out[0]) != 0) return 6;
        if (!out[0].valid || out[0].npoints != N || out[0].ninliers != N - 1 || out[0].h[8] != 1.0) return 7;
        for (int i = 0; i < 9; ++i)
            if (std::fabs(out[0].h[i] - T[i]) > 1e-3 * (i % 3 == 2 && i < 8 ? 100 : 1)) return 8;
        const std::vector<uint8_t> mask = fetch(dmask, 2 * N);
        for (int i = 0; i < N; ++i)
            if (mask[i] != (i == 3 ? 0 : 1) || mask[i] != mask[N + i]) return 9;
        tbdk::warpPerspective(ctx, src, b, out[0].h);
        if (fetch(da, hfill.size()) != fetch(db, hfill.size())) return 10;
        if (fetch(da, hfill.size()) == hfill) return 11;
        // bad parameters
        tbdk_homography_params q = p;
        q.method = 4;
        if (tbdk_find_homography(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 12;
        q = p, q.max_iters = 0;
        if (tbdk_find_homography(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 13;
        q = p, q.confidence = 1.0;
        if (tbdk_find_homography(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 14;
        if (tbdk_find_homography(ctx.get(), nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr, nullptr, nullptr) != TBDK_OK)
            return 15;
        if (tbdk_warp_perspective_dev(ctx.get(), dimg, TBDK_PIX_U8, 1, SW, SH, SW, da, DW, DH, DW, nullptr, nullptr,
                                      TBDK_INTER_LINEAR, TBDK_BORDER_CONSTANT, tbdk::Scalar().val, nullptr) != TBDK_EINVAL)
            return 16;
        std::printf("facade findHomography: ok\n");
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("%s\n", e.what());
        return want_gpu ? 1 : (e.code() == TBDK_ENODEV ? 0 : 2);
    }
}
