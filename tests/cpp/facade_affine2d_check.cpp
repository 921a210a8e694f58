// facade_affine2d_check.cpp — compiles tbdk::estimateAffine2D,
// tbdk::estimateAffinePartial2D and tbdk::warpAffineDeviceMatrix of the C++
// facade (include/tbdk.hpp) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV); the default parameters are
//            the reference's
//   GPU    : on pairs under an exact similarity the facade calls equal the C
//            entry bit for bit and recover the matrix; the warp by the device
//            matrix equals the warp by the downloaded one byte for byte, queued
//            behind estimateAffine2D with no synchronisation; bad parameters
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
    tbdk_affine2d_params p;
    if (tbdk_affine2d_default_params(&p) != TBDK_OK || p.model != TBDK_AFFINE2D_FULL ||
        p.method != TBDK_AFFINE2D_RANSAC || p.reproj_threshold != 3.0 || p.max_iters != 2000 || p.confidence != 0.99 ||
        p.refine_iters != 10)
        return 20;
    if (tbdk_affine2d_default_params(nullptr) != TBDK_EINVAL) return 21;
    static_assert(sizeof(tbdk_affine2d) == 64 && sizeof(tbdk_affine2d_params) == 40, "layout of include/tbdk.h");
    static_assert(tbdk::LMEDS == 4 && tbdk::RANSAC == 8 && TBDK_AFFINE2D_MAX_PAIRS == 4096, "the reference's values");
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        constexpr int N = 40, SW = 97, SH = 61, DW = 70, DH = 33;
        const double T[6] = {1.02, -0.03, 3.0, 0.03, 1.02, -2.0};  // a similarity: both models recover it
        std::vector<float> hs(2 * N), hd(2 * N);
        for (int i = 0; i < N; ++i) {
            const double x = 5.0 + 13.0 * (i % 8) + 0.37 * i, y = 4.0 + 11.0 * (i / 8) + 0.11 * i;
            hs[2 * i] = (float)x, hs[2 * i + 1] = (float)y;
            hd[2 * i] = (float)(T[0] * x + T[1] * y + T[2]), hd[2 * i + 1] = (float)(T[3] * x + T[4] * y + T[5]);
        }
        hd[6] += 25.f;  // one outlier
        const std::vector<int32_t> hoff = {0, N};
        float *ds = upload(hs), *dd = upload(hd);
        int32_t* doff = upload(hoff);
        std::vector<tbdk_affine2d> hz(3);
        std::memset(hz.data(), 0, sizeof(tbdk_affine2d) * 3);
        tbdk_affine2d* dout = upload(hz);
        std::vector<uint8_t> hm(3 * N, 7);
        uint8_t* dmask = upload(hm);
        std::vector<uint8_t> himg((size_t)SW * SH), hfill((size_t)DW * DH, 9);
        for (size_t i = 0; i < himg.size(); ++i) himg[i] = (uint8_t)((i * 2654435761u) >> 24);
        uint8_t *dimg = upload(himg), *da = upload(hfill), *db = upload(hfill);
        if (!ds || !dd || !doff || !dout || !dmask || !dimg || !da || !db) return 4;
        // the facade, then the warp by its device matrix, nothing in between
        tbdk::estimateAffine2D(ctx, ds, dd, nullptr, doff, 1, dout, dmask);
        const tbdk::GpuImage src{dimg, SW, SH, SW};
        tbdk::GpuImage a{da, DW, DH, DW}, b{db, DW, DH, DW};
        tbdk::warpAffineDeviceMatrix(ctx, src, a, dout[0].m, &dout[0].valid);
        // the C entry into the second slot, the partial model into the third
        if (tbdk_estimate_affine_2d(ctx.get(), ds, dd, nullptr, doff, 1, &p, dout + 1, dmask + N, nullptr) != TBDK_OK) return 5;
        tbdk::estimateAffinePartial2D(ctx, ds, dd, nullptr, doff, 1, dout + 2, dmask + 2 * N, tbdk::LMEDS);
        const std::vector<tbdk_affine2d> out = fetch(dout, 3);
        if (std::memcmp(&out[0], &out[1], sizeof out[0]) != 0) return 6;
        for (int k = 0; k < 3; k += 2) {
            if (!out[k].valid || out[k].npoints != N || out[k].ninliers != N - 1) return 7;
            for (int i = 0; i < 6; ++i)
                if (std::fabs(out[k].m[i] - T[i]) > 1e-3 * (i % 3 == 2 ? 100 : 1)) return 8;
        }
        if (out[2].m[0] != out[2].m[4] || out[2].m[1] != -out[2].m[3]) return 17;
        const std::vector<uint8_t> mask = fetch(dmask, 3 * N);
        for (int i = 0; i < N; ++i)
            if (mask[i] != (i == 3 ? 0 : 1) || mask[i] != mask[N + i] || mask[i] != mask[2 * N + i]) return 9;
        tbdk::cuda::warpAffine(ctx, src, b, out[0].m);
        if (fetch(da, hfill.size()) != fetch(db, hfill.size())) return 10;
        if (fetch(da, hfill.size()) == hfill) return 11;
        // bad parameters
        tbdk_affine2d_params q = p;
        q.method = 0;
        if (tbdk_estimate_affine_2d(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 12;
        q = p, q.max_iters = 0;
        if (tbdk_estimate_affine_2d(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 13;
        q = p, q.confidence = 1.0;
        if (tbdk_estimate_affine_2d(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 14;
        q = p, q.model = 2;
        if (tbdk_estimate_affine_2d(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 18;
        q = p, q.refine_iters = 101;
        if (tbdk_estimate_affine_2d(ctx.get(), ds, dd, nullptr, doff, 1, &q, dout, nullptr, nullptr) != TBDK_EINVAL) return 19;
        if (tbdk_estimate_affine_2d(ctx.get(), nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr, nullptr, nullptr) != TBDK_OK)
            return 15;
        if (tbdk_warp_affine_u8_dev(ctx.get(), dimg, SW, SH, SW, da, DW, DH, DW, nullptr, nullptr, TBDK_INTER_LINEAR,
                                    TBDK_BORDER_CONSTANT, 0, nullptr) != TBDK_EINVAL)
            return 16;
        std::printf("facade estimateAffine2D: ok\n");
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("%s\n", e.what());
        return want_gpu ? 1 : (e.code() == TBDK_ENODEV ? 0 : 2);
    }
}
