// facade_remap_check.cpp — compiles tbdk::remap, tbdk::remapFlow and
// tbdk::warpPerspective of the C++ facade (include/tbdk.hpp) against libtbdk.so.
// Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV); the host-side 3x3 inverse
//            (tbdk_warp_perspective_invert) works without a device
//   GPU    : the facade calls equal the C entries byte for byte; remapFlow equals
//            remap with the map formed on the host; warpPerspective by the
//            identity copies the image; bad arguments return TBDK_EINVAL: an
//            unknown map kind, CV_16SC2 without a fraction plane under LINEAR, a
//            non-finite matrix, CUBIC on 32F, aliasing, sides of 32767 or more
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

namespace {

constexpr int SW = 97, SH = 61, DW = 70, DH = 33, CN = 3;

template <typename T>
T* upload(const std::vector<T>& v)
{
    T* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) return nullptr;
    (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}

std::vector<uint8_t> fetch(const void* d, size_t n)
{
    std::vector<uint8_t> h(n);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(h.data(), d, n, hipMemcpyDeviceToHost);
    return h;
}

int expect_einval(int rc, int code) { return rc == TBDK_EINVAL ? 0 : code; }

}  // namespace

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    // host only: the inverse of a diagonal matrix, and of a singular one (the zero matrix)
    const double Md[9] = {2, 0, 0, 0, 4, 0, 0, 0, 1}, Ms[9] = {1, 2, 3, 2, 4, 6, 0, 0, 1};
    double inv[9];
    if (tbdk_warp_perspective_invert(Md, inv) != TBDK_OK || inv[0] != 0.5 || inv[4] != 0.25 || inv[8] != 1.0) return 20;
    if (tbdk_warp_perspective_invert(Ms, inv) != TBDK_OK) return 21;
    for (double v : inv)
        if (v != 0.0) return 22;
    if (tbdk_warp_perspective_invert(nullptr, inv) != TBDK_EINVAL) return 23;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        std::vector<uint8_t> hs((size_t)SW * SH * CN), hd((size_t)DW * DH * CN, 9);
        for (size_t i = 0; i < hs.size(); ++i) hs[i] = (uint8_t)((i * 2654435761u) >> 24);
        std::vector<float> hmap((size_t)DW * DH * 2), hflow((size_t)DW * DH * 2), hgrid((size_t)DW * DH * 2);
        for (int y = 0; y < DH; ++y)
            for (int x = 0; x < DW; ++x) {
                const size_t i = ((size_t)y * DW + x) * 2;
                hflow[i] = 3.5f * std::sin(0.3f * y) + 0.01f * x;
                hflow[i + 1] = -2.25f * std::cos(0.2f * x);
                hgrid[i] = (float)x + hflow[i];
                hgrid[i + 1] = (float)y + hflow[i + 1];
                hmap[i] = 1.3f * x - 4.f;
                hmap[i + 1] = 1.7f * y + 0.5f * x - 6.f;
            }
        uint8_t *ds = upload(hs), *da = upload(hd), *db = upload(hd);
        float *dmap = upload(hmap), *dflow = upload(hflow), *dgrid = upload(hgrid);
        std::vector<int16_t> hxy((size_t)DW * DH * 2, 3);
        int16_t* dxy = upload(hxy);
        if (!ds || !da || !db || !dmap || !dflow || !dgrid || !dxy) return 4;
        const size_t dbytes = hd.size();
        const tbdk::GpuMatView src{ds, SW, SH, SW * CN, tbdk::DEPTH_8U, CN};
        tbdk::GpuMatView a{da, DW, DH, DW * CN, tbdk::DEPTH_8U, CN}, b{db, DW, DH, DW * CN, tbdk::DEPTH_8U, CN};
        const tbdk::GpuMatView map{dmap, DW, DH, DW * 8, tbdk::DEPTH_32F, 2}, none{};
        const tbdk::GpuMatView flow{dflow, DW, DH, DW * 8, tbdk::DEPTH_32F, 2}, grid{dgrid, DW, DH, DW * 8, tbdk::DEPTH_32F, 2};
        const tbdk::Scalar bv(10, 20, 30);
        // remap: the facade is the C entry
        tbdk::remap(ctx, src, a, map, none, TBDK_INTER_CUBIC, TBDK_BORDER_CONSTANT, bv);
        tbdk::check(tbdk_remap(ctx.get(), ds, TBDK_PIX_U8, CN, SW, SH, SW * CN, db, DW, DH, DW * CN, dmap, DW * 8, nullptr,
                               0, TBDK_MAP_32FC2, TBDK_INTER_CUBIC, TBDK_BORDER_CONSTANT, bv.val, nullptr),
                    "tbdk_remap");
        std::vector<uint8_t> ra = fetch(da, dbytes), rb = fetch(db, dbytes);
        if (ra != rb || ra == hd) return 6;
        // remapFlow equals remap with grid + flow
        tbdk::remapFlow(ctx, src, a, flow, 1, TBDK_INTER_LINEAR, TBDK_BORDER_REFLECT_101);
        tbdk::remap(ctx, src, b, grid, none, TBDK_INTER_LINEAR, TBDK_BORDER_REFLECT_101);
        ra = fetch(da, dbytes), rb = fetch(db, dbytes);
        if (ra != rb) return 7;
        // warpPerspective by the identity, NEAREST: the top-left DW x DH of the source
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        tbdk::warpPerspective(ctx, src, a, I, TBDK_INTER_NEAREST);
        ra = fetch(da, dbytes);
        for (int y = 0; y < DH; ++y)
            if (std::memcmp(&ra[(size_t)y * DW * CN], &hs[(size_t)y * SW * CN], (size_t)DW * CN) != 0) return 8;
        // what the calls do not take
        const double nanM[9] = {1, 0, 0, 0, 1, 0, 0, std::numeric_limits<double>::quiet_NaN(), 1};
        const double z4[4] = {0, 0, 0, 0};
        int rc = 0;
        rc = rc ? rc : expect_einval(tbdk_remap(ctx.get(), ds, TBDK_PIX_U8, CN, SW, SH, SW * CN, da, DW, DH, DW * CN, dmap,
                                                DW * 8, nullptr, 0, 7, TBDK_INTER_LINEAR, 0, z4, nullptr), 10);
        rc = rc ? rc : expect_einval(tbdk_remap(ctx.get(), ds, TBDK_PIX_U8, CN, SW, SH, SW * CN, da, DW, DH, DW * CN, dxy,
                                                DW * 4, nullptr, 0, TBDK_MAP_16SC2, TBDK_INTER_LINEAR, 0, z4, nullptr), 11);
        rc = rc ? rc : expect_einval(tbdk_warp_perspective(ctx.get(), ds, TBDK_PIX_U8, CN, SW, SH, SW * CN, da, DW, DH,
                                                           DW * CN, nanM, TBDK_INTER_LINEAR, 0, z4, nullptr), 12);
        rc = rc ? rc : expect_einval(tbdk_remap(ctx.get(), dmap, TBDK_PIX_F32, 1, DW, DH, DW * 8, dgrid, DW, DH, DW * 8, dflow,
                                                DW * 8, nullptr, 0, TBDK_MAP_32FC2, TBDK_INTER_CUBIC, 0, z4, nullptr), 13);
        rc = rc ? rc : expect_einval(tbdk_remap_flow(ctx.get(), ds, TBDK_PIX_U8, CN, SW, SH, SW * CN, ds + 5, DW, DH, DW * CN,
                                                     dflow, DW * 8, 1, TBDK_INTER_LINEAR, 0, z4, nullptr), 14);
        rc = rc ? rc : expect_einval(tbdk_remap(ctx.get(), ds, TBDK_PIX_U8, 1, 32767, 1, 32767, da, DW, DH, DW * CN, dmap,
                                                DW * 8, nullptr, 0, TBDK_MAP_32FC2, TBDK_INTER_LINEAR, 0, z4, nullptr), 15);
        rc = rc ? rc : expect_einval(tbdk_warp_perspective(ctx.get(), ds, TBDK_PIX_U8, 1, SW, SH, SW * CN, da, 1, 32767, 1, I,
                                                           TBDK_INTER_LINEAR, 0, z4, nullptr), 16);
        if (rc) return rc;
        // the 16SC2 map alone is a NEAREST map: every pixel is source pixel (3, 3)
        tbdk::remap(ctx, src, a, tbdk::GpuMatView{dxy, DW, DH, DW * 4, tbdk::DEPTH_16S, 2}, none, TBDK_INTER_NEAREST);
        ra = fetch(da, dbytes);
        if (std::memcmp(&ra[0], &hs[((size_t)3 * SW + 3) * CN], CN) != 0 || std::memcmp(&ra[dbytes - CN], &ra[0], CN) != 0)
            return 17;
        try {  // mismatched depths throw before the C entry
            tbdk::GpuMatView f32 = a;
            f32.depth = tbdk::DEPTH_32F;
            tbdk::remapFlow(ctx, src, f32, flow);
            return 18;
        } catch (const tbdk::Error& e) {
            if (e.code() != TBDK_EINVAL) return 19;
        }
        std::printf("facade remap ok\n");
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 5;
    }
}
