// facade_mog2_check.cpp — compiles tbdk::BackgroundSubtractorMOG2 of the C++ facade
// (include/tbdk.hpp) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV); the default configuration is the
//            reference's
//   GPU    : facade_mog2_check gpu <frames.bin> <out.bin> <w> <h> <n> <history>
//            runs the n 8-bit one-channel frames of frames.bin through the class, into
//            pitched masks, and writes the n masks and the final background image to
//            out.bin (the test compares them with the recorded reference); the getters
//            show the reference's defaults, a frame of another size and a changed
//            nmixtures throw
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    tbdk_mog2_config c;
    if (tbdk_mog2_config_default(64, 48, TBDK_DEPTH_8U, 3, &c) != TBDK_OK || c.width != 64 || c.height != 48 ||
        c.channels != 3 || c.history != 500 || c.nmixtures != 5 || c.detect_shadows != 1 || c.shadow_value != 127 ||
        c.var_threshold != 16.0 || c.var_threshold_gen != 9.f || c.var_init != 15.f || c.var_min != 4.f ||
        c.var_max != 75.f || c.background_ratio != 0.9f || c.complexity_reduction != 0.05f ||
        c.shadow_threshold != 0.5f)
        return 20;
    if (tbdk_mog2_config_default(1, 1, 0, 1, nullptr) != TBDK_EINVAL) return 21;
    static_assert(sizeof(tbdk_mog2_config) == 72, "layout of include/tbdk.h");
    if (tbdk_mog2_apply(nullptr, nullptr, 0, nullptr, 0, -1.0, nullptr) != TBDK_EINVAL) return 22;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        if (argc != 8) return 4;
        const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), n = std::atoi(argv[6]), history = std::atoi(argv[7]);
        std::vector<uint8_t> frames((size_t)w * h * n);
        FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) return 5;
        std::fclose(f);
        // history <= 0 and varThreshold <= 0 keep the defaults, as the reference's constructor does
        {
            std::unique_ptr<tbdk::BackgroundSubtractorMOG2> d = tbdk::createBackgroundSubtractorMOG2(ctx, 0, -1.0, false);
            if (d->getHistory() != 500 || d->getVarThreshold() != 16.0 || d->getDetectShadows()) return 6;
        }
        std::unique_ptr<tbdk::BackgroundSubtractorMOG2> m = tbdk::createBackgroundSubtractorMOG2(ctx, history);
        if (m->getHistory() != history || m->getNMixtures() != 5 || !m->getDetectShadows() || m->getShadowValue() != 127 ||
            m->getVarThresholdGen() != 9.0 || m->getVarInit() != 15.0 || m->getVarMin() != 4.0 || m->getVarMax() != 75.0 ||
            m->getShadowThreshold() != 0.5 || m->frames() != 0)
            return 7;
        const int mpitch = w + 13;
        uint8_t *dframes = nullptr, *dmasks = nullptr, *dbg = nullptr;
        if (hipMalloc(&dframes, frames.size()) != hipSuccess || hipMalloc(&dmasks, (size_t)mpitch * h * n) != hipSuccess ||
            hipMalloc(&dbg, (size_t)w * h) != hipSuccess)
            return 8;
        (void)hipMemcpy(dframes, frames.data(), frames.size(), hipMemcpyHostToDevice);
        (void)hipMemset(dmasks, 7, (size_t)mpitch * h * n);
        for (int t = 0; t < n; ++t) {
            const tbdk::GpuMatView img{dframes + (size_t)w * h * t, w, h, w, tbdk::DEPTH_8U, 1};
            const tbdk::GpuImage mask{dmasks + (size_t)mpitch * h * t, w, h, mpitch};
            m->apply(img, mask);
        }
        if (m->frames() != n) return 9;
        m->getBackgroundImage(tbdk::GpuMatView{dbg, w, h, w, tbdk::DEPTH_8U, 1});
        if (hipDeviceSynchronize() != hipSuccess) return 10;
        std::vector<uint8_t> pm((size_t)mpitch * h * n), bg((size_t)w * h);
        (void)hipMemcpy(pm.data(), dmasks, pm.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpy(bg.data(), dbg, bg.size(), hipMemcpyDeviceToHost);
        FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 11;
        for (int r = 0; r < h * n; ++r) {
            std::fwrite(pm.data() + (size_t)r * mpitch, 1, w, o);
            for (int x = w; x < mpitch; ++x)
                if (pm[(size_t)r * mpitch + x] != 7) return 12;  // the mask's padding was written
        }
        std::fwrite(bg.data(), 1, bg.size(), o);
        if (std::fclose(o) != 0) return 13;
        // what may not change
        int thrown = 0;
        try {
            m->setNMixtures(3);
        } catch (const tbdk::Error& e) {
            thrown += e.code() == TBDK_EINVAL;
        }
        try {
            m->apply(tbdk::GpuMatView{dframes, w - 1, h, w, tbdk::DEPTH_8U, 1}, tbdk::GpuImage{dmasks, w - 1, h, mpitch});
        } catch (const tbdk::Error& e) {
            thrown += e.code() == TBDK_EINVAL;
        }
        try {
            m->setHistory(0);
        } catch (const tbdk::Error& e) {
            thrown += e.code() == TBDK_EINVAL;
        }
        if (thrown != 3 || m->frames() != n || m->getHistory() != history) return 14;
        m->setShadowValue(0);
        m->reset();
        if (m->frames() != 0) return 15;
        std::printf("facade BackgroundSubtractorMOG2: ok\n");
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("%s\n", e.what());
        return want_gpu ? 1 : (e.code() == TBDK_ENODEV ? 0 : 2);
    }
}
