// facade_knn_check.cpp — compiles tbdk::BackgroundSubtractorKNN of the C++ facade
// (include/tbdk.hpp) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV); the default configuration is the
//            reference's
//   GPU    : facade_knn_check gpu <frames.bin> <out.bin> <w> <h> <n> <history>
//            runs the n 8-bit one-channel frames of frames.bin through the class, into
//            pitched masks, and writes the n masks, the final background image and the RNG
//            state (8 bytes) to out.bin (the test compares them with the recorded
//            reference); the getters show the reference's defaults, the setters hold, a
//            frame of another size, a changed nSamples and the rates without a defined
//            result throw and leave the state as it was
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    tbdk_knn_config c;
    if (tbdk_knn_config_default(64, 48, 3, &c) != TBDK_OK || c.width != 64 || c.height != 48 || c.channels != 3 ||
        c.history != 500 || c.nsamples != 7 || c.knn_samples != 2 || c.detect_shadows != 1 || c.shadow_value != 127 ||
        c.dist2_threshold != 400.f || c.shadow_threshold != 0.5f || c.rng_state != 0xffffffffull)
        return 20;
    if (tbdk_knn_config_default(1, 1, 1, nullptr) != TBDK_EINVAL) return 21;
    static_assert(sizeof(tbdk_knn_config) == 48, "layout of include/tbdk.h");
    if (tbdk_knn_apply(nullptr, nullptr, 0, nullptr, 0, -1.0, nullptr) != TBDK_EINVAL) return 22;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        if (argc != 8) return 4;
        const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), n = std::atoi(argv[6]), history = std::atoi(argv[7]);
        std::vector<uint8_t> frames((size_t)w * h * n);
        FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) return 5;
        std::fclose(f);
        // history <= 0 and dist2Threshold <= 0 keep the defaults, as the reference's constructor does
        {
            std::unique_ptr<tbdk::BackgroundSubtractorKNN> d = tbdk::createBackgroundSubtractorKNN(ctx, 0, -1.0, false);
            if (d->getHistory() != 500 || d->getDist2Threshold() != 400.0 || d->getDetectShadows()) return 6;
            // before the first apply every setter holds, nSamples included, and kNNSamples does not follow it
            d->setNSamples(3);
            d->setkNNSamples(4);
            d->setDist2Threshold(90.5);
            d->setShadowValue(300);
            d->setShadowThreshold(0.25);
            d->setHistory(9);
            d->setDetectShadows(true);
            if (d->getNSamples() != 3 || d->getkNNSamples() != 4 || d->getDist2Threshold() != 90.5 ||
                d->getShadowValue() != 44 || d->getShadowThreshold() != 0.25 || d->getHistory() != 9 || !d->getDetectShadows())
                return 16;
            d->setNSamples(16);
            if (d->getkNNSamples() != 4) return 17;
        }
        std::unique_ptr<tbdk::BackgroundSubtractorKNN> m = tbdk::createBackgroundSubtractorKNN(ctx, history);
        if (m->getHistory() != history || m->getNSamples() != 7 || m->getkNNSamples() != 2 || !m->getDetectShadows() ||
            m->getShadowValue() != 127 || m->getDist2Threshold() != 400.0 || m->getShadowThreshold() != 0.5 || m->frames() != 0)
            return 7;
        const int mpitch = w + 13;
        uint8_t *dframes = nullptr, *dmasks = nullptr, *dbg = nullptr;
        uint64_t* dstate = nullptr;
        if (hipMalloc(&dframes, frames.size()) != hipSuccess || hipMalloc(&dmasks, (size_t)mpitch * h * n) != hipSuccess ||
            hipMalloc(&dbg, (size_t)w * h) != hipSuccess || hipMalloc(&dstate, 8) != hipSuccess)
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
        // what may not change, and the rates the reference has no defined result for
        int thrown = 0;
        try {
            m->setNSamples(3);
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
        const double bad_rates[] = {0.0, 1.25, 1e-13, std::nan("")};
        for (double r : bad_rates) {
            try {
                m->apply(tbdk::GpuMatView{dframes, w, h, w, tbdk::DEPTH_8U, 1}, tbdk::GpuImage{dmasks, w, h, mpitch}, r);
            } catch (const tbdk::Error& e) {
                thrown += e.code() == TBDK_EINVAL;
            }
        }
        try {
            m->apply(tbdk::GpuMatView{dframes, w, h, w - 1, tbdk::DEPTH_8U, 1}, tbdk::GpuImage{dmasks, w, h, mpitch});
        } catch (const tbdk::Error& e) {
            thrown += e.code() == TBDK_EINVAL;
        }
        try {
            m->apply(tbdk::GpuMatView{nullptr, w, h, w, tbdk::DEPTH_8U, 1}, tbdk::GpuImage{dmasks, w, h, mpitch});
        } catch (const tbdk::Error& e) {
            thrown += e.code() == TBDK_EINVAL;
        }
        if (thrown != 9 || m->frames() != n || m->getHistory() != history || m->getNSamples() != 7) return 14;
        // the state after the refused calls is the state after the n frames
        if (tbdk_knn_get_model(m->get(), nullptr, nullptr, nullptr, nullptr, dstate, nullptr) != TBDK_OK) return 18;
        if (hipDeviceSynchronize() != hipSuccess) return 10;
        std::vector<uint8_t> pm((size_t)mpitch * h * n), bg((size_t)w * h);
        uint64_t state = 0;
        (void)hipMemcpy(pm.data(), dmasks, pm.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpy(bg.data(), dbg, bg.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpy(&state, dstate, 8, hipMemcpyDeviceToHost);
        FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 11;
        for (int r = 0; r < h * n; ++r) {
            std::fwrite(pm.data() + (size_t)r * mpitch, 1, w, o);
            for (int x = w; x < mpitch; ++x)
                if (pm[(size_t)r * mpitch + x] != 7) return 12;  // the mask's padding was written
        }
        std::fwrite(bg.data(), 1, bg.size(), o);
        std::fwrite(&state, 1, 8, o);
        if (std::fclose(o) != 0) return 13;
        m->setShadowValue(0);
        m->setkNNSamples(1);
        if (m->getShadowValue() != 0 || m->getkNNSamples() != 1) return 19;
        m->reset();
        if (m->frames() != 0) return 15;
        std::printf("facade BackgroundSubtractorKNN: ok\n");
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("%s\n", e.what());
        return want_gpu ? 1 : (e.code() == TBDK_ENODEV ? 0 : 2);
    }
}
