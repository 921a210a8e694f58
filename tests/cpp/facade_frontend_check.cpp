// facade_frontend_check.cpp — the front-end and detection-driven parts of the
// C++ facade (include/tbdk.hpp: cuda::cvtColor, cuda::resize, DetectingTbd)
// against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV)
//   GPU    : cvtColor -> resize equals the fused call; DetectingTbd::step equals
//            cvtColor -> HOG::detectMultiScale -> TbdLoop::step
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const int W = 320, H = 240, DW = 256, DH = 192;
    tbdk_tbd_detect_config dc = tbdk::DetectingTbd::defaultConfig(DW, DH);
    if (dc.hog.nlevels != 15 || dc.hog.hit_threshold != 0.45 || dc.make_gray != 1 || dc.src_cn != 3 ||
        dc.confidence_mode != 0 || dc.width != DW || dc.src_height != DH)
        return 2;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        std::vector<uint8_t> h((size_t)W * H * 3);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c)
                    h[((size_t)y * W + x) * 3 + c] = (uint8_t)((x * (7 + c) + y * 13 + ((x / 9) ^ (y / 7)) * 40) & 255);
        uint8_t *bgr, *gray, *small, *fused;
        if (hipMalloc(&bgr, h.size()) || hipMalloc(&gray, (size_t)W * H) || hipMalloc(&small, (size_t)DW * DH) ||
            hipMalloc(&fused, (size_t)DW * DH))
            return 4;
        (void)hipMemcpy(bgr, h.data(), h.size(), hipMemcpyHostToDevice);
        tbdk::GpuMatView vb{bgr, W, H, W * 3, tbdk::DEPTH_8U, 3}, vg{gray, W, H, W, tbdk::DEPTH_8U, 1};
        tbdk::GpuMatView vs{small, DW, DH, DW, tbdk::DEPTH_8U, 1};
        tbdk::cuda::cvtColor(ctx, vb, vg, TBDK_COLOR_BGR2GRAY);
        tbdk::cuda::resize(ctx, vg, vs);
        tbdk::check(tbdk_cvt_resize_gray_u8(ctx.get(), bgr, W, H, W * 3, TBDK_COLOR_BGR2GRAY, fused, DW, DH, DW, nullptr),
                    "tbdk_cvt_resize_gray_u8");
        std::vector<uint8_t> a((size_t)DW * DH), b((size_t)DW * DH);
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(a.data(), small, a.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpy(b.data(), fused, b.size(), hipMemcpyDeviceToHost);
        if (a != b) return 5;
        bool threw = false;
        try {  // a code that is not built, a channel count that does not fit
            tbdk::cuda::cvtColor(ctx, vb, vg, 5);
        } catch (const tbdk::Error& e) {
            threw = e.code() == TBDK_EINVAL;
        }
        if (!threw) return 6;
        threw = false;
        try {
            tbdk::cuda::resize(ctx, vg, vs, TBDK_INTER_CUBIC);
        } catch (const tbdk::Error& e) {
            threw = e.code() == TBDK_EINVAL;
        }
        if (!threw) return 6;

        // the detection-driven step against the same calls made one by one
        auto hog = tbdk::cuda::HOG::create(ctx, {48, 96});
        std::vector<float> svm(hog->getDescriptorSize() + 1, 0.f);
        svm.back() = 1.f;  // bias only: every window scores 1
        hog->setSVMDetector(svm);
        hog->setNumLevels(3);
        tbdk_tbd_config lc = tbdk::TbdLoop::defaultConfig(DW, DH);
        lc.track_confidence_threshold = -1;
        tbdk::TbdLoop la(ctx, lc), lb(ctx, lc);
        dc.src_width = W, dc.src_height = H, dc.resize = 1, dc.confidence_mode = 1;
        tbdk::DetectingTbd det(ctx, la, *hog, dc);
        for (int f = 0; f < 3; ++f) {
            std::vector<tbdk_detection> used;
            const tbdk_frame_metrics ma = det.step(vb, f, &used);
            std::vector<double> conf;
            const tbdk::GpuImage gi{small, DW, DH, DW};
            const auto rects = hog->detectMultiScale(gi, 1, &conf);
            std::vector<tbdk_detection> mine;
            for (size_t i = 0; i < rects.size(); ++i)
                mine.push_back(tbdk_detection{-1, rects[i].x, rects[i].y, rects[i].width, rects[i].height, conf[i]});
            const tbdk_frame_metrics mb = lb.step(gi, f, mine);
            if (used.empty() || used.size() != mine.size()) return 7;
            for (size_t i = 0; i < used.size(); ++i)
                if (used[i].id != -1 || used[i].x != mine[i].x || used[i].y != mine[i].y ||
                    used[i].width != mine[i].width || used[i].height != mine[i].height ||
                    used[i].confidence != mine[i].confidence)
                    return 8;
            if (ma.ntracks != mb.ntracks || ma.lk_points != mb.lk_points || ma.klt_predicted != mb.klt_predicted)
                return 9;
            std::printf("frame %d: %zu detections, %d tracks\n", f, used.size(), ma.ntracks);
        }
        return la.tracks().size() == lb.tracks().size() && !la.tracks().empty() ? 0 : 10;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 7;
    }
}
