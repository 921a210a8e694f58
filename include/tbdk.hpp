// tbdk.hpp — header-only C++ facade over the C ABI (tbdk.h), shaped like the
// reference's cv::cuda interfaces for this path so a caller of
//   cv::cuda::SparsePyrLKOpticalFlow   (modules/cudaoptflow/include/opencv2/cudaoptflow.hpp:160-180)
//   cv::cuda::CornersDetector          (modules/cudaimgproc/include/opencv2/cudaimgproc.hpp:570-604)
//   cv::cuda::pyrDown / warpAffine     (modules/cudawarping/include/opencv2/cudawarping.hpp:126,201)
//   cv::cuda::cvtColor / resize        (cudaimgproc.hpp, cudawarping.hpp: 8-bit, the sample's codes, INTER_LINEAR)
// changes types, not call structure.  Differences from the reference:
//   - images are non-owning device views (GpuImage) instead of GpuMat; the
//     caller owns all device memory;
//   - numerics follow the CPU reference (calcOpticalFlowPyrLK,
//     goodFeaturesToTrack, warpAffine), not the CUDA module's float variants;
//   - errors: tbdk::Error (a std::runtime_error carrying the TBDK_E* code)
//     where the reference throws cv::Exception.
#ifndef TBDK_HPP
#define TBDK_HPP

#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "tbdk.h"

namespace tbdk {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& what) : std::runtime_error(what + ": " + name(code)), code_(code) {}
    int code() const { return code_; }
    static const char* name(int code)
    {
        switch (code) {
        case TBDK_EINVAL: return "TBDK_EINVAL (bad argument)";
        case TBDK_EHIP: return "TBDK_EHIP (HIP runtime error)";
        case TBDK_ENOMEM: return "TBDK_ENOMEM (device allocation failed)";
        case TBDK_ENODEV: return "TBDK_ENODEV (no such device)";
        default: return "unknown status";
        }
    }

private:
    int code_;
};

inline void check(int rc, const char* what)
{
    if (rc != TBDK_OK) throw Error(rc, what);
}

struct Size {
    int width = 0, height = 0;
};

// cv::TermCriteria: type is COUNT, EPS or both
struct TermCriteria {
    enum Type { COUNT = 1, MAX_ITER = COUNT, EPS = 2 };
    int type = COUNT | EPS, maxCount = 20;
    double epsilon = 0.03;
};

// Non-owning device u8 image view (GpuMat of CV_8UC1 analogue).
struct GpuImage {
    uint8_t* data = nullptr;
    int width = 0, height = 0, pitch = 0;  // pitch in bytes
};

// Element depths of a typed view (cv::Mat depth codes): the types
// cv::cuda::SparsePyrLKOpticalFlow::calc accepts (cudaoptflow/src/pyrlk.cpp:189-205)
constexpr int DEPTH_8U = 0, DEPTH_16U = 2, DEPTH_32F = 5;

// Non-owning device image view with a depth and cn interleaved channels
// (GpuMat of CV_8UC1..4 / CV_16UC1..4 / CV_32FC1..4 analogue)
struct GpuMatView {
    void* data = nullptr;
    int width = 0, height = 0, pitch = 0;  // pitch in bytes
    int depth = DEPTH_8U, cn = 1;
};

// One context per (host thread, device); owns GFTT scratch and timing records.
class Context {
public:
    explicit Context(int device = 0) { check(tbdk_ctx_create(device, &h_), "tbdk_ctx_create"); }
    ~Context() { tbdk_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    tbdk_ctx* get() const { return h_; }
    int device() const { return tbdk_ctx_device(h_); }

private:
    tbdk_ctx* h_ = nullptr;
};

// Padded pyramid with Scharr derivative planes (buildOpticalFlowPyramid with
// withDerivatives=true, video/src/lkpyramid.cpp:697-793); depth TBDK_DEPTH_16F
// gives the fp16 pixel path's pyramid (tbdk_pyr_create_f16).
class Pyramid {
public:
    // depth TBDK_DEPTH_8U or TBDK_DEPTH_32F (cn 1..4 channels, interleaved), TBDK_DEPTH_16F (one channel)
    Pyramid(Context& ctx, int width, int height, int max_level, Size win = {21, 21}, int depth = TBDK_DEPTH_8U,
            int cn = 1)
        : ctx_(&ctx)
    {
        if (cn != 1 && depth == TBDK_DEPTH_16F) throw Error(TBDK_EINVAL, "Pyramid: fp16 pyramids are one-channel");
        if (depth == TBDK_DEPTH_16F)
            check(tbdk_pyr_create_f16(ctx.get(), width, height, max_level, win.width, win.height, &p_),
                  "tbdk_pyr_create_f16");
        else if (depth == TBDK_DEPTH_32F && cn != 1)
            check(tbdk_pyr_create_f32_cn(ctx.get(), width, height, cn, max_level, win.width, win.height, &p_),
                  "tbdk_pyr_create_f32_cn");
        else if (depth == TBDK_DEPTH_32F)
            check(tbdk_pyr_create_f32(ctx.get(), width, height, max_level, win.width, win.height, &p_),
                  "tbdk_pyr_create_f32");
        else if (cn != 1)
            check(tbdk_pyr_create_cn(ctx.get(), width, height, cn, max_level, win.width, win.height, &p_),
                  "tbdk_pyr_create_cn");
        else
            check(tbdk_pyr_create(ctx.get(), width, height, max_level, win.width, win.height, &p_), "tbdk_pyr_create");
    }
    ~Pyramid() { tbdk_pyr_destroy(ctx_->get(), &p_); }
    Pyramid(const Pyramid&) = delete;
    Pyramid& operator=(const Pyramid&) = delete;
    void build(const GpuImage& img, void* stream = nullptr)
    {
        if (img.width != p_.lv[0].width || img.height != p_.lv[0].height) throw Error(TBDK_EINVAL, "Pyramid::build");
        check(tbdk_pyr_build(ctx_->get(), img.data, img.pitch, &p_, stream), "tbdk_pyr_build");
    }
    // fp16 frame (pitch in bytes) into an fp16 pyramid
    void build_f16(const uint16_t* data, int width, int height, int pitch, void* stream = nullptr)
    {
        if (width != p_.lv[0].width || height != p_.lv[0].height) throw Error(TBDK_EINVAL, "Pyramid::build_f16");
        check(tbdk_pyr_build_f16(ctx_->get(), data, pitch, &p_, stream), "tbdk_pyr_build_f16");
    }
    // 16U / 32F frames (pitch in bytes) into an fp32 pyramid (the CUDA class's other depths)
    void build_u16(const uint16_t* data, int width, int height, int pitch, void* stream = nullptr)
    {
        if (width != p_.lv[0].width || height != p_.lv[0].height) throw Error(TBDK_EINVAL, "Pyramid::build_u16");
        check(tbdk_pyr_build_u16(ctx_->get(), data, pitch, &p_, stream), "tbdk_pyr_build_u16");
    }
    void build_f32(const float* data, int width, int height, int pitch, void* stream = nullptr)
    {
        if (width != p_.lv[0].width || height != p_.lv[0].height) throw Error(TBDK_EINVAL, "Pyramid::build_f32");
        check(tbdk_pyr_build_f32(ctx_->get(), data, pitch, &p_, stream), "tbdk_pyr_build_f32");
    }
    // any typed view the pyramid takes: u8 into either depth, u16 / fp32 into fp32
    // pyramids, with the pyramid's channel count
    void build(const GpuMatView& img, void* stream = nullptr)
    {
        if (img.width != p_.lv[0].width || img.height != p_.lv[0].height || img.cn != channels())
            throw Error(TBDK_EINVAL, "Pyramid::build");
        if (img.depth == DEPTH_8U)
            check(tbdk_pyr_build(ctx_->get(), static_cast<const uint8_t*>(img.data), img.pitch, &p_, stream),
                  "tbdk_pyr_build");
        else if (img.depth == DEPTH_16U)
            check(tbdk_pyr_build_u16(ctx_->get(), static_cast<const uint16_t*>(img.data), img.pitch, &p_, stream),
                  "tbdk_pyr_build_u16");
        else if (img.depth == DEPTH_32F)
            check(tbdk_pyr_build_f32(ctx_->get(), static_cast<const float*>(img.data), img.pitch, &p_, stream),
                  "tbdk_pyr_build_f32");
        else
            throw Error(TBDK_EINVAL, "Pyramid::build: depth");
    }
    int depth() const { return p_.depth; }
    int channels() const { return p_.cn > 1 ? p_.cn : 1; }
    const tbdk_pyr& get() const { return p_; }
    int levels() const { return p_.nlevels; }

private:
    Context* ctx_;
    tbdk_pyr p_{};
};

namespace cuda {

// cv::cuda::SparsePyrLKOpticalFlow (cudaoptflow.hpp:160-180; impl pyrlk.cpp:301-350).
// Like the reference implementation object it caches the prev/next pyramids
// (prevPyr_/nextPyr_, pyrlk.cpp:101-102) and rebuilds them per calc() on images.
class SparsePyrLKOpticalFlow {
public:
    static std::unique_ptr<SparsePyrLKOpticalFlow> create(Context& ctx, Size winSize = {21, 21}, int maxLevel = 3,
                                                          int iters = 30, bool useInitialFlow = false)
    {
        return std::unique_ptr<SparsePyrLKOpticalFlow>(
            new SparsePyrLKOpticalFlow(ctx, winSize, maxLevel, iters, useInitialFlow));
    }

    Size getWinSize() const { return win_; }
    void setWinSize(Size s) { win_ = s; pyr_[0].reset(); pyr_[1].reset(); }
    int getMaxLevel() const { return max_level_; }
    void setMaxLevel(int v) { max_level_ = v; pyr_[0].reset(); pyr_[1].reset(); }
    int getNumIters() const { return iters_; }
    void setNumIters(int v) { iters_ = v; }
    bool getUseInitialFlow() const { return use_initial_flow_; }
    void setUseInitialFlow(bool v) { use_initial_flow_ = v; }
    // CPU-path extras (calcOpticalFlowPyrLK arguments): epsilon, flags, minEigThreshold
    void setEpsilon(double e) { eps_ = e; }
    void setMinEigThreshold(float t) { min_eig_ = t; }
    void setGetMinEigenvals(bool v) { min_eig_flag_ = v; }

    // calc(prevImg, nextImg, prevPts, nextPts, status, err, stream): all point
    // buffers are device arrays of n entries (float2 points, u8 status, f32 err);
    // err may be null (noArray()).
    void calc(const GpuImage& prevImg, const GpuImage& nextImg, const float* prevPts, float* nextPts,
              uint8_t* status, float* err, int n, void* stream = nullptr)
    {
        if (n == 0) return;  // reference: empty prevPts releases the outputs (pyrlk.cpp:221-227)
        for (int i = 0; i < 2; ++i) {
            const GpuImage& im = i == 0 ? prevImg : nextImg;
            if (!pyr_[i] || pyr_[i]->get().lv[0].width != im.width || pyr_[i]->get().lv[0].height != im.height ||
                pyr_[i]->depth() != TBDK_DEPTH_8U || pyr_[i]->channels() != 1)
                pyr_[i].reset(new Pyramid(*ctx_, im.width, im.height, max_level_, win_));
            pyr_[i]->build(im, stream);
        }
        calc(*pyr_[0], *pyr_[1], prevPts, nextPts, status, err, n, stream);
    }

    // Typed images (the CUDA class's accepted types, pyrlk.cpp:189-205): CV_8UC1..4
    // on the u8 path, CV_16UC1..4 / CV_32FC1..4 on the fp32 pixel path; both
    // images of one type.  The pyramids are cached per (size, depth, channels).
    void calc(const GpuMatView& prevImg, const GpuMatView& nextImg, const float* prevPts, float* nextPts,
              uint8_t* status, float* err, int n, void* stream = nullptr)
    {
        if (n == 0) return;
        if (prevImg.depth != nextImg.depth || prevImg.cn != nextImg.cn) throw Error(TBDK_EINVAL, "calc: types");
        // the CUDA class asserts cn 1, 3 or 4 on its frames (pyrlk.cpp:142,228);
        // prebuilt Pyramids (below) take any count, as calcOpticalFlowPyrLK does
        if (prevImg.cn != 1 && prevImg.cn != 3 && prevImg.cn != 4) throw Error(TBDK_EINVAL, "calc: channels");
        const int pdepth = prevImg.depth == DEPTH_8U ? TBDK_DEPTH_8U : TBDK_DEPTH_32F;
        for (int i = 0; i < 2; ++i) {
            const GpuMatView& im = i == 0 ? prevImg : nextImg;
            if (!pyr_[i] || pyr_[i]->get().lv[0].width != im.width || pyr_[i]->get().lv[0].height != im.height ||
                pyr_[i]->depth() != pdepth || pyr_[i]->channels() != im.cn)
                pyr_[i].reset(new Pyramid(*ctx_, im.width, im.height, max_level_, win_, pdepth, im.cn));
            pyr_[i]->build(im, stream);
        }
        calc(*pyr_[0], *pyr_[1], prevPts, nextPts, status, err, n, stream);
    }

    // Pyramids given explicitly (calcOpticalFlowPyrLK accepts prebuilt pyramids,
    // video/src/lkpyramid.cpp:1270-1324): the TBD loop reuses prev frame's.
    void calc(const Pyramid& prev, const Pyramid& next, const float* prevPts, float* nextPts, uint8_t* status,
              float* err, int n, void* stream = nullptr, int32_t* iters = nullptr)
    {
        tbdk_lk_params p;
        p.win_w = win_.width;
        p.win_h = win_.height;
        p.max_level = max_level_;
        p.max_count = iters_;
        p.epsilon = eps_;
        p.flags = (use_initial_flow_ ? TBDK_OPTFLOW_USE_INITIAL_FLOW : 0) |
                  (min_eig_flag_ ? TBDK_OPTFLOW_LK_GET_MIN_EIGENVALS : 0);
        p.min_eig_threshold = min_eig_;
        p.impl = 0;
        check(tbdk_lk_sparse(ctx_->get(), &prev.get(), &next.get(), prevPts, nextPts, status, err, iters, n, &p,
                             stream),
              "tbdk_lk_sparse");
    }

    // calc with the forward-backward check of the reference's KLT tracker samples
    // (checkedTrace, samples/python/lk_homography.py:42-47; tbdk_lk_sparse_fb):
    // the tracked points are tracked back nextImg -> prevImg, and status stays 1
    // only where both passes have status 1 and max(|dx|, |dy|) between prevPts
    // and the point tracked back is below backThreshold.  nextPts and err are
    // calc's; fbErr (n floats, may be null) gets that distance, +inf where
    // either pass lost the point.  8-bit one-channel images.
    void calcChecked(const GpuImage& prevImg, const GpuImage& nextImg, const float* prevPts, float* nextPts,
                     uint8_t* status, int n, float backThreshold = 1.0f, float* err = nullptr,
                     float* fbErr = nullptr, void* stream = nullptr)
    {
        if (n == 0) return;
        for (int i = 0; i < 2; ++i) {
            const GpuImage& im = i == 0 ? prevImg : nextImg;
            if (!pyr_[i] || pyr_[i]->get().lv[0].width != im.width || pyr_[i]->get().lv[0].height != im.height ||
                pyr_[i]->depth() != TBDK_DEPTH_8U || pyr_[i]->channels() != 1)
                pyr_[i].reset(new Pyramid(*ctx_, im.width, im.height, max_level_, win_));
            pyr_[i]->build(im, stream);
        }
        calcChecked(*pyr_[0], *pyr_[1], prevPts, nextPts, status, n, backThreshold, err, fbErr, stream);
    }

    // the same on prebuilt pyramids; backPts (n float2, may be null): the points tracked back
    void calcChecked(const Pyramid& prev, const Pyramid& next, const float* prevPts, float* nextPts, uint8_t* status,
                     int n, float backThreshold = 1.0f, float* err = nullptr, float* fbErr = nullptr,
                     void* stream = nullptr, float* backPts = nullptr, int32_t* iters = nullptr)
    {
        tbdk_lk_params p;
        p.win_w = win_.width;
        p.win_h = win_.height;
        p.max_level = max_level_;
        p.max_count = iters_;
        p.epsilon = eps_;
        p.flags = (use_initial_flow_ ? TBDK_OPTFLOW_USE_INITIAL_FLOW : 0) |
                  (min_eig_flag_ ? TBDK_OPTFLOW_LK_GET_MIN_EIGENVALS : 0);
        p.min_eig_threshold = min_eig_;
        p.impl = 0;
        check(tbdk_lk_sparse_fb(ctx_->get(), &prev.get(), &next.get(), prevPts, nextPts, status, err, iters, backPts,
                                fbErr, n, &p, backThreshold, stream),
              "tbdk_lk_sparse_fb");
    }

private:
    SparsePyrLKOpticalFlow(Context& ctx, Size win, int max_level, int iters, bool uif)
        : ctx_(&ctx), win_(win), max_level_(max_level), iters_(iters), use_initial_flow_(uif)
    {
    }
    Context* ctx_;
    Size win_;
    int max_level_, iters_;
    bool use_initial_flow_;
    double eps_ = 0.01;
    float min_eig_ = 1e-4f;
    bool min_eig_flag_ = false;
    std::unique_ptr<Pyramid> pyr_[2];
};

// cv::cuda::DensePyrLKOpticalFlow (cudaoptflow.hpp:182-208; impl pyrlk.cpp:238-299,
// 352-397): the PyrLK of every level-0 pixel, written as a CV_32FC2 flow field.
// useInitialFlow is kept for the interface and, as in the reference, has no effect.
class DensePyrLKOpticalFlow {
public:
    static std::unique_ptr<DensePyrLKOpticalFlow> create(Context& ctx, Size winSize = {13, 13}, int maxLevel = 3,
                                                         int iters = 30, bool useInitialFlow = false)
    {
        return std::unique_ptr<DensePyrLKOpticalFlow>(
            new DensePyrLKOpticalFlow(ctx, winSize, maxLevel, iters, useInitialFlow));
    }

    Size getWinSize() const { return win_; }
    void setWinSize(Size s) { win_ = s; pyr_[0].reset(); pyr_[1].reset(); }
    int getMaxLevel() const { return max_level_; }
    void setMaxLevel(int v) { max_level_ = v; pyr_[0].reset(); pyr_[1].reset(); }
    int getNumIters() const { return iters_; }
    void setNumIters(int v) { iters_ = v; }
    bool getUseInitialFlow() const { return use_initial_flow_; }
    void setUseInitialFlow(bool v) { use_initial_flow_ = v; }

    // calc(I0, I1, flow, stream): flow is a device CV_32FC2 image (flowPitch bytes
    // per row); status, when given, is a device u8 plane of statusPitch bytes per row.
    void calc(const GpuImage& I0, const GpuImage& I1, float* flow, int flowPitch, void* stream = nullptr,
              uint8_t* status = nullptr, int statusPitch = 0)
    {
        for (int i = 0; i < 2; ++i) {
            const GpuImage& im = i == 0 ? I0 : I1;
            if (!pyr_[i] || pyr_[i]->get().lv[0].width != im.width || pyr_[i]->get().lv[0].height != im.height)
                pyr_[i].reset(new Pyramid(*ctx_, im.width, im.height, max_level_, win_));
            pyr_[i]->build(im, stream);
        }
        tbdk_lk_params p;
        p.win_w = win_.width;
        p.win_h = win_.height;
        p.max_level = max_level_;
        p.max_count = iters_;
        p.epsilon = 0.01;
        p.flags = use_initial_flow_ ? TBDK_OPTFLOW_USE_INITIAL_FLOW : 0;
        p.min_eig_threshold = 1e-4f;
        p.impl = 0;
        check(tbdk_lk_dense(ctx_->get(), &pyr_[0]->get(), &pyr_[1]->get(), flow, flowPitch, status, statusPitch, &p,
                            stream),
              "tbdk_lk_dense");
    }

private:
    DensePyrLKOpticalFlow(Context& ctx, Size win, int max_level, int iters, bool uif)
        : ctx_(&ctx), win_(win), max_level_(max_level), iters_(iters), use_initial_flow_(uif)
    {
    }
    Context* ctx_;
    Size win_;
    int max_level_, iters_;
    bool use_initial_flow_;
    std::unique_ptr<Pyramid> pyr_[2];
};

// cv::cuda::CornersDetector from createGoodFeaturesToTrackDetector(srcType,
// maxCorners, qualityLevel, minDistance, blockSize=3, useHarris=false, harrisK=0.04)
// (cudaimgproc.hpp:582,603-604).  detect() runs on the whole image; detectRois()
// is the batched per-box form the TBD loop uses (one launch set for all boxes).
// A GpuImage is CV_8UC1; a GpuMatView carries its depth: DEPTH_8U, DEPTH_32F
// (CV_32FC1, finite pixels) or DEPTH_16U (the 32F result of the same values),
// one channel (tbdk_gftt_rois_px); any other view throws Error(TBDK_EINVAL).
class CornersDetector {
public:
    static std::unique_ptr<CornersDetector> create(Context& ctx, int maxCorners = 1000, double qualityLevel = 0.01,
                                                   double minDistance = 0.0, int blockSize = 3,
                                                   bool useHarrisDetector = false, double harrisK = 0.04)
    {
        if (blockSize < 1 || blockSize > 63) throw Error(TBDK_EINVAL, "createGoodFeaturesToTrackDetector");
        return std::unique_ptr<CornersDetector>(
            new CornersDetector(ctx, maxCorners, qualityLevel, minDistance, blockSize, useHarrisDetector, harrisK));
    }

    // corners: device, maxCorners float2; count: device int32, the corners found
    // (never negative: a frame of any size and any maxCorners is served, the large
    // ones by the wide selection path of tbdk_gftt_rois).  The count stays on the
    // device (no host sync).
    void detect(const GpuImage& image, float* corners, int32_t* count, void* stream = nullptr)
    {
        tbdk_roi r{0, 0, image.width, image.height};
        detectRois(image, &r, 1, corners, count, stream);
    }

    // CornersDetector::detect(image, corners, mask, stream) (gftt.cpp:98): mask is a
    // u8 image of the image's size; the quality threshold comes from the maximum
    // over its non-zero pixels and only they can be corners (tbdk_gftt_rois_masked)
    void detect(const GpuImage& image, const GpuImage& mask, float* corners, int32_t* count, void* stream = nullptr)
    {
        tbdk_roi r{0, 0, image.width, image.height};
        detectRois(image, mask, &r, 1, corners, count, stream);
    }

    // rois: host array; corners: device nroi x maxCorners float2; counts: device nroi int32
    void detectRois(const GpuImage& image, const tbdk_roi* rois, int nroi, float* corners, int32_t* counts,
                    void* stream = nullptr)
    {
        check(tbdk_gftt_rois(ctx_->get(), image.data, image.width, image.height, image.pitch, rois, nroi, &p_,
                             corners, counts, stream),
              "tbdk_gftt_rois");
    }

    // ... under a mask of the image's size, each ROI reading its own rectangle of it
    void detectRois(const GpuImage& image, const GpuImage& mask, const tbdk_roi* rois, int nroi, float* corners,
                    int32_t* counts, void* stream = nullptr)
    {
        if (!mask.data || mask.width != image.width || mask.height != image.height)
            throw Error(TBDK_EINVAL, "CornersDetector: mask size");
        check(tbdk_gftt_rois_masked(ctx_->get(), image.data, image.width, image.height, image.pitch, mask.data,
                                    mask.pitch, rois, nroi, &p_, corners, counts, stream),
              "tbdk_gftt_rois_masked");
    }

    // ... on a typed view (8U, 16U or 32F, one channel), without and with a mask
    void detect(const GpuMatView& image, float* corners, int32_t* count, void* stream = nullptr)
    {
        tbdk_roi r{0, 0, image.width, image.height};
        detectRois(image, &r, 1, corners, count, stream);
    }
    void detect(const GpuMatView& image, const GpuImage& mask, float* corners, int32_t* count, void* stream = nullptr)
    {
        tbdk_roi r{0, 0, image.width, image.height};
        detectRois(image, mask, &r, 1, corners, count, stream);
    }
    void detectRois(const GpuMatView& image, const tbdk_roi* rois, int nroi, float* corners, int32_t* counts,
                    void* stream = nullptr)
    {
        check(tbdk_gftt_rois_px(ctx_->get(), image.data, pixOf(image, "CornersDetector: image type"), image.width,
                                image.height, image.pitch, nullptr, 0, rois, nroi, &p_, corners, counts, stream),
              "tbdk_gftt_rois_px");
    }
    void detectRois(const GpuMatView& image, const GpuImage& mask, const tbdk_roi* rois, int nroi, float* corners,
                    int32_t* counts, void* stream = nullptr)
    {
        if (!mask.data || mask.width != image.width || mask.height != image.height)
            throw Error(TBDK_EINVAL, "CornersDetector: mask size");
        check(tbdk_gftt_rois_px(ctx_->get(), image.data, pixOf(image, "CornersDetector: image type"), image.width,
                                image.height, image.pitch, mask.data, mask.pitch, rois, nroi, &p_, corners, counts,
                                stream),
              "tbdk_gftt_rois_px");
    }

    // TBDK_PIX_* of a one-channel 8U / 16U / 32F view
    static int pixOf(const GpuMatView& v, const char* what)
    {
        if (v.cn == 1 && v.depth == DEPTH_8U) return TBDK_PIX_U8;
        if (v.cn == 1 && v.depth == DEPTH_16U) return TBDK_PIX_U16;
        if (v.cn == 1 && v.depth == DEPTH_32F) return TBDK_PIX_F32;
        throw Error(TBDK_EINVAL, what);
    }

private:
    CornersDetector(Context& ctx, int maxc, double q, double md, int block, bool harris, double k) : ctx_(&ctx)
    {
        p_.max_corners = maxc;
        p_.quality_level = q;
        p_.min_distance = md;
        p_.block_size = block;
        p_.use_harris = harris ? 1 : 0;
        p_.harris_k = k;
    }
    Context* ctx_;
    tbdk_gftt_params p_{};
};

// cv::cuda::createMinEigenValCorner(CV_8UC1, blockSize, 3)->compute (harris false) and
// cv::cuda::createHarrisCorner(CV_8UC1, blockSize, 3, k)->compute (harris true)
// (cudaimgproc.hpp:548-566): dst is a device float plane (dst_pitch bytes)
inline void cornerResponse(Context& ctx, const GpuImage& src, float* dst, int dst_pitch, int blockSize = 3,
                           bool harris = false, double k = 0.04, void* stream = nullptr)
{
    check(tbdk_corner_response(ctx.get(), src.data, src.width, src.height, src.pitch, dst, dst_pitch, blockSize,
                               harris ? 1 : 0, k, stream),
          "tbdk_corner_response");
}

// ... of a typed view: createMinEigenValCorner / createHarrisCorner(CV_8UC1 or CV_32FC1, ...),
// and 16U as the 32F result of the same values (tbdk_corner_response_px)
inline void cornerResponse(Context& ctx, const GpuMatView& src, float* dst, int dst_pitch, int blockSize = 3,
                           bool harris = false, double k = 0.04, void* stream = nullptr)
{
    check(tbdk_corner_response_px(ctx.get(), src.data, CornersDetector::pixOf(src, "cornerResponse: image type"),
                                  src.width, src.height, src.pitch, dst, dst_pitch, blockSize, harris ? 1 : 0, k,
                                  stream),
          "tbdk_corner_response_px");
}

// cv::cuda::pyrDown (cudawarping.hpp:201): dst must be ((w+1)/2, (h+1)/2)
inline void pyrDown(Context& ctx, const GpuImage& src, GpuImage& dst, void* stream = nullptr)
{
    if (dst.width != (src.width + 1) / 2 || dst.height != (src.height + 1) / 2) throw Error(TBDK_EINVAL, "pyrDown");
    check(tbdk_pyr_down_u8(ctx.get(), src.data, src.width, src.height, src.pitch, dst.data, dst.pitch, stream),
          "tbdk_pyr_down_u8");
}

// cv::cuda::warpAffine(src, dst, M, dsize, flags, borderMode, borderValue, stream)
// (cudawarping.hpp:126); dsize is dst's size; M is a host 2x3 row-major matrix.
inline void warpAffine(Context& ctx, const GpuImage& src, GpuImage& dst, const double M[6],
                       int flags = TBDK_INTER_LINEAR, int borderMode = TBDK_BORDER_CONSTANT, int borderValue = 0,
                       void* stream = nullptr)
{
    check(tbdk_warp_affine_u8(ctx.get(), src.data, src.width, src.height, src.pitch, dst.data, dst.width,
                              dst.height, dst.pitch, M, flags, borderMode, borderValue, stream),
          "tbdk_warp_affine_u8");
}

// cv::cuda::cvtColor(src, dst, code, dcn, stream) (cudaimgproc.hpp) for 8-bit
// images: TBDK_COLOR_BGR2GRAY / RGB2GRAY / BGRA2GRAY / RGBA2GRAY / BGR2BGRA /
// GRAY2BGR with the CPU cv::cvtColor's bits.  dst is the caller's image of
// src's size and the code's channel count.
inline void cvtColor(Context& ctx, const GpuMatView& src, GpuMatView& dst, int code, void* stream = nullptr)
{
    const bool gray = code == TBDK_COLOR_BGR2GRAY || code == TBDK_COLOR_RGB2GRAY || code == TBDK_COLOR_BGRA2GRAY ||
                      code == TBDK_COLOR_RGBA2GRAY;
    const int scn = code == TBDK_COLOR_GRAY2BGR ? 1 : (code == TBDK_COLOR_BGRA2GRAY || code == TBDK_COLOR_RGBA2GRAY) ? 4 : 3;
    const int dcn = gray ? 1 : code == TBDK_COLOR_BGR2BGRA ? 4 : code == TBDK_COLOR_GRAY2BGR ? 3 : 0;
    if (src.depth != DEPTH_8U || dst.depth != DEPTH_8U || dcn == 0 || src.cn != scn || dst.cn != dcn ||
        dst.width != src.width || dst.height != src.height)
        throw Error(TBDK_EINVAL, "cvtColor");
    check(tbdk_cvt_color_u8(ctx.get(), static_cast<const uint8_t*>(src.data), src.width, src.height, src.pitch,
                            static_cast<uint8_t*>(dst.data), dst.pitch, code, stream),
          "tbdk_cvt_color_u8");
}

// cv::cuda::resize(src, dst, dsize, 0, 0, INTER_LINEAR, stream) (cudawarping.hpp)
// for 8-bit images of 1, 3 or 4 channels with the CPU cv::resize's bits; dsize
// is dst's size.  Only TBDK_INTER_LINEAR is built.
inline void resize(Context& ctx, const GpuMatView& src, GpuMatView& dst, int interpolation = TBDK_INTER_LINEAR,
                   void* stream = nullptr)
{
    if (interpolation != TBDK_INTER_LINEAR || src.depth != DEPTH_8U || dst.depth != DEPTH_8U || dst.cn != src.cn)
        throw Error(TBDK_EINVAL, "resize");
    check(tbdk_resize_linear_u8(ctx.get(), static_cast<const uint8_t*>(src.data), src.width, src.height, src.pitch,
                                src.cn, static_cast<uint8_t*>(dst.data), dst.width, dst.height, dst.pitch, stream),
          "tbdk_resize_linear_u8");
}

// cv::estimateRigidTransform(src1, src2, false, ransacMaxIters, ransacGoodRatio, 3)
// (video/tracking.hpp) on device point sets, batched: set i is points
// [offsets[i], offsets[i + 1]) of prevPts -> nextPts (device float2 arrays),
// status a device u8 mask or nullptr.  out[i].m is the 2x3 transform (the
// identity and valid = 0 where the reference returns an empty Mat), out[i].cx/cy
// the centre of boxes[i] mapped by it; iters / inliers may be nullptr
// (tbdk_box_propagate_ransac).
inline void estimateRigidTransform(Context& ctx, const float* prevPts, const float* nextPts, const uint8_t* status,
                                   const int32_t* offsets, const tbdk_roi* boxes, int nsets, tbdk_box_fit* out,
                                   int ransacMaxIters = 500, double ransacGoodRatio = 0.5, int minPoints = 3,
                                   int32_t* iters = nullptr, uint8_t* inliers = nullptr, void* stream = nullptr)
{
    tbdk_ransac_params p;
    check(tbdk_ransac_default_params(&p), "tbdk_ransac_default_params");
    p.max_iters = ransacMaxIters;
    p.good_ratio = ransacGoodRatio;
    check(tbdk_box_propagate_ransac(ctx.get(), prevPts, nextPts, status, offsets, boxes, nsets, minPoints, &p, out,
                                    iters, inliers, stream),
          "tbdk_box_propagate_ransac");
}

// cv::cuda::FarnebackOpticalFlow (cudaoptflow.hpp:210-252): create() with the
// reference's defaults, the getters/setters, calc(I0, I1, flow, stream).
// flow: device CV_32FC2 (dx, dy interleaved), flowPitch in bytes.
class FarnebackOpticalFlow {
public:
    static std::unique_ptr<FarnebackOpticalFlow> create(Context& ctx, int numLevels = 5, double pyrScale = 0.5,
                                                        bool fastPyramids = false, int winSize = 13,
                                                        int numIters = 10, int polyN = 5, double polySigma = 1.1,
                                                        int flags = 0)
    {
        std::unique_ptr<FarnebackOpticalFlow> f(new FarnebackOpticalFlow(ctx));
        f->p_ = tbdk_farneback_params{numLevels, pyrScale, fastPyramids ? 1 : 0, winSize, numIters, polyN,
                                      polySigma, flags};
        return f;
    }
    int getNumLevels() const { return p_.num_levels; }
    void setNumLevels(int v) { p_.num_levels = v; }
    double getPyrScale() const { return p_.pyr_scale; }
    void setPyrScale(double v) { p_.pyr_scale = v; }
    bool getFastPyramids() const { return p_.fast_pyramids != 0; }
    void setFastPyramids(bool v) { p_.fast_pyramids = v ? 1 : 0; }
    int getWinSize() const { return p_.win_size; }
    void setWinSize(int v) { p_.win_size = v; }
    int getNumIters() const { return p_.num_iters; }
    void setNumIters(int v) { p_.num_iters = v; }
    int getPolyN() const { return p_.poly_n; }
    void setPolyN(int v) { p_.poly_n = v; }
    double getPolySigma() const { return p_.poly_sigma; }
    void setPolySigma(double v) { p_.poly_sigma = v; }
    int getFlags() const { return p_.flags; }
    void setFlags(int v) { p_.flags = v; }

    void calc(const GpuImage& I0, const GpuImage& I1, float* flow, int flowPitch, void* stream = nullptr)
    {
        if (I0.width != I1.width || I0.height != I1.height || I0.pitch != I1.pitch)
            throw Error(TBDK_EINVAL, "FarnebackOpticalFlow::calc");
        check(tbdk_farneback(ctx_->get(), I0.data, I1.data, I0.width, I0.height, I0.pitch, flow, flowPitch, &p_,
                             stream),
              "tbdk_farneback");
    }

private:
    explicit FarnebackOpticalFlow(Context& ctx) : ctx_(&ctx) {}
    Context* ctx_;
    tbdk_farneback_params p_{};
};

}  // namespace cuda

// cv::Scalar for a border value: four doubles, each saturated to the pixel type per channel
struct Scalar {
    double val[4] = {0, 0, 0, 0};
    Scalar() = default;
    Scalar(double v0, double v1 = 0, double v2 = 0, double v3 = 0) : val{v0, v1, v2, v3} {}
};

namespace detail {
inline int warp_pix(const GpuMatView& src, const GpuMatView& dst, const char* what)
{
    if (src.depth != dst.depth || src.cn != dst.cn || (src.depth != DEPTH_8U && src.depth != DEPTH_32F))
        throw Error(TBDK_EINVAL, what);
    return src.depth == DEPTH_8U ? TBDK_PIX_U8 : TBDK_PIX_F32;
}
}  // namespace detail

// cv::cuda::remap(src, dst, xmap, ymap, interpolation, borderMode, borderValue, stream)
// (cudawarping.hpp) with the CPU cv::remap's bits, for CV_8UC1..4 and CV_32FC1..4.
// The maps are views of dst's size: two CV_32FC1 planes as cv::cuda::remap takes
// them, or cv::remap's other forms: one CV_32FC2 view (ymap empty), or a CV_16SC2
// view (depth DEPTH_16S, cn 2) with an optional CV_16UC1 fraction plane.
constexpr int DEPTH_16S = 3;
inline void remap(Context& ctx, const GpuMatView& src, GpuMatView& dst, const GpuMatView& xmap, const GpuMatView& ymap,
                  int interpolation, int borderMode = TBDK_BORDER_CONSTANT, const Scalar& borderValue = Scalar(),
                  void* stream = nullptr)
{
    const int pix = detail::warp_pix(src, dst, "remap");
    int kind;
    if (xmap.depth == DEPTH_32F && xmap.cn == 2) kind = TBDK_MAP_32FC2;
    else if (xmap.depth == DEPTH_32F && xmap.cn == 1 && ymap.data && ymap.depth == DEPTH_32F && ymap.cn == 1)
        kind = TBDK_MAP_32FC1;
    else if (xmap.depth == DEPTH_16S && xmap.cn == 2 && (!ymap.data || (ymap.depth == DEPTH_16U && ymap.cn == 1)))
        kind = TBDK_MAP_16SC2;
    else throw Error(TBDK_EINVAL, "remap: map types");
    if (xmap.width != dst.width || xmap.height != dst.height ||
        (kind != TBDK_MAP_32FC2 && ymap.data && (ymap.width != dst.width || ymap.height != dst.height)))
        throw Error(TBDK_EINVAL, "remap: map size");
    check(tbdk_remap(ctx.get(), src.data, pix, src.cn, src.width, src.height, src.pitch, dst.data, dst.width,
                     dst.height, dst.pitch, xmap.data, xmap.pitch, kind == TBDK_MAP_32FC2 ? nullptr : ymap.data,
                     ymap.pitch, kind, interpolation, borderMode, borderValue.val, stream),
          "tbdk_remap");
}

// remap by grid + sign * flow without storing the map: flow is the CV_32FC2 plane
// FarnebackOpticalFlow / DensePyrLKOpticalFlow write (dst's size).  sign +1 warps
// frame B onto frame A given the flow A -> B; -1 is opt_flow.py's warp_flow.
inline void remapFlow(Context& ctx, const GpuMatView& src, GpuMatView& dst, const GpuMatView& flow, int sign = 1,
                      int interpolation = TBDK_INTER_LINEAR, int borderMode = TBDK_BORDER_CONSTANT,
                      const Scalar& borderValue = Scalar(), void* stream = nullptr)
{
    const int pix = detail::warp_pix(src, dst, "remapFlow");
    if (flow.depth != DEPTH_32F || flow.cn != 2 || flow.width != dst.width || flow.height != dst.height)
        throw Error(TBDK_EINVAL, "remapFlow: flow must be CV_32FC2 of dst's size");
    check(tbdk_remap_flow(ctx.get(), src.data, pix, src.cn, src.width, src.height, src.pitch, dst.data, dst.width,
                          dst.height, dst.pitch, static_cast<const float*>(flow.data), flow.pitch, sign,
                          interpolation, borderMode, borderValue.val, stream),
          "tbdk_remap_flow");
}

// cv::cuda::warpPerspective(src, dst, M, dsize, flags, borderMode, borderValue, stream)
// (cudawarping.hpp) with the CPU cv::warpPerspective's bits; dsize is dst's size;
// M is a host 3x3 row-major matrix.
inline void warpPerspective(Context& ctx, const GpuMatView& src, GpuMatView& dst, const double M[9],
                            int flags = TBDK_INTER_LINEAR, int borderMode = TBDK_BORDER_CONSTANT,
                            const Scalar& borderValue = Scalar(), void* stream = nullptr)
{
    const int pix = detail::warp_pix(src, dst, "warpPerspective");
    check(tbdk_warp_perspective(ctx.get(), src.data, pix, src.cn, src.width, src.height, src.pitch, dst.data,
                                dst.width, dst.height, dst.pitch, M, flags, borderMode, borderValue.val, stream),
          "tbdk_warp_perspective");
}

// The same with M in DEVICE memory (nine doubles, e.g. &H[i].h[0] of
// findHomography below, produced earlier on the same stream): the overload is
// named, since a host and a device pointer have one type.  valid: an optional
// device int32 (&H[i].valid); where it reads 0 dst is left untouched.
inline void warpPerspectiveDeviceMatrix(Context& ctx, const GpuMatView& src, GpuMatView& dst, const double* deviceM,
                                        const int32_t* deviceValid = nullptr, int flags = TBDK_INTER_LINEAR,
                                        int borderMode = TBDK_BORDER_CONSTANT, const Scalar& borderValue = Scalar(),
                                        void* stream = nullptr)
{
    const int pix = detail::warp_pix(src, dst, "warpPerspective");
    check(tbdk_warp_perspective_dev(ctx.get(), src.data, pix, src.cn, src.width, src.height, src.pitch, dst.data,
                                    dst.width, dst.height, dst.pitch, deviceM, deviceValid, flags, borderMode,
                                    borderValue.val, stream),
          "tbdk_warp_perspective_dev");
}

// cv::findHomography(srcPoints, dstPoints, method, ransacReprojThreshold, mask,
// maxIters, confidence) (calib3d.hpp) on device point sets, batched as
// estimateRigidTransform above: set i is pairs [offsets[i], offsets[i + 1]) of
// src -> dst (device float2 arrays), status a device u8 mask or nullptr.  out
// (device, nsets entries) gets H row-major with valid = 0 and the identity where
// the reference returns an empty Mat; mask (device u8 per pair, or nullptr) the
// inliers.  method is 0 or RANSAC (8).  Nothing is copied to the host
// (tbdk_find_homography).
enum { LSQ = TBDK_HOMOGRAPHY_LSQ, RANSAC = TBDK_HOMOGRAPHY_RANSAC };
inline void findHomography(Context& ctx, const float* src, const float* dst, const uint8_t* status,
                           const int32_t* offsets, int nsets, tbdk_homography* out, int method = RANSAC,
                           double ransacReprojThreshold = 3.0, uint8_t* mask = nullptr, int maxIters = 2000,
                           double confidence = 0.995, bool refine = true, void* stream = nullptr)
{
    tbdk_homography_params p;
    check(tbdk_homography_default_params(&p), "tbdk_homography_default_params");
    p.method = method;
    p.reproj_threshold = ransacReprojThreshold;
    p.max_iters = maxIters;
    p.confidence = confidence;
    p.refine = refine ? 1 : 0;
    check(tbdk_find_homography(ctx.get(), src, dst, status, offsets, nsets, &p, out, mask, stream),
          "tbdk_find_homography");
}

// cv::estimateAffine2D(from, to, inliers, method, ransacReprojThreshold, maxIters,
// confidence, refineIters) (calib3d.hpp) on device point sets, batched and laid
// out as findHomography above.  out (device, nsets entries) gets the 2x3 matrix
// row-major, with valid = 0 and [1 0 0; 0 1 0] where the reference returns an
// empty Mat; inliers (device u8 per pair, or nullptr) the mask.  method is RANSAC
// (8) or LMEDS (4); the threshold is taken as given, as the reference takes it.
// Nothing is copied to the host (tbdk_estimate_affine_2d).
enum { LMEDS = TBDK_AFFINE2D_LMEDS };
namespace detail {
inline void estimate_affine(Context& ctx, int model, const float* from, const float* to, const uint8_t* status,
                            const int32_t* offsets, int nsets, tbdk_affine2d* out, uint8_t* inliers, int method,
                            double ransacReprojThreshold, int maxIters, double confidence, int refineIters,
                            void* stream)
{
    tbdk_affine2d_params p;
    check(tbdk_affine2d_default_params(&p), "tbdk_affine2d_default_params");
    p.model = model;
    p.method = method;
    p.reproj_threshold = ransacReprojThreshold;
    p.max_iters = maxIters;
    p.confidence = confidence;
    p.refine_iters = refineIters;
    check(tbdk_estimate_affine_2d(ctx.get(), from, to, status, offsets, nsets, &p, out, inliers, stream),
          "tbdk_estimate_affine_2d");
}
}  // namespace detail

inline void estimateAffine2D(Context& ctx, const float* from, const float* to, const uint8_t* status,
                             const int32_t* offsets, int nsets, tbdk_affine2d* out, uint8_t* inliers = nullptr,
                             int method = RANSAC, double ransacReprojThreshold = 3.0, int maxIters = 2000,
                             double confidence = 0.99, int refineIters = 10, void* stream = nullptr)
{
    detail::estimate_affine(ctx, TBDK_AFFINE2D_FULL, from, to, status, offsets, nsets, out, inliers, method,
                            ransacReprojThreshold, maxIters, confidence, refineIters, stream);
}

// cv::estimateAffinePartial2D: the same with the 4-DOF model (rotation, uniform scale, translation)
inline void estimateAffinePartial2D(Context& ctx, const float* from, const float* to, const uint8_t* status,
                                    const int32_t* offsets, int nsets, tbdk_affine2d* out, uint8_t* inliers = nullptr,
                                    int method = RANSAC, double ransacReprojThreshold = 3.0, int maxIters = 2000,
                                    double confidence = 0.99, int refineIters = 10, void* stream = nullptr)
{
    detail::estimate_affine(ctx, TBDK_AFFINE2D_PARTIAL, from, to, status, offsets, nsets, out, inliers, method,
                            ransacReprojThreshold, maxIters, confidence, refineIters, stream);
}

// warpAffine with M in DEVICE memory (six doubles, e.g. &A[i].m[0] of
// estimateAffine2D, produced earlier on the same stream).  valid: an optional
// device int32 (&A[i].valid); where it reads 0 dst is left untouched.
inline void warpAffineDeviceMatrix(Context& ctx, const GpuImage& src, GpuImage& dst, const double* deviceM,
                                   const int32_t* deviceValid = nullptr, int flags = TBDK_INTER_LINEAR,
                                   int borderMode = TBDK_BORDER_CONSTANT, int borderValue = 0, void* stream = nullptr)
{
    check(tbdk_warp_affine_u8_dev(ctx.get(), src.data, src.width, src.height, src.pitch, dst.data, dst.width,
                                  dst.height, dst.pitch, deviceM, deviceValid, flags, borderMode, borderValue, stream),
          "tbdk_warp_affine_u8_dev");
}

// cv::cornerSubPix(image, corners, winSize, zeroZone, criteria) (imgproc.hpp;
// imgproc/src/cornersubpix.cpp:44-156; the reference has no CUDA form) on the
// device, with the CPU function's bits: corners is device memory, nrows x rowCap
// float2 refined in place; counts (device, nrows int32, or nullptr: every row
// full) are CornersDetector::detectRois' counts, read on the device (no host
// sync).  A flat list of n points is nrows = 1, rowCap = n.  The defaults are
// samples/cpp/lkdemo.cpp:85's call.  The image is a one-channel 8U, 16U or 32F view.
inline void cornerSubPix(Context& ctx, const GpuMatView& image, float* corners, const int32_t* counts, int nrows,
                         int rowCap, Size win = Size{10, 10}, Size zeroZone = Size{-1, -1},
                         TermCriteria criteria = TermCriteria(), void* stream = nullptr)
{
    tbdk_subpix_params p{win.width, win.height, zeroZone.width, zeroZone.height, criteria.type, criteria.maxCount,
                         criteria.epsilon};
    check(tbdk_corner_sub_pix(ctx.get(), image.data, cuda::CornersDetector::pixOf(image, "cornerSubPix: image type"),
                              image.width, image.height, image.pitch, corners, counts, nrows, rowCap, &p, stream),
          "tbdk_corner_sub_pix");
}
// ... of a flat list of n points
inline void cornerSubPix(Context& ctx, const GpuMatView& image, float* corners, int n, Size win = Size{10, 10},
                         Size zeroZone = Size{-1, -1}, TermCriteria criteria = TermCriteria(), void* stream = nullptr)
{
    cornerSubPix(ctx, image, corners, nullptr, 1, n, win, zeroZone, criteria, stream);
}
// ... on a CV_8UC1 image
inline void cornerSubPix(Context& ctx, const GpuImage& image, float* corners, int n, Size win = Size{10, 10},
                         Size zeroZone = Size{-1, -1}, TermCriteria criteria = TermCriteria(), void* stream = nullptr)
{
    cornerSubPix(ctx, GpuMatView{image.data, image.width, image.height, image.pitch, DEPTH_8U, 1}, corners, nullptr, 1,
                 n, win, zeroZone, criteria, stream);
}

namespace cuda {

// cv::cuda::HOG (cudaobjdetect.hpp:75-180) with the CPU HOGDescriptor's results
// (objdetect/src/hog.cpp): create / setters / setSVMDetector / detectMultiScale.
// Detector coefficients stay on the host; getDefaultPeopleDetector's tables ship
// as opencv_amd/data/hog_people_{64x128,48x96}.f32 (loadDetector reads them).
class HOG {
public:
    static std::unique_ptr<HOG> create(Context& ctx, Size winSize = {64, 128}, Size blockSize = {16, 16},
                                       Size blockStride = {8, 8}, Size cellSize = {8, 8}, int nbins = 9)
    {
        std::unique_ptr<HOG> h(new HOG(ctx));
        tbdk_hog_default_params(&h->p_);
        h->p_.win_w = winSize.width, h->p_.win_h = winSize.height;
        h->p_.block_w = blockSize.width, h->p_.block_h = blockSize.height;
        h->p_.block_stride_x = blockStride.width, h->p_.block_stride_y = blockStride.height;
        h->p_.cell_w = cellSize.width, h->p_.cell_h = cellSize.height;
        h->p_.nbins = nbins;
        h->p_.win_stride_x = blockStride.width, h->p_.win_stride_y = blockStride.height;
        h->getDescriptorSize();  // throws on an invalid geometry (HOG_Impl's asserts)
        return h;
    }
    void setGammaCorrection(bool v) { p_.gamma_correction = v; }
    void setL2HysThreshold(double v) { p_.l2hys_threshold = v; }
    void setNumLevels(int v) { p_.nlevels = v; }
    int getNumLevels() const { return p_.nlevels; }
    void setHitThreshold(double v) { p_.hit_threshold = v; }
    double getHitThreshold() const { return p_.hit_threshold; }
    void setWinStride(Size s) { p_.win_stride_x = s.width, p_.win_stride_y = s.height; }
    void setScaleFactor(double v) { p_.scale0 = v; }
    double getScaleFactor() const { return p_.scale0; }
    void setGroupThreshold(int v) { p_.group_threshold = v; }
    int getGroupThreshold() const { return p_.group_threshold; }
    void setWinSigma(double v) { p_.win_sigma = v; }
    int getDescriptorSize() const
    {
        int n = 0;
        check(tbdk_hog_descriptor_size(&p_, &n), "HOG: invalid geometry");
        return n;
    }
    void setSVMDetector(const std::vector<float>& d)
    {
        const size_t n = (size_t)getDescriptorSize();
        if (d.size() != n && d.size() != n + 1) throw Error(TBDK_EINVAL, "HOG::setSVMDetector");
        svm_ = d;
    }
    // reads one of the shipped detector tables (little-endian float32)
    static std::vector<float> loadDetector(const char* path)
    {
        std::vector<float> v;
        if (FILE* f = std::fopen(path, "rb")) {
            float x;
            while (std::fread(&x, 4, 1, f) == 1) v.push_back(x);
            std::fclose(f);
        }
        if (v.empty()) throw Error(TBDK_EINVAL, "HOG::loadDetector");
        return v;
    }
    // img: device u8, 1 (gray), 3 (BGR) or 4 (BGRA) channels; returns (x, y, w, h) rects
    std::vector<tbdk_roi> detectMultiScale(const GpuImage& img, int channels, std::vector<double>* confidences = nullptr,
                                           void* stream = nullptr)
    {
        std::vector<int32_t> r;
        std::vector<double> w;
        int n = 0;
        for (int cap = 4096;; cap *= 4) {  // grow and call again while the results overflow
            r.resize(4 * (size_t)cap);
            w.resize(cap);
            const int rc = tbdk_hog_detect_multiscale(ctx_->get(), img.data, img.width, img.height, img.pitch,
                                                      channels, &p_, svm_.data(), (int)svm_.size(), r.data(),
                                                      w.data(), cap, &n, stream);
            if (rc == TBDK_ENOMEM && n == cap) continue;
            check(rc, "tbdk_hog_detect_multiscale");
            break;
        }
        std::vector<tbdk_roi> out(n);
        for (int i = 0; i < n; ++i) out[i] = tbdk_roi{r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
        if (confidences) confidences->assign(w.begin(), w.begin() + n);
        return out;
    }
    const tbdk_hog_params& params() const { return p_; }
    const std::vector<float>& detector() const { return svm_; }

private:
    explicit HOG(Context& ctx) : ctx_(&ctx) {}
    Context* ctx_;
    tbdk_hog_params p_{};
    std::vector<float> svm_;
};

}  // namespace cuda


// The tracking section of samples/gpu/tbd.cpp:624-706 (cv::tbd::Tracker +
// KLT box propagation) for one video stream.
class TbdLoop {
public:
    TbdLoop(Context& ctx, const tbdk_tbd_config& cfg) { check(tbdk_tbd_create(ctx.get(), &cfg, &h_), "tbdk_tbd_create"); }
    ~TbdLoop() { tbdk_tbd_destroy(h_); }
    TbdLoop(const TbdLoop&) = delete;
    TbdLoop& operator=(const TbdLoop&) = delete;
    static tbdk_tbd_config defaultConfig(int width, int height)
    {
        tbdk_tbd_config c;
        check(tbdk_tbd_default_config(width, height, &c), "tbdk_tbd_default_config");
        return c;
    }
    tbdk_frame_metrics step(const GpuImage& frame, int frameId, const std::vector<tbdk_detection>& dets,
                            void* stream = nullptr)
    {
        tbdk_frame_metrics m;
        check(tbdk_tbd_step(h_, frame.data, frame.pitch, frameId, dets.data(), (int)dets.size(), &m, stream),
              "tbdk_tbd_step");
        return m;
    }
    std::vector<tbdk_track_info> tracks() const
    {
        std::vector<tbdk_track_info> out(4096);
        int n = 0;
        check(tbdk_tbd_tracks(h_, out.data(), (int)out.size(), &n), "tbdk_tbd_tracks");
        out.resize((size_t)(n < (int)out.size() ? n : (int)out.size()));
        return out;
    }
    tbdk_tbd* get() const { return h_; }

private:
    tbdk_tbd* h_ = nullptr;
};

// The loop of the reference's KLT samples (samples/python/lk_track.py App.run:48-86,
// samples/cpp/lkdemo.cpp's cornerSubPix and click-to-add) as one device-resident
// object (tbdk_klt_tracker): step() tracks every live point with the
// forward-backward check, drops the lost ones (both statuses gate, unlike
// lk_track.py:57-60) and, every detect_interval frames, detects new corners away
// from the live ones.  A step only enqueues work; read() synchronises.
class KltTracker {
public:
    // the live tracks in order: hist holds trackLen float2 per track, oldest first, zero beyond lens[i]
    struct State {
        std::vector<int32_t> ids, lens;
        std::vector<float> lastPts, hist;
        tbdk_klt_tracker_stats stats;
        int trackLen = 0;
        size_t size() const { return ids.size(); }
    };
    KltTracker(Context& ctx, const tbdk_klt_tracker_config& cfg) : track_len_(cfg.track_len)
    {
        check(tbdk_klt_tracker_create(ctx.get(), &cfg, &h_), "tbdk_klt_tracker_create");
    }
    ~KltTracker() { tbdk_klt_tracker_destroy(h_); }
    KltTracker(const KltTracker&) = delete;
    KltTracker& operator=(const KltTracker&) = delete;
    static tbdk_klt_tracker_config defaultConfig(int width, int height)
    {
        tbdk_klt_tracker_config c;
        check(tbdk_klt_tracker_default_config(width, height, &c), "tbdk_klt_tracker_default_config");
        return c;
    }
    void step(const GpuImage& frame, bool detectNow = false, void* stream = nullptr)
    {
        check(tbdk_klt_tracker_step(h_, frame.data, frame.pitch, detectNow ? TBDK_KLT_DETECT_NOW : 0, stream),
              "tbdk_klt_tracker_step");
    }
    // n device points (float2) become new tracks (lkdemo's click-to-add)
    void addPoints(const float* devicePts, int n, void* stream = nullptr)
    {
        check(tbdk_klt_tracker_add_points(h_, devicePts, n, stream), "tbdk_klt_tracker_add_points");
    }
    void reset() { check(tbdk_klt_tracker_reset(h_), "tbdk_klt_tracker_reset"); }
    State read()
    {
        State s;
        int n = 0;
        check(tbdk_klt_tracker_read(h_, nullptr, nullptr, nullptr, nullptr, 0, &n, &s.stats), "tbdk_klt_tracker_read");
        const size_t k = n > 0 ? (size_t)n : 0;
        s.trackLen = track_len_;
        s.ids.resize(k);
        s.lens.resize(k);
        s.lastPts.resize(2 * k);
        s.hist.resize(2 * k * (size_t)track_len_);
        if (k)
            check(tbdk_klt_tracker_read(h_, s.ids.data(), s.lastPts.data(), s.lens.data(), s.hist.data(), (int)k, &n,
                                        &s.stats),
                  "tbdk_klt_tracker_read");
        return s;
    }
    tbdk_klt_tracker* get() const { return h_; }

private:
    tbdk_klt_tracker* h_ = nullptr;
    int track_len_ = 0;
};

// cv::BackgroundSubtractorMOG2 / cv::cuda::BackgroundSubtractorMOG2 (video/background_segm.hpp:90-219,
// cudabgsegm.hpp) over tbdk_mog2: the model stays on the device, apply() only enqueues work.  The model is
// allocated by the first apply, from the frame's size and type, which may not change afterwards; so may
// nmixtures not.  Masks, background images and the model are the CPU reference's bit for bit.
class BackgroundSubtractorMOG2 {
public:
    BackgroundSubtractorMOG2(Context& ctx, int history = 500, double varThreshold = 16, bool detectShadows = true)
        : ctx_(&ctx)
    {
        check(tbdk_mog2_config_default(0, 0, DEPTH_8U, 1, &cfg_), "tbdk_mog2_config_default");
        // the reference's constructor keeps its defaults for non-positive arguments (bgfg_gaussmix2.cpp:157-158)
        if (history > 0) cfg_.history = history;
        if (varThreshold > 0) cfg_.var_threshold = varThreshold;
        cfg_.detect_shadows = detectShadows ? 1 : 0;
    }
    ~BackgroundSubtractorMOG2()
    {
        if (h_) tbdk_mog2_destroy(h_);
    }
    BackgroundSubtractorMOG2(const BackgroundSubtractorMOG2&) = delete;
    BackgroundSubtractorMOG2& operator=(const BackgroundSubtractorMOG2&) = delete;

    // image: 8U or 32F, 1 or 3 channels; fgmask: 8-bit, the image's size
    void apply(const GpuMatView& image, const GpuImage& fgmask, double learningRate = -1, void* stream = nullptr)
    {
        if (!h_) {
            cfg_.width = image.width, cfg_.height = image.height, cfg_.depth = image.depth, cfg_.channels = image.cn;
            check(tbdk_mog2_create(ctx_->get(), &cfg_, &h_), "tbdk_mog2_create");
        }
        if (image.width != cfg_.width || image.height != cfg_.height || image.depth != cfg_.depth ||
            image.cn != cfg_.channels || fgmask.width != cfg_.width || fgmask.height != cfg_.height)
            throw Error(TBDK_EINVAL, "BackgroundSubtractorMOG2::apply: the frame's size and type may not change");
        check(tbdk_mog2_apply(h_, image.data, image.pitch, fgmask.data, fgmask.pitch, learningRate, stream),
              "tbdk_mog2_apply");
    }
    void getBackgroundImage(const GpuMatView& backgroundImage, void* stream = nullptr)
    {
        if (!h_ || backgroundImage.width != cfg_.width || backgroundImage.height != cfg_.height ||
            backgroundImage.depth != cfg_.depth || backgroundImage.cn != cfg_.channels)
            throw Error(TBDK_EINVAL, "BackgroundSubtractorMOG2::getBackgroundImage: an image of the frames' size and type");
        check(tbdk_mog2_get_background(h_, backgroundImage.data, backgroundImage.pitch, stream),
              "tbdk_mog2_get_background");
    }
    void reset()
    {
        if (h_) check(tbdk_mog2_reset(h_), "tbdk_mog2_reset");
    }
    int frames() const
    {
        int n = 0;
        if (h_) check(tbdk_mog2_frames(h_, &n), "tbdk_mog2_frames");
        return n;
    }

    int getHistory() const { return cfg_.history; }
    void setHistory(int v) { set(&tbdk_mog2_config::history, v); }
    int getNMixtures() const { return cfg_.nmixtures; }
    void setNMixtures(int v)  // before the first apply only
    {
        if (h_ && v != cfg_.nmixtures) throw Error(TBDK_EINVAL, "BackgroundSubtractorMOG2::setNMixtures: model allocated");
        cfg_.nmixtures = v;
    }
    double getBackgroundRatio() const { return cfg_.background_ratio; }
    void setBackgroundRatio(double v) { set(&tbdk_mog2_config::background_ratio, (float)v); }
    double getVarThreshold() const { return cfg_.var_threshold; }
    void setVarThreshold(double v) { set(&tbdk_mog2_config::var_threshold, v); }
    double getVarThresholdGen() const { return cfg_.var_threshold_gen; }
    void setVarThresholdGen(double v) { set(&tbdk_mog2_config::var_threshold_gen, (float)v); }
    double getVarInit() const { return cfg_.var_init; }
    void setVarInit(double v) { set(&tbdk_mog2_config::var_init, (float)v); }
    double getVarMin() const { return cfg_.var_min; }
    void setVarMin(double v) { set(&tbdk_mog2_config::var_min, (float)v); }
    double getVarMax() const { return cfg_.var_max; }
    void setVarMax(double v) { set(&tbdk_mog2_config::var_max, (float)v); }
    double getComplexityReductionThreshold() const { return cfg_.complexity_reduction; }
    void setComplexityReductionThreshold(double v) { set(&tbdk_mog2_config::complexity_reduction, (float)v); }
    bool getDetectShadows() const { return cfg_.detect_shadows != 0; }
    void setDetectShadows(bool v) { set(&tbdk_mog2_config::detect_shadows, (int32_t)(v ? 1 : 0)); }
    int getShadowValue() const { return cfg_.shadow_value; }
    void setShadowValue(int v) { set(&tbdk_mog2_config::shadow_value, (int32_t)(v & 255)); }  // narrowed to uchar
    double getShadowThreshold() const { return cfg_.shadow_threshold; }
    void setShadowThreshold(double v) { set(&tbdk_mog2_config::shadow_threshold, (float)v); }
    tbdk_mog2* get() const { return h_; }

private:
    template <typename T>
    void set(T tbdk_mog2_config::*field, T v)
    {
        const T old = cfg_.*field;
        cfg_.*field = v;
        if (!h_) return;
        const int rc = tbdk_mog2_set_params(h_, &cfg_);
        if (rc != TBDK_OK) {
            cfg_.*field = old;
            throw Error(rc, "tbdk_mog2_set_params");
        }
    }
    Context* ctx_;
    tbdk_mog2_config cfg_{};
    tbdk_mog2* h_ = nullptr;
};

// cv::createBackgroundSubtractorMOG2(history, varThreshold, detectShadows)
inline std::unique_ptr<BackgroundSubtractorMOG2> createBackgroundSubtractorMOG2(Context& ctx, int history = 500,
                                                                                double varThreshold = 16,
                                                                                bool detectShadows = true)
{
    return std::unique_ptr<BackgroundSubtractorMOG2>(new BackgroundSubtractorMOG2(ctx, history, varThreshold, detectShadows));
}

// cv::BackgroundSubtractorKNN, the CPU class (video/background_segm.hpp:222-300, video/src/bgfg_KNN.cpp), over
// tbdk_knn: the model and the RNG stay on the device, apply() only enqueues work.  The model is allocated by the
// first apply, from the frame's size and channels (8-bit, 1 or 3), which may not change afterwards; so may
// nSamples not.  rngState is cv::theRNG().state of the thread that would run the reference.  Masks, background
// images, model, counters and RNG state are the CPU reference's bit for bit.
class BackgroundSubtractorKNN {
public:
    BackgroundSubtractorKNN(Context& ctx, int history = 500, double dist2Threshold = 400.0, bool detectShadows = true,
                            uint64_t rngState = 0xffffffffull)
        : ctx_(&ctx)
    {
        check(tbdk_knn_config_default(0, 0, 1, &cfg_), "tbdk_knn_config_default");
        // the reference's constructor keeps its defaults for non-positive arguments (bgfg_KNN.cpp:108,117)
        if (history > 0) cfg_.history = history;
        if (dist2Threshold > 0) cfg_.dist2_threshold = (float)dist2Threshold;
        cfg_.detect_shadows = detectShadows ? 1 : 0;
        cfg_.rng_state = rngState;
    }
    ~BackgroundSubtractorKNN()
    {
        if (h_) tbdk_knn_destroy(h_);
    }
    BackgroundSubtractorKNN(const BackgroundSubtractorKNN&) = delete;
    BackgroundSubtractorKNN& operator=(const BackgroundSubtractorKNN&) = delete;

    // image: 8U, 1 or 3 channels; fgmask: 8-bit, the image's size
    void apply(const GpuMatView& image, const GpuImage& fgmask, double learningRate = -1, void* stream = nullptr)
    {
        if (image.depth != DEPTH_8U) throw Error(TBDK_EINVAL, "BackgroundSubtractorKNN::apply: 8-bit frames only");
        if (!h_) {
            cfg_.width = image.width, cfg_.height = image.height, cfg_.channels = image.cn;
            check(tbdk_knn_create(ctx_->get(), &cfg_, &h_), "tbdk_knn_create");
        }
        if (image.width != cfg_.width || image.height != cfg_.height || image.cn != cfg_.channels ||
            fgmask.width != cfg_.width || fgmask.height != cfg_.height)
            throw Error(TBDK_EINVAL, "BackgroundSubtractorKNN::apply: the frame's size and type may not change");
        check(tbdk_knn_apply(h_, static_cast<const uint8_t*>(image.data), image.pitch, fgmask.data, fgmask.pitch,
                             learningRate, stream),
              "tbdk_knn_apply");
    }
    void getBackgroundImage(const GpuMatView& backgroundImage, void* stream = nullptr)
    {
        if (!h_ || backgroundImage.width != cfg_.width || backgroundImage.height != cfg_.height ||
            backgroundImage.depth != DEPTH_8U || backgroundImage.cn != cfg_.channels)
            throw Error(TBDK_EINVAL, "BackgroundSubtractorKNN::getBackgroundImage: an image of the frames' size and type");
        check(tbdk_knn_get_background(h_, static_cast<uint8_t*>(backgroundImage.data), backgroundImage.pitch, stream),
              "tbdk_knn_get_background");
    }
    void reset()
    {
        if (h_) check(tbdk_knn_reset(h_), "tbdk_knn_reset");
    }
    int frames() const
    {
        int n = 0;
        if (h_) check(tbdk_knn_frames(h_, &n), "tbdk_knn_frames");
        return n;
    }

    int getHistory() const { return cfg_.history; }
    void setHistory(int v) { set(&tbdk_knn_config::history, (int32_t)v); }
    int getNSamples() const { return cfg_.nsamples; }
    void setNSamples(int v)  // before the first apply only
    {
        if (h_ && v != cfg_.nsamples) throw Error(TBDK_EINVAL, "BackgroundSubtractorKNN::setNSamples: model allocated");
        cfg_.nsamples = v;
    }
    double getDist2Threshold() const { return cfg_.dist2_threshold; }
    void setDist2Threshold(double v) { set(&tbdk_knn_config::dist2_threshold, (float)v); }
    int getkNNSamples() const { return cfg_.knn_samples; }
    void setkNNSamples(int v) { set(&tbdk_knn_config::knn_samples, (int32_t)v); }
    bool getDetectShadows() const { return cfg_.detect_shadows != 0; }
    void setDetectShadows(bool v) { set(&tbdk_knn_config::detect_shadows, (int32_t)(v ? 1 : 0)); }
    int getShadowValue() const { return cfg_.shadow_value; }
    void setShadowValue(int v) { set(&tbdk_knn_config::shadow_value, (int32_t)(v & 255)); }  // narrowed to uchar
    double getShadowThreshold() const { return cfg_.shadow_threshold; }
    void setShadowThreshold(double v) { set(&tbdk_knn_config::shadow_threshold, (float)v); }
    tbdk_knn* get() const { return h_; }

private:
    template <typename T>
    void set(T tbdk_knn_config::*field, T v)
    {
        const T old = cfg_.*field;
        cfg_.*field = v;
        if (!h_) return;
        const int rc = tbdk_knn_set_params(h_, &cfg_);
        if (rc != TBDK_OK) {
            cfg_.*field = old;
            throw Error(rc, "tbdk_knn_set_params");
        }
    }
    Context* ctx_;
    tbdk_knn_config cfg_{};
    tbdk_knn* h_ = nullptr;
};

// cv::createBackgroundSubtractorKNN(history, dist2Threshold, detectShadows)
inline std::unique_ptr<BackgroundSubtractorKNN> createBackgroundSubtractorKNN(Context& ctx, int history = 500,
                                                                              double dist2Threshold = 400.0,
                                                                              bool detectShadows = true,
                                                                              uint64_t rngState = 0xffffffffull)
{
    return std::unique_ptr<BackgroundSubtractorKNN>(
        new BackgroundSubtractorKNN(ctx, history, dist2Threshold, detectShadows, rngState));
}

// ---- morphology and connected components (imgproc/src/morph.dispatch.cpp, connectedcomponents.cpp) over
// tbdk_morph_u8 / tbdk_connected_components: 8-bit one-channel device images in, everything out stays on the
// device, nothing synchronises.  Results are the CPU reference's bit for bit, label numbering included.
enum MorphTypes { MORPH_ERODE = 0, MORPH_DILATE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3 };
enum MorphShapes { MORPH_RECT = 0, MORPH_CROSS = 1, MORPH_ELLIPSE = 2 };
enum ConnectedComponentsAlgorithmsTypes { CCL_WU = 0, CCL_DEFAULT = -1, CCL_GRANA = 1 };
enum ConnectedComponentsTypes { CC_STAT_LEFT = 0, CC_STAT_TOP = 1, CC_STAT_WIDTH = 2, CC_STAT_HEIGHT = 3, CC_STAT_AREA = 4 };
constexpr int MORPH_DEFAULT_BORDER_VALUE = -1;  // cv::morphologyDefaultBorderValue()

struct Point {
    int x = -1, y = -1;
};

// A host structuring element (a cv::Mat of CV_8U): rows first, non-zero = in.  Empty: the reference's empty
// Mat, the 3 x 3 rectangle.
struct StructuringElement {
    int width = 0, height = 0;
    std::vector<uint8_t> data;
    bool empty() const { return data.empty(); }
};

// cv::getStructuringElement(shape, ksize, anchor)
inline StructuringElement getStructuringElement(int shape, Size ksize, Point anchor = Point())
{
    StructuringElement e;
    if (ksize.width < 1 || ksize.height < 1) throw Error(TBDK_EINVAL, "getStructuringElement");
    e.width = ksize.width, e.height = ksize.height;
    e.data.resize((size_t)ksize.width * ksize.height);
    check(tbdk_structuring_element(shape, ksize.width, ksize.height, anchor.x, anchor.y, e.data.data()),
          "tbdk_structuring_element");
    return e;
}

// cv::morphologyEx(src, dst, op, kernel, anchor, iterations, borderType, borderValue), MORPH_ERODE / DILATE /
// OPEN / CLOSE; dst may be src.  borderValue: MORPH_DEFAULT_BORDER_VALUE or 0..255
inline void morphologyEx(Context& ctx, const GpuImage& src, const GpuImage& dst, int op, const StructuringElement& kernel,
                         Point anchor = Point(), int iterations = 1, int borderType = TBDK_BORDER_CONSTANT,
                         int borderValue = MORPH_DEFAULT_BORDER_VALUE, void* stream = nullptr)
{
    if (src.width != dst.width || src.height != dst.height) throw Error(TBDK_EINVAL, "morphologyEx: dst must have src's size");
    check(tbdk_morph_u8(ctx.get(), op, src.data, src.width, src.height, src.pitch, dst.data, dst.pitch,
                        kernel.empty() ? nullptr : kernel.data.data(), kernel.width, kernel.height, anchor.x, anchor.y,
                        iterations, borderType, borderValue, stream),
          "tbdk_morph_u8");
}
// cv::erode / cv::dilate
inline void erode(Context& ctx, const GpuImage& src, const GpuImage& dst, const StructuringElement& kernel,
                  Point anchor = Point(), int iterations = 1, int borderType = TBDK_BORDER_CONSTANT,
                  int borderValue = MORPH_DEFAULT_BORDER_VALUE, void* stream = nullptr)
{
    morphologyEx(ctx, src, dst, MORPH_ERODE, kernel, anchor, iterations, borderType, borderValue, stream);
}
inline void dilate(Context& ctx, const GpuImage& src, const GpuImage& dst, const StructuringElement& kernel,
                   Point anchor = Point(), int iterations = 1, int borderType = TBDK_BORDER_CONSTANT,
                   int borderValue = MORPH_DEFAULT_BORDER_VALUE, void* stream = nullptr)
{
    morphologyEx(ctx, src, dst, MORPH_DILATE, kernel, anchor, iterations, borderType, borderValue, stream);
}

// The CV_32S label image of connectedComponents: device int32, pitch in bytes (a multiple of 4)
struct GpuLabels {
    int32_t* data = nullptr;
    int width = 0, height = 0, pitch = 0;
};

// cv::connectedComponents(image, labels, connectivity, CV_32S, ccltype): nLabels (device int32) gets the
// return value N, with no host synchronisation
inline void connectedComponents(Context& ctx, const GpuImage& image, const GpuLabels& labels, int32_t* nLabels,
                                int connectivity = 8, int ccltype = CCL_DEFAULT, void* stream = nullptr)
{
    if (image.width != labels.width || image.height != labels.height)
        throw Error(TBDK_EINVAL, "connectedComponents: labels must have the image's size");
    check(tbdk_connected_components(ctx.get(), image.data, image.width, image.height, image.pitch, labels.data,
                                    labels.pitch, connectivity, ccltype, nullptr, nullptr, 0, nLabels, stream),
          "tbdk_connected_components");
}
// cv::connectedComponentsWithStats: stats (device int32 [maxLabels][5], CC_STAT_*) and centroids (device double
// [maxLabels][2]) get the rows below min(N, maxLabels), row 0 the background's; the rest stays as it was
inline void connectedComponentsWithStats(Context& ctx, const GpuImage& image, const GpuLabels& labels, int32_t* stats,
                                         double* centroids, int maxLabels, int32_t* nLabels, int connectivity = 8,
                                         int ccltype = CCL_DEFAULT, void* stream = nullptr)
{
    if (image.width != labels.width || image.height != labels.height)
        throw Error(TBDK_EINVAL, "connectedComponentsWithStats: labels must have the image's size");
    check(tbdk_connected_components(ctx.get(), image.data, image.width, image.height, image.pitch, labels.data,
                                    labels.pitch, connectivity, ccltype, stats, centroids, maxLabels, nLabels, stream),
          "tbdk_connected_components");
}

// ---- GaussianBlur on 8-bit images and threshold (imgproc/src/smooth.dispatch.cpp, smooth.simd.hpp, thresh.cpp)
// over tbdk_gaussian_blur_u8 / tbdk_threshold.  Results are the CPU reference's bit for bit; nothing synchronises.
enum ThresholdTypes {
    THRESH_BINARY = 0, THRESH_BINARY_INV = 1, THRESH_TRUNC = 2, THRESH_TOZERO = 3, THRESH_TOZERO_INV = 4, THRESH_OTSU = 8
};

// the threshold stage GaussianBlur can fuse in: cv::threshold(blurred, dst, thresh, maxval, type), a plain type
struct FusedThreshold {
    double thresh = 0, maxval = 255;
    int type = THRESH_BINARY;
};

// getFixedpointGaussianKernel<ufixedpoint16>(n, sigma): the 8.8 coefficients the 8-bit blur uses
inline std::vector<uint16_t> getGaussianKernelU8(int n, double sigma)
{
    if (n < 1) throw Error(TBDK_EINVAL, "getGaussianKernelU8");
    std::vector<uint16_t> k((size_t)n);
    check(tbdk_gaussian_kernel_u8(n, sigma, k.data()), "tbdk_gaussian_kernel_u8");
    return k;
}

// cv::GaussianBlur(src, dst, ksize, sigmaX, sigmaY, borderType | BORDER_ISOLATED) on CV_8UC1 / 8UC3 / 8UC4 views;
// dst may be src.  fused: applied to every output byte in the same launch
inline void GaussianBlur(Context& ctx, const GpuMatView& src, const GpuMatView& dst, Size ksize, double sigmaX,
                         double sigmaY = 0, int borderType = TBDK_BORDER_REFLECT_101, void* stream = nullptr,
                         const FusedThreshold* fused = nullptr)
{
    if (src.depth != DEPTH_8U || dst.depth != DEPTH_8U || src.width != dst.width || src.height != dst.height ||
        src.cn != dst.cn)
        throw Error(TBDK_EINVAL, "GaussianBlur: 8-bit views of one size and channel count expected");
    tbdk_thresh_params t{0, 0, 0, 0};
    if (fused) t = tbdk_thresh_params{fused->thresh, fused->maxval, fused->type, 0};
    check(tbdk_gaussian_blur_u8(ctx.get(), static_cast<const uint8_t*>(src.data), src.width, src.height, src.cn,
                                src.pitch, static_cast<uint8_t*>(dst.data), dst.pitch, ksize.width, ksize.height, sigmaX,
                                sigmaY, borderType, fused ? &t : nullptr, stream),
          "tbdk_gaussian_blur_u8");
}
inline void GaussianBlur(Context& ctx, const GpuImage& src, const GpuImage& dst, Size ksize, double sigmaX,
                         double sigmaY = 0, int borderType = TBDK_BORDER_REFLECT_101, void* stream = nullptr,
                         const FusedThreshold* fused = nullptr)
{
    GaussianBlur(ctx, GpuMatView{src.data, src.width, src.height, src.pitch, DEPTH_8U, 1},
                 GpuMatView{dst.data, dst.width, dst.height, dst.pitch, DEPTH_8U, 1}, ksize, sigmaX, sigmaY, borderType,
                 stream, fused);
}

// cv::threshold(src, dst, thresh, maxval, type) on 8-bit views of any channel count and CV_32F views; returns
// what the reference returns.  With THRESH_OTSU (CV_8UC1) the value exists only on the device: otsu (a device
// int32) receives it in stream order and the return value is NaN
inline double threshold(Context& ctx, const GpuMatView& src, const GpuMatView& dst, double thresh, double maxval,
                        int type, void* stream = nullptr, int32_t* otsu = nullptr)
{
    if (src.depth != dst.depth || (src.depth != DEPTH_8U && src.depth != DEPTH_32F) || src.width != dst.width ||
        src.height != dst.height || src.cn != dst.cn)
        throw Error(TBDK_EINVAL, "threshold: 8-bit or 32F views of one size and channel count expected");
    double used = 0;
    check(tbdk_threshold(ctx.get(), src.data, src.depth == DEPTH_8U ? TBDK_PIX_U8 : TBDK_PIX_F32, src.width, src.height,
                         src.cn, src.pitch, dst.data, dst.pitch, thresh, maxval, type, &used, otsu, stream),
          "tbdk_threshold");
    return used;
}

// The sample's whole per-frame path (samples/gpu/tbd.cpp:568-622) on a TbdLoop:
// colour frame -> cvtColor -> optional resize -> HOG detectMultiScale -> the
// loop (tbdk_tbd_step_image).  `loop` and `ctx` must outlive it.
class DetectingTbd {
public:
    // cfg: tbdk_tbd_detect_default_config(loop width, loop height) with the
    // source size / channels / confidence mode set; its HOG settings and the
    // detector coefficients are taken from `hog`
    DetectingTbd(Context& ctx, TbdLoop& loop, const cuda::HOG& hog, tbdk_tbd_detect_config cfg)
    {
        cfg.hog = hog.params();
        check(tbdk_tbd_detector_create(ctx.get(), loop.get(), &cfg, hog.detector().data(), (int)hog.detector().size(),
                                       &h_),
              "tbdk_tbd_detector_create");
    }
    ~DetectingTbd() { tbdk_tbd_detector_destroy(h_); }
    DetectingTbd(const DetectingTbd&) = delete;
    DetectingTbd& operator=(const DetectingTbd&) = delete;
    static tbdk_tbd_detect_config defaultConfig(int width, int height)
    {
        tbdk_tbd_detect_config c;
        check(tbdk_tbd_detect_default_config(width, height, &c), "tbdk_tbd_detect_default_config");
        return c;
    }
    // frame: the colour frame (cfg.src_width x src_height x src_cn); detections (optional): the ones used
    tbdk_frame_metrics step(const GpuMatView& frame, int frameId, std::vector<tbdk_detection>* detections = nullptr,
                            void* stream = nullptr)
    {
        tbdk_frame_metrics m;
        int n = 0;
        if (frame.depth != DEPTH_8U) throw Error(TBDK_EINVAL, "DetectingTbd::step");
        dets_.resize(dets_.empty() ? 4096 : dets_.size());
        check(tbdk_tbd_step_image(h_, static_cast<const uint8_t*>(frame.data), frame.pitch, frameId, dets_.data(),
                                  (int)dets_.size(), &n, &m, stream),
              "tbdk_tbd_step_image");
        if (detections) detections->assign(dets_.begin(), dets_.begin() + (n < (int)dets_.size() ? n : (int)dets_.size()));
        return m;
    }

private:
    tbdk_tbd_detector* h_ = nullptr;
    std::vector<tbdk_detection> dets_;
};

}  // namespace tbdk

#endif  // TBDK_HPP
