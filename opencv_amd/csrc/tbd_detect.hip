// tbd_detect.hip — the detection-driven TBD step: a colour frame in, HOG
// detections, tracks out.  The per-frame path of samples/gpu/tbd.cpp:568-622
// in front of the loop: cvtColor -> optional resize (frontend.hip) ->
// HOG detectMultiScale (hog.hip) -> one Detection per rect -> tbdk_tbd_step
// (tbd_loop.hip, untouched), and the sample's loop over an image sequence
// (binary PNM files, pnm_reader.hpp) without a bbox file.
#include <cstring>
#include <fstream>
#include <new>
#include <string>

#include "pnm_reader.hpp"
#include "tbdk_internal.hpp"

using namespace tbdk;

struct tbdk_tbd_detector {
    tbdk_ctx* ctx = nullptr;
    tbdk_tbd* tbd = nullptr;
    tbdk_tbd_detect_config cfg;
    std::vector<float> svm;
    uint8_t* gray = nullptr;   // the loop's frame (width x height)
    int gray_pitch = 0;
    uint8_t* color = nullptr;  // make_gray = 0 with resize: the resized colour frame HOG reads
    int color_pitch = 0;
    std::vector<int32_t> rects;
    std::vector<double> weights;
    std::vector<tbdk_detection> dets;
};

namespace {

int gray_code_of(int cn, int rgb)
{
    return cn == 3 ? (rgb ? TBDK_COLOR_RGB2GRAY : TBDK_COLOR_BGR2GRAY) : (rgb ? TBDK_COLOR_RGBA2GRAY : TBDK_COLOR_BGRA2GRAY);
}

}  // namespace

extern "C" {

int tbdk_tbd_detect_default_config(int width, int height, tbdk_tbd_detect_config* cfg)
{
    if (!cfg || width <= 0 || height <= 0) return TBDK_EINVAL;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->width = cfg->src_width = width;
    cfg->height = cfg->src_height = height;
    cfg->src_cn = 3;
    cfg->make_gray = 1;
    cfg->max_detections = 4096;
    tbdk_hog_default_params(&cfg->hog);
    cfg->hog.nlevels = 15;           // samples/gpu/tbd.cpp:437-438
    cfg->hog.hit_threshold = 0.45;   // :441
    return TBDK_OK;
}

int tbdk_tbd_detector_create(tbdk_ctx* ctx, tbdk_tbd* tbd, const tbdk_tbd_detect_config* cfg, const float* svm,
                             int svm_len, tbdk_tbd_detector** out)
{
    if (!out) return TBDK_EINVAL;
    *out = nullptr;
    if (!ctx || !tbd || !cfg || !svm) return TBDK_EINVAL;
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->src_width <= 0 || cfg->src_height <= 0 ||
        (cfg->src_cn != 1 && cfg->src_cn != 3 && cfg->src_cn != 4) || cfg->max_detections <= 0 ||
        (cfg->confidence_mode != 0 && cfg->confidence_mode != 1))
        return TBDK_EINVAL;
    if (!cfg->resize && (cfg->src_width != cfg->width || cfg->src_height != cfg->height)) return TBDK_EINVAL;
    int dsize = 0;
    if (tbdk_hog_descriptor_size(&cfg->hog, &dsize) != TBDK_OK) return TBDK_EINVAL;
    if (svm_len != dsize && svm_len != dsize + 1) return TBDK_EINVAL;
    tbdk_tbd_detector* d = new (std::nothrow) tbdk_tbd_detector();
    if (!d) return TBDK_ENOMEM;
    d->ctx = ctx, d->tbd = tbd, d->cfg = *cfg;
    d->svm.assign(svm, svm + svm_len);
    d->rects.resize(4 * (size_t)cfg->max_detections);
    d->weights.resize((size_t)cfg->max_detections);
    DeviceGuard g(ctx->device);
    const bool resized = cfg->src_width != cfg->width || cfg->src_height != cfg->height;
    hipError_t e = hipSuccess;
    if (cfg->src_cn != 1 || resized) {  // gray frames of the loop's size are used in place
        d->gray_pitch = align_up(cfg->width, 64);
        e = dev_alloc(&d->gray, (size_t)d->gray_pitch * cfg->height, ctx->opt_alloc_fill);
    }
    if (e == hipSuccess && cfg->src_cn != 1 && !cfg->make_gray && resized) {
        d->color_pitch = align_up(cfg->width * cfg->src_cn, 64);
        e = dev_alloc(&d->color, (size_t)d->color_pitch * cfg->height, ctx->opt_alloc_fill);
    }
    if (e != hipSuccess) {
        (void)tbdk_tbd_detector_destroy(d);
        return TBDK_ENOMEM;
    }
    *out = d;
    return TBDK_OK;
}

int tbdk_tbd_detector_destroy(tbdk_tbd_detector* d)
{
    if (!d) return TBDK_EINVAL;
    DeviceGuard g(d->ctx->device);
    if (d->gray) (void)hipFree(d->gray);
    if (d->color) (void)hipFree(d->color);
    delete d;
    return TBDK_OK;
}

int tbdk_tbd_step_image(tbdk_tbd_detector* d, const uint8_t* frame, int pitch, int frame_id, tbdk_detection* dets_out,
                        int cap, int* ndets, tbdk_frame_metrics* metrics, void* stream)
{
    if (ndets) *ndets = 0;
    if (!d || !frame || cap < 0 || (cap > 0 && !dets_out)) return TBDK_EINVAL;
    const tbdk_tbd_detect_config& c = d->cfg;
    if (pitch < (int64_t)c.src_width * c.src_cn) return TBDK_EINVAL;
    DeviceGuard g(d->ctx->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int W = c.width, H = c.height;
    const bool resized = c.src_width != W || c.src_height != H;
    // 1. the front end (samples/gpu/tbd.cpp:573-578)
    const uint8_t* hog_img = d->gray;
    int hog_pitch = d->gray_pitch, hog_cn = 1;
    const uint8_t* klt = d->gray;
    int klt_pitch = d->gray_pitch;
    int rc = TBDK_OK;
    if (c.src_cn == 1) {
        if (resized) {
            rc = front_resize_linear(d->ctx, frame, c.src_width, c.src_height, pitch, 1, d->gray, W, H, d->gray_pitch, s);
        } else {
            hog_img = klt = frame;
            hog_pitch = klt_pitch = pitch;
        }
    } else if (c.make_gray) {
        const int code = gray_code_of(c.src_cn, c.rgb_order);
        rc = resized ? front_cvt_resize_gray(d->ctx, frame, c.src_width, c.src_height, pitch, code, d->gray, W, H,
                                             d->gray_pitch, s)
                     : front_cvt_color(d->ctx, frame, W, H, pitch, d->gray, d->gray_pitch, code, s);
    } else {
        hog_img = frame, hog_pitch = pitch, hog_cn = c.src_cn;
        if (resized) {
            rc = front_resize_linear(d->ctx, frame, c.src_width, c.src_height, pitch, c.src_cn, d->color, W, H,
                                     d->color_pitch, s);
            hog_img = d->color, hog_pitch = d->color_pitch;
        }
        if (rc == TBDK_OK)
            rc = front_cvt_color(d->ctx, hog_img, W, H, hog_pitch, d->gray, d->gray_pitch,
                                 gray_code_of(c.src_cn, c.rgb_order), s);
    }
    if (rc != TBDK_OK) return rc;
    // 2. detectMultiScale; its output order is the reference's (hits sorted into
    // level / row-major window order before groupRectangles, hog.hip fetch_hits)
    int n = 0;
    rc = tbdk_hog_detect_multiscale(d->ctx, hog_img, W, H, hog_pitch, hog_cn, &c.hog, d->svm.data(), (int)d->svm.size(),
                                    d->rects.data(), d->weights.data(), c.max_detections, &n, stream);
    if (rc != TBDK_OK) return rc;
    // 3. Detection(-1, frame, rect, -1.0) per rect (samples/gpu/tbd.cpp:615-621), in that order
    d->dets.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        tbdk_detection& o = d->dets[(size_t)i];
        o.id = -1;
        o.x = d->rects[4 * (size_t)i], o.y = d->rects[4 * (size_t)i + 1];
        o.width = d->rects[4 * (size_t)i + 2], o.height = d->rects[4 * (size_t)i + 3];
        o.confidence = c.confidence_mode == 1 ? d->weights[(size_t)i] : -1.0;
    }
    for (int i = 0; i < n && i < cap; ++i) dets_out[i] = d->dets[(size_t)i];
    if (ndets) *ndets = n;
    // 4. the loop
    return tbdk_tbd_step(d->tbd, klt, klt_pitch, frame_id, d->dets.data(), n, metrics, stream);
}

int tbdk_app_image_default_args(tbdk_app_image_args* a)
{
    if (!a) return TBDK_EINVAL;
    std::memset(a, 0, sizeof(*a));
    a->num_tracking_frames = 100;  // samples/gpu/tbd.cpp:256-257
    a->make_gray = 1;
    a->width = 640, a->height = 480;
    tbdk_tbd_detect_config c;
    tbdk_tbd_detect_default_config(a->width, a->height, &c);
    a->hog = c.hog;
    tbdk_tracker_default_args(&a->tracker);
    return TBDK_OK;
}

int tbdk_app_run_images(const tbdk_app_image_args* a, tbdk_app_image_result* res)
{
    if (!a || !a->image_list_filename || !a->image_list_filename[0] || a->num_tracking_frames < 0 || !a->svm ||
        a->svm_len <= 0 || (a->resize_src && (a->width <= 0 || a->height <= 0)))
        return TBDK_EINVAL;
    if (res) std::memset(res, 0, sizeof(*res));
    // the list, and every file's header and size, before any GPU work
    const std::string list = a->image_list_filename;
    const size_t slash = list.find_last_of('/');
    const std::string dir = slash == std::string::npos ? std::string() : list.substr(0, slash + 1);
    std::ifstream in(list);
    if (!in) return TBDK_EINVAL;
    std::vector<std::string> paths;
    for (std::string line; (int)paths.size() < a->num_tracking_frames && std::getline(in, line);) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty()) continue;
        paths.push_back(line[0] == '/' ? line : dir + line);
    }
    PnmInfo first;
    for (size_t i = 0; i < paths.size(); ++i) {
        PnmInfo pi;
        const int rc = pnm_check_file(paths[i], &pi);
        if (rc != kPnmOk || (i > 0 && (pi.width != first.width || pi.height != first.height || pi.cn != first.cn))) {
            if (a->verbose) std::fprintf(stdout, "error: %s: not a readable P5/P6 frame (%d)\n", paths[i].c_str(), rc);
            return TBDK_EINVAL;
        }
        if (i == 0) first = pi;
    }
    if (paths.empty()) return TBDK_EINVAL;
    const int W = a->resize_src ? a->width : first.width, H = a->resize_src ? a->height : first.height;

    tbdk_ctx* ctx = nullptr;
    tbdk_tbd* tbd = nullptr;
    tbdk_tbd_detector* det = nullptr;
    tbdk_trajectories* traj = nullptr;
    uint8_t* dframe = nullptr;
    int rc = tbdk_ctx_create(a->device, &ctx);
    if (rc != TBDK_OK) return rc;
    tbdk_tbd_config lc;
    tbdk_tbd_default_config(W, H, &lc);
    lc.cost_of_non_assignment = a->tracker.cost_of_non_assignment;
    lc.time_window_size = a->tracker.time_window_size;
    lc.track_age_threshold = a->tracker.track_age_threshold;
    lc.track_visibility_threshold = a->tracker.track_visibility_threshold;
    lc.track_confidence_threshold = a->tracker.track_confidence_threshold;
    lc.bounds_xmin = a->tracker.bounds_xmin, lc.bounds_xmax = a->tracker.bounds_xmax;
    lc.bounds_ymin = a->tracker.bounds_ymin, lc.bounds_ymax = a->tracker.bounds_ymax;
    tbdk_tbd_detect_config dc;
    tbdk_tbd_detect_default_config(W, H, &dc);
    dc.src_width = first.width, dc.src_height = first.height, dc.src_cn = first.cn;
    dc.rgb_order = 1;  // P6 pixels are R, G, B
    dc.make_gray = a->make_gray;
    dc.resize = a->resize_src;
    dc.confidence_mode = a->confidence_mode;
    dc.hog = a->hog;
    const int fpitch = align_up(first.width * first.cn, 64);
    std::vector<uint8_t> file;
    std::vector<uint32_t> ages;
    if ((rc = tbdk_tbd_create(ctx, &lc, &tbd)) == TBDK_OK && (rc = tbdk_trajectories_create(&traj)) == TBDK_OK &&
        (rc = tbdk_tbd_set_trajectories(tbd, traj)) == TBDK_OK &&
        (rc = tbdk_tbd_detector_create(ctx, tbd, &dc, a->svm, a->svm_len, &det)) == TBDK_OK) {
        DeviceGuard g(a->device);
        rc = map_status(dev_alloc(&dframe, (size_t)fpitch * first.height, ctx->opt_alloc_fill));
        for (size_t i = 0; i < paths.size() && rc == TBDK_OK; ++i) {
            PnmInfo pi;
            if (pnm_read_file(paths[i], file, &pi) != kPnmOk || pi.width != first.width || pi.height != first.height ||
                pi.cn != first.cn) {
                rc = TBDK_EINVAL;  // changed since the check
                break;
            }
            rc = map_status(hipMemcpy2D(dframe, (size_t)fpitch, file.data() + pi.offset, (size_t)pi.width * pi.cn,
                                        (size_t)pi.width * pi.cn, (size_t)pi.height, hipMemcpyHostToDevice));
            int n = 0;
            if (rc == TBDK_OK) rc = tbdk_tbd_step_image(det, dframe, fpitch, (int)i, nullptr, 0, &n, nullptr, nullptr);
            if (rc != TBDK_OK) break;
            ages.push_back(1);  // no track history buffer: every frame continues from the previous one
            if (res) {
                res->frames++;
                res->detections += n;
            }
        }
        if (rc == TBDK_OK) {
            tbdk_scenario_metrics m;
            rc = tbdk_tbd_tracking_write(tbd, ages.data(), (int)ages.size(), (int)ages.size(), a->tracking_filepath,
                                         a->verbose, &m);
            if (rc == TBDK_OK && res) res->scenario = m;
        }
        if (dframe) (void)hipFree(dframe);
    }
    if (det) (void)tbdk_tbd_detector_destroy(det);
    if (tbd) (void)tbdk_tbd_destroy(tbd);
    if (traj) (void)tbdk_trajectories_destroy(traj);
    (void)tbdk_ctx_destroy(ctx);
    return rc;
}

}  // extern "C"
