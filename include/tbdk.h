/*
 * tbdk.h — C ABI of the MI355X-native TBD/KLT hot path (libtbdk.so).
 *
 * This is the drop-in boundary for the per-frame tracking-by-detection path of
 * the reference (tkortz/opencv, OpenCV 3.4.7 fork).  Each entry point names the
 * reference interface it replaces.  Conventions:
 *   - plain pointers and sizes; every image/point buffer is DEVICE memory owned
 *     by the caller (hipMalloc / torch), except where a parameter says "host";
 *   - every call is asynchronous on the given HIP stream (passed as void*,
 *     NULL = the legacy default stream); no hidden host sync, no device
 *     globals, so contexts on different devices/threads are independent;
 *   - every call returns an int status (TBDK_OK or a negative TBDK_E*);
 *     n == 0 is a no-op returning TBDK_OK (reference: pyrlk.cpp:221-227
 *     releases the outputs on empty input).
 */
#ifndef TBDK_H
#define TBDK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBDK_OK 0
#define TBDK_EINVAL (-1)   /* bad argument (reference: CV_Assert -> cv::Exception)   */
#define TBDK_EHIP (-2)     /* HIP runtime error (reference: cudaSafeCall)             */
#define TBDK_ENOMEM (-3)   /* device allocation failed                                */
#define TBDK_ENODEV (-4)   /* no such device / no GPU (reference: throw_no_cuda())    */

#define TBDK_MAX_LEVELS 8

/* pixel depths of a pyramid (cv::Mat depth codes: CV_8U = 0; 7 is OpenCV 4's CV_16F) */
#define TBDK_DEPTH_8U 0
#define TBDK_DEPTH_16F 7
#define TBDK_DEPTH_32F 5

/* flags, same values as the reference (video/include/opencv2/video/tracking.hpp:56-57) */
#define TBDK_OPTFLOW_USE_INITIAL_FLOW 4
#define TBDK_OPTFLOW_LK_GET_MIN_EIGENVALS 8

typedef struct tbdk_ctx tbdk_ctx;

/* One pyramid level in device memory.  Interior pixel (x, y) is at
 * data[(y + pad) * pitch + x + pad]; the `pad`-wide frame around it holds
 * BORDER_REFLECT_101 values, as cv::buildOpticalFlowPyramid's padded levels do
 * (video/src/lkpyramid.cpp:726-762). */
typedef struct tbdk_level {
    uint8_t* data;
    int32_t width, height, pitch, pad;
} tbdk_level;

/* A pyramid, the layout of cv::buildOpticalFlowPyramid (lkpyramid.cpp:697-793):
 * lv[i] are the u8 levels, each with a reflect-101 frame of `pad` pixels; with
 * derivatives (tbdk_pyr_create, withDerivatives=true, lkpyramid.cpp:765-780)
 * dv[i] are the Scharr planes of calcSharrDeriv (lkpyramid.cpp:55-144), CV_16SC2
 * interleaved (Ix, Iy) per pixel (4 bytes; pitch in bytes) with a zero
 * (BORDER_CONSTANT) frame of `pad` pixels; without (tbdk_pyr_create_levels)
 * dv[i].data is NULL and tbdk_lk_sparse derives the window's Scharr values
 * itself (same results).  A tbdk_pyr must come from tbdk_pyr_create* (which
 * fill every field); callers never fill one themselves.
 * ABI 2 (TBDK_ABI_VERSION): `depth` and `flags` follow `storage`, so every
 * field before them has its offset of the original (depth-less) layout. */
typedef struct tbdk_pyr {
    int32_t nlevels;                 /* levels built = maxLevel used + 1 */
    int32_t win_w, win_h;            /* window the level count was derived for */
    tbdk_level lv[TBDK_MAX_LEVELS];
    tbdk_level dv[TBDK_MAX_LEVELS];
    void* storage;                   /* owned by the library; free with tbdk_pyr_destroy */
    int32_t depth;                   /* TBDK_DEPTH_8U (tbdk_pyr_create*), TBDK_DEPTH_16F
                                        (tbdk_pyr_create_f16: fp16 levels, fp16 (Ix, Iy)
                                        derivative pairs) or TBDK_DEPTH_32F
                                        (tbdk_pyr_create_f32: fp32 levels and pairs) */
    int32_t flags;                   /* TBDK_PYR_NO_DERIVS: levels only */
    int32_t cn;                      /* channels per pixel, interleaved (1; 2..4 from
                                        tbdk_pyr_create_cn); level rows hold
                                        (width + 2*pad)*cn bytes, derivative rows
                                        (Ix_c, Iy_c) pairs for c = 0..cn-1 */
} tbdk_pyr;

#define TBDK_ABI_VERSION 3   /* 3: tbdk_homography_params, tbdk_homography and tbdk_find_homography */
#define TBDK_PYR_NO_DERIVS 1

/* cv::TermCriteria(COUNT+EPS, maxCount, epsilon) + flags + minEigThreshold of
 * cv::calcOpticalFlowPyrLK (video/include/opencv2/video/tracking.hpp:178-183) */
typedef struct tbdk_lk_params {
    int32_t win_w, win_h;            /* default 21, 21 */
    int32_t max_level;               /* default 3 (clamped to the pyramids) */
    int32_t max_count;               /* default 30, clamped to [0, 100] */
    double epsilon;                  /* default 0.01, clamped to [0, 10] then squared */
    int32_t flags;                   /* TBDK_OPTFLOW_* */
    float min_eig_threshold;         /* default 1e-4 */
    int32_t impl;                    /* 0 auto; 1 register-strip kernel; 2 generic LDS kernel;
                                        3 several points per wave (all bit-identical) */
} tbdk_lk_params;

/* ---- context ------------------------------------------------------------ */

/* Creates a context bound to HIP device `device` (one per thread x device).
 * It also creates the library's side streams (Farneback's level prep, the HOG
 * level lanes): HIP maps streams onto a few hardware queues in creation order,
 * so creating the context before the caller's own streams keeps those side
 * streams off the caller's queue (HOG "Side streams"). */
int tbdk_ctx_create(int device, tbdk_ctx** out);
int tbdk_ctx_destroy(tbdk_ctx* ctx);
/* Context options (test and tuning knobs; TBDK_EINVAL for unknown names):
 *   "gftt_eig_redo" (0/1): treat every row-segment boundary of the GFTT
 *       eigenvalue strips as a fresh-start mismatch, forcing the re-walk
 *       rounds taken when a segment's fresh start differs from the
 *       reference's running box-filter sum (results equal).
 *   "gftt_wide" (0/1, default 0): 0: tbdk_gftt_rois* select a ROI's corners in
 *       one workgroup's LDS where its candidates and accepted corners fit, and
 *       by the wide path (candidates and accepted state in global scratch)
 *       where they do not; 1: every ROI by the wide path (results equal).
 *   "blur_generic" (0/1, default 0): tbdk_gaussian_blur_u8: 1 runs every kernel
 *       size through the instance that takes its sizes at run time; 0: square
 *       kernels of 3, 5, 7 and 11 through their compile-time instances
 *       (results equal).
 *   "pyr_fuse" (0/1, default 1): tbdk_pyr_build of a u8 pyramid: 1
 *       computes level 0's padded copy and level 1 in one launch, then one
 *       launch per level; 0: one launch per level
 *       (results equal).  fp16 / fp32 pyramids: 1 builds L levels in L
 *       role-split launches (level 0's copy, level 1 and level 0's Scharr
 *       plane from the frame, then level i and plane i-1 from level i-1);
 *       0 takes one launch per level and one for every plane (results equal).
 *   "pyr_xcd" (0/1, default 1): the u8 two-role and fp16 / fp32 role-split
 *       pyramid launches deal each role's blocks to the 8 XCDs in contiguous
 *       row bands, so rows a role reads twice share one XCD's L2 (results equal).
 *   "pyr_rows" (1/2/4, default 1): rows per thread of the u8 two-role
 *       launch (pyr_fuse 1: level 0's 16-byte copies of that many rows, level
 *       1 in row pairs sharing their 7 frame rows when > 1) and of the fp16 /
 *       fp32 role-split launches (copies and Scharr planes that many rows,
 *       levels in pairs at most); more than 1 measured slower (fewer waves
 *       to hide the loads' latency), kept for A/B runs (results equal).
 *   "lk_scharr_fly" (0/1, default 0): the several-points-per-wave PyrLK
 *       kernel derives the window's Scharr values from the u8 level even when
 *       the pyramid has derivative planes (it always does without them;
 *       results equal).
 *   "lk_solo" (0..100, default 4): the several-points-per-wave PyrLK kernel
 *       runs a wave's last stepping point on all the wave's lanes (its window
 *       rows split over the lane groups) once the wave's other points have
 *       stopped, from Newton step lk_solo of the level on (0: never; padded
 *       levels only; results equal).
 *   "lk_impl" (0..3): the PyrLK kernel taken when tbdk_lk_params.impl is 0
 *       (the TBD loop's setting): 0 auto, else as tbdk_lk_params.impl
 *       (results equal).
 *   "hog_block_tiled" (0..2, default 1): HOG block histograms of 2x2-cell,
 *       9-bin geometries by the LDS-tiled kernel, its histograms in LDS (1)
 *       or in registers (2); 0 forces the per-cell kernel of every other
 *       geometry (results equal).
 *   "hog_level_streams" (1..4, default 3): tbdk_hog_detect_multiscale runs
 *       the levels' resize/gradient/block chains on this many streams (the
 *       caller's and internal ones, joined back before the window pass;
 *       results equal).
 *   "hog_window_tiled" (0/1, default 1): tbdk_hog_detect_multiscale's window
 *       pass stages each row of 16 windows' blocks and the detector in LDS
 *       (36-float blocks); 0 reads them per window from L2 (results equal).
 *   "fb_prep_ahead" (0/1, default 1): tbdk_farneback computes every level's
 *       images and polynomial expansions on an internal stream, coarse to
 *       fine, while the coarser levels iterate on the caller's stream
 *       (results equal).
 *   "alloc_fill" (-1..255, default -1 = off): a test aid.  While 0..255, every
 *       device allocation the library makes for the context, and for any
 *       object created from it afterwards (pyramids, TBD loops, KLT trackers,
 *       MOG2 subtractors, detectors, tbdk_synth_render's temporary), is filled
 *       with that byte and the device drained before anything else uses it;
 *       the clears the library documents (a pyramid's derivative frames, a
 *       loop's and a tracker's state) follow the fill.  Off, an allocation is
 *       the plain hipMalloc.  Results must not depend on the value. */
int tbdk_ctx_set_option(tbdk_ctx* ctx, const char* name, int64_t value);
/* A test aid: no result may depend on what the context's scratch held before
 * a call, and this call lets a test put known content there.  It synchronises
 * the device, fills every device buffer the context owns (the GFTT, Farneback,
 * dense PyrLK, HOG, morphology and connected-components scratch and the front
 * end's coefficient tables) over its
 * whole capacity with `byte` (0..255), and forgets every cache keyed by host
 * state (the front end's table slots, HOG's uploaded cell plan and detector),
 * so the next call builds and uploads them again.  Buffers not yet allocated
 * are skipped.  Memory of objects (pyramids, loops, trackers, subtractors,
 * detectors) is not touched: they keep state between calls.
 * *bytes_filled (optional): the bytes filled. */
int tbdk_ctx_debug_fill_scratch(tbdk_ctx* ctx, int byte, int64_t* bytes_filled);
/*   "tbd_early_gftt" (0/1/2, default 2): the TBD loop runs GFTT over the
 *       detections that will start new tracks at the start of the step, off
 *       the critical path; 2 also over the box each existing track would get
 *       on a re-detection frame from the detection overlapping it most (a
 *       guess: boxes the tracker step does not confirm take the regular GFTT;
 *       results equal).
 *   "tbd_spec_lookahead" (0/1, default 1): with a look-ahead frame, the TBD
 *       loop starts the next frame's PyrLK of the point sets that stay
 *       unchanged unless their track is deleted before the host tracker step
 *       (results equal).
 *   "tbd_zero_copy" (0/1, default 1; taken by tbdk_tbd_create): the TBD loop's
 *       kernels read their host tables from, and the fit writes its results
 *       to, coherent pinned host memory directly instead of through copies
 *       (results equal).
 *   "tbd_early_la" (0/1/2, default 1): with a look-ahead frame, the TBD loop
 *       tracks this step's early GFTT rows into the next frame right after the
 *       fit (1: on re-detection frames, where no speculative PyrLK runs; 2:
 *       every frame); the next step's refreshed-set PyrLK skips them (results
 *       equal).
 *   "tbd_fit_flag" (0/1, default 1; taken by tbdk_tbd_create, with zero copy):
 *       the fit kernel's last wave publishes the frame's results by a
 *       system-scope flag in pinned memory that the host polls, instead of an
 *       event recorded behind the fit (whose marker held the next frame's
 *       pyramid back; results equal).
 *   "tbd_pyr_derivs" (0/1, default 0; taken by tbdk_tbd_create): the loop's
 *       pyramids carry Scharr derivative planes and PyrLK reads them instead of
 *       deriving the window's values (results equal; A/B runs).
 *   "lk_seg_inline", "tbd_fit_inline", "gftt_inline" (0/1, default 1): the TBD
 *       loop's PyrLK segment lists (up to 256), the fit's per-track table (up
 *       to 256 tracks) and GFTT ROI tables (up to 128 ROIs, also in
 *       tbdk_gftt_rois) travel in the kernel arguments instead of being read
 *       from the staged tables (with zero copy: pinned host memory, one
 *       host-link round trip per first read); larger tables are read from
 *       memory (results equal).
 *   "tbd_fit_wgpub" (0/1, default 1): with the fit flag, each fit workgroup
 *       publishes its tracks' results with one system-scope release (wave 0
 *       stores them), not one release per wave (results equal).
 *   "tbd_la_pyr_side" (0/1/2, default 2): where the TBD loop builds the
 *       look-ahead pyramid: 0 on the caller's stream behind the fit; 1 on its
 *       look-ahead stream behind the step's PyrLK launches, beside the fit; 2 on
 *       the look-ahead stream right after the step's critical PyrLK launch,
 *       behind only the caller's work before the step (the loop keeps three
 *       pyramids, so the one it overwrites is two frames old and no longer
 *       read). The look-ahead PyrLK that follows it needs no cross-stream edge
 *       (results equal).
 *   "tbd_post_direct" (0/1, default 1): after a step that runs no post-tracker
 *       GFTT, the next step's refreshed-set PyrLK waits for the early GFTT's
 *       completion directly rather than through the post-tracker stream's
 *       event (results equal).
 *   "gftt_compact" (0/1, default 1): GFTT with quality <= 1 (blockSize 3,
 *       min-eigenvalue) writes no eigenvalue plane, only its local maxima's
 *       values per strip row (corner lists equal; quality > 1, Harris and other
 *       block sizes keep the plane).
 *   "tbd_gftt_ahead" (0/1, default 1): inside tbdk_tbd_run each step also
 *       launches the NEXT frame's early GFTT over its new-track ROIs (that
 *       frame's detections beyond the bounds filter), over the caller's next
 *       frame, so the refreshed-set PyrLK of the step after it does not wait for
 *       a GFTT launched only one step earlier; the step of that frame launches
 *       just the ROIs it misses (re-detection guesses).  The caller's stream
 *       waits for that work before the call returns (results equal).
 *   "tbd_borrow_l0" (0/1, default 0): inside tbdk_tbd_run the loop's pyramids
 *       take the caller's frames as level 0 (no padded copy; PyrLK reads
 *       windows across a frame's edge by reflect-101 coordinates, the values
 *       the copy holds); when the call returns the last frame's level 0 has
 *       been copied into the loop's own buffer and the caller's stream waits
 *       for the last read of a frame, so the frames may be reused once that
 *       stream is synchronised (results equal; PyrLK measured slower reading
 *       the frames than the loop's reused buffers, so off by default).
 *       tbdk_tbd_step / _step_ahead / _run_host always copy.
 *   "tbd_fit_gate" (0/1, default 1): the TBD loop's host waits (polling) for
 *       the look-ahead PyrLK's completion event and then launches the fit on
 *       the step's stream behind the step's own PyrLK, instead of enqueuing a
 *       cross-stream wait in front of the fit (results equal; A/B runs).
 *   "tbd_fit_ransac" (0..10000, default 0; taken by tbdk_tbd_create): 0: the
 *       TBD loop fits each track's similarity to all its tracked corners
 *       (getRTMatrix); N > 0: the fit is cv::estimateRigidTransform's, RANSAC
 *       with ransacMaxIters = N and ransacGoodRatio = 0.5 over the same
 *       corners (see tbdk_box_propagate_ransac); a track without consensus
 *       gets no KLT prediction in that frame.  The tracked sets themselves
 *       are unchanged (outlier corners are kept).
 *   "tbd_fb_check" (0..1048576, default 0; taken by tbdk_tbd_create): 0: off;
 *       N > 0: every PyrLK launch of the TBD loop is followed by the backward
 *       pass of the forward-backward check (see tbdk_lk_sparse_fb) with
 *       back_threshold = N / 1024 px (1024: the reference samples' 1.0 px).  A
 *       corner that fails it leaves its track's set before the fit, so the fit
 *       (least squares or tbd_fit_ransac), min_points and min_fit_points see
 *       the kept pairs only.  tbdk_frame_metrics: lk_points counts the points
 *       entering the forward pass, klt_points the pairs kept after the check,
 *       lk_iters the forward pass's iterations.
 *   "tbd_subpix" (0..15, default 0; taken by tbdk_tbd_create): 0: off; N > 0:
 *       every corner set the TBD loop's GFTT produces is refined by
 *       tbdk_corner_sub_pix on the frame it was detected on (the whole frame,
 *       not the ROI as an isolated image), window (N, N), no zero zone,
 *       criteria (COUNT|EPS, 20, 0.03), before PyrLK reads it; N = 10 is the
 *       call of the reference's KLT sample (samples/cpp/lkdemo.cpp:85).  The
 *       corner mask does not apply to the refinement.  Frames smaller than
 *       2N + 5 in either dimension make tbdk_tbd_create return TBDK_EINVAL.
 *   "timing_every" (>= 1, default 1): HIP events on a pseudo-random 1/N of the
 *       launches of each kernel selected for timing: launch i (counted per
 *       kernel name from tbdk_timing_enable) is timed iff splitmix64(i) % N == 0
 *       (see tbdk_timing_calls). */

/* device ordinal of the context */
int tbdk_ctx_device(const tbdk_ctx* ctx);

/* Per-kernel timing with HIP events recorded on the launch stream.
 * enable != 0 starts recording (clears previous records). */
int tbdk_timing_enable(tbdk_ctx* ctx, int enable);
/* Synchronises the recorded events and returns, for kernel `name`
 * ("pyr_build", "lk_sparse", "lk_dense" (tbdk_lk_dense), ...), the number of launches and the summed
 * device milliseconds. */
int tbdk_timing_query(tbdk_ctx* ctx, const char* name, int64_t* launches, double* total_ms);
/* Restrict recording to the comma-separated kernel names in `names` (NULL or
 * "" = all).  Each timed launch costs two event records on the host. */
int tbdk_timing_select(tbdk_ctx* ctx, const char* names);
/* Selected launches of kernel `name` since tbdk_timing_enable, timed or not:
 * with the ctx option "timing_every" = N only a 1/N sample of them records events
 * (tbdk_timing_query counts those), to keep the event records' host cost out
 * of a measured loop. */
int tbdk_timing_calls(tbdk_ctx* ctx, const char* name, int64_t* calls);

/* ---- image layout -------------------------------------------------------- */

/* Every entry point that takes an image takes its row pitch in bytes, and a
 * region of interest of a larger frame, a decoder's padded surface or a pitched
 * GpuMat-like buffer is passed as it is, with no copy:
 *   - u8 images, source or destination, 1 to 4 interleaved channels: any
 *     pointer and any pitch >= width * cn.  Nothing has to be aligned; the
 *     kernels choose their wide loads and stores from the addresses they get and
 *     fall back to narrower ones.  Bytes of a row beyond width * cn are never
 *     written, and never read as pixels.
 *   - u16 / fp16 / fp32 images: pointer and pitch multiples of the element size
 *     (2 or 4), pitch >= a row.
 *   - two-value planes (CV_32FC2 flows and gradients, 8 bytes per pixel; the
 *     HOG bin plane, 2 bytes per pixel): pointer and pitch multiples of the
 *     pixel size.
 * A pitch below a row, or one that breaks these rules, is TBDK_EINVAL, and
 * nothing is enqueued.  Results do not depend on the layout.
 * tests/test_gpu_views_*.py check this contract entry point by entry point.
 *
 * Extents.  A pitch is an int, so below 2^31 bytes, and nothing else bounds
 * pitch * height: a small image with a huge pitch (a column crop of a large
 * mosaic, one plane of a huge interleaved surface) is legal, its rows may span
 * 2 GiB, 4 GiB and more, and every kernel forms row addresses in 64 bits.  The
 * exception are the kernels that read the caller's memory through a buffer
 * descriptor, whose sizes and row offsets are 32-bit unsigned (rebasing per row
 * would cost registers on the loop's critical chain): the GFTT eigenvalue walk
 * and PyrLK on a level 0 borrowed from the caller.  They return TBDK_EINVAL,
 * with nothing enqueued, beyond these bounds (in bytes):
 *   - tbdk_gftt_rois, _masked, _px: each ROI's rows may span at most 4294967295
 *     bytes: (roi.height - 1) * pitch + roi.width * pixel bytes, and with a mask
 *     (roi.height - 1) * mask_pitch + roi.width.  The bound is per ROI: a small
 *     ROI may lie anywhere in a frame of any extent.
 *   - tbdk_corner_min_eig_val, and tbdk_corner_response / _px with block_size 3
 *     and no Harris (the same walk, over the whole image as one ROI):
 *     (height - 1) * pitch + width * pixel bytes at most 4294967295.  The other
 *     block sizes and Harris have no bound, and dst_pitch has none.
 *   - tbdk_pyr_build_borrowed: pitch * height at most 4294967295 (and so
 *     tbdk_lk_sparse / tbdk_lk_sparse_fb on that pyramid).
 *   - tbdk_tbd_run: pitch * height at most 4294967295 (its GFTT launched ahead
 *     reads the caller's next frame; with tbd_borrow_l0 PyrLK reads the frames).
 *     tbdk_tbd_step, _step_ahead, _step_image and tbdk_klt_tracker_step copy the
 *     frame into their own pyramid first and have no bound.
 *   - tbdk_tbd_set_corner_mask: (height - 1) * mask_pitch + width at most
 *     4294967295.
 * tests/test_gpu_far_views.py runs every pitch-taking entry point on views that
 * span 2^31 and 2^32 bytes, and each bound at its last accepted and first
 * rejected pitch. */

/* ---- pyramids ------------------------------------------------------------ */

/* Allocates a padded pyramid for width x height u8 frames.  The level count
 * follows cv::buildOpticalFlowPyramid's stop rule for window (win_w, win_h)
 * (video/src/lkpyramid.cpp:782-787).  Not for the hot path (hipMalloc). */
int tbdk_pyr_create(tbdk_ctx* ctx, int width, int height, int max_level,
                    int win_w, int win_h, tbdk_pyr* pyr);
int tbdk_pyr_destroy(tbdk_ctx* ctx, tbdk_pyr* pyr);

/* Builds every level of `pyr` (and its derivative planes) from the device u8
 * image `img` (row pitch in bytes; any pointer, any pitch >= width * cn: "image
 * layout" above).  Replaces cv::buildOpticalFlowPyramid (video/src/lkpyramid.cpp:697)
 * and, level by level, cv::cuda::pyrDown
 * (modules/cudawarping/include/opencv2/cudawarping.hpp:201) — bit-exact with
 * the CPU pyrDown_<FixPtCast<uchar,8>> (imgproc/src/pyramids.cpp:722-857). */
int tbdk_pyr_build(tbdk_ctx* ctx, const uint8_t* img, int pitch, tbdk_pyr* pyr, void* stream);
/* A u8 pyramid without derivative planes (flags TBDK_PYR_NO_DERIVS, dv[i].data
 * NULL): levels only; tbdk_pyr_build writes no Scharr planes (level 0's padded
 * copy and level 1 in one launch, then one launch per level).  PyrLK on it
 * derives the window's Scharr values in the kernel (identical results); the
 * TBD loop's pyramids are of this kind. */
int tbdk_pyr_create_levels(tbdk_ctx* ctx, int width, int height, int max_level, int win_w, int win_h,
                           tbdk_pyr* pyr);
/* Levels 1.. of a levels-only u8 pyramid (tbdk_pyr_create_levels) from the
 * device frame `img`, which becomes level 0 itself: no padded copy, as the
 * pyramid of cv::cuda::SparsePyrLKOpticalFlow, whose level 0 is the input
 * GpuMat (cudaoptflow/src/pyrlk.cpp:144-145).  tbdk_lk_sparse (its
 * several-points-per-wave kernel: impl 0 or 3, 1 channel, window width <= 31)
 * reads that level with buildOpticalFlowPyramid's reflect-101 border
 * (lkpyramid.cpp:726-740) by coordinates, with the same results as the padded
 * copy; other kernels return TBDK_EINVAL.  The frame must stay valid and
 * unchanged while the pyramid is read; the next tbdk_pyr_build gives the
 * pyramid its own level 0 again.  Levels are as tbdk_pyr_build's, bit for bit.
 * Any pointer and any pitch >= width: level 0 keeps the frame's pointer and
 * pitch (pad 0), and PyrLK bounds its reads by them.  TBDK_EINVAL under ctx
 * option pyr_fuse 0 (the one-launch-per-level build has no borrowed form). */
int tbdk_pyr_build_borrowed(tbdk_ctx* ctx, const uint8_t* img, int pitch, tbdk_pyr* pyr, void* stream);

/* Multi-channel frames (cv::cuda::SparsePyrLKOpticalFlow takes 1, 3 or 4
 * channels, cudaoptflow/src/pyrlk.cpp:140-142,197-205; the CPU
 * calcOpticalFlowPyrLK any count, lkpyramid.cpp:55-144,178-695): a pyramid of
 * interleaved cn-channel u8 levels (cn = 1..4) with CV_16SC(2cn) derivative
 * planes.  tbdk_pyr_build fills it from an interleaved frame (pitch >=
 * width*cn); tbdk_lk_sparse on two such pyramids runs LKTrackerInvoker over
 * winW*cn elements per window row (klt_cn.hip). */
int tbdk_pyr_create_cn(tbdk_ctx* ctx, int width, int height, int cn, int max_level, int win_w, int win_h,
                       tbdk_pyr* pyr);

/* The fp16 pixel path (no reference implementation: the
 * reference's CPU PyrLK takes 8-bit levels only, lkpyramid.cpp:1272-1276, and
 * its CUDA class reads CV_32F through textures, cudaoptflow/src/pyrlk.cpp:197-205).
 * A pyramid of fp16 levels (2 bytes per pixel) and fp16 (Ix, Iy) derivative
 * pairs (4 bytes per pixel), same padding and level rule as tbdk_pyr_create.
 * tbdk_pyr_build fills it from a u8 frame (converted exactly);
 * tbdk_pyr_build_f16 from an fp16 frame (pitch in bytes).  Levels follow
 * pyrDown_<FltCast<float,8>> (imgproc/src/pyramids.cpp:722-857) in fp32,
 * rounded to fp16; tbdk_lk_sparse on two such pyramids runs LKTrackerInvoker's
 * algorithm in fp32.
 * Finite domain: a derivative is at most 16 times the largest pixel step, so
 * the fp16 planes are finite for pixel values <= 4094 (16 * 4094 = 65504, the
 * largest finite fp16); 12-bit white (4095) at a hard edge already rounds to
 * an infinity.  Beyond that the levels and planes are still the rounded values
 * (infinities included), and tbdk_lk_sparse returns status 0 for every point
 * whose window position stops being finite: a NaN or infinite position fails
 * the bounds gate like a position outside the level.  No point comes back with
 * status 1 and a non-finite next_pts or err; the next_pts of such a status-0
 * point may be NaN. */
int tbdk_pyr_create_f16(tbdk_ctx* ctx, int width, int height, int max_level,
                        int win_w, int win_h, tbdk_pyr* pyr);
int tbdk_pyr_build_f16(tbdk_ctx* ctx, const uint16_t* img, int pitch, tbdk_pyr* pyr, void* stream);

/* The fp32 pixel path, for the 16U and 32F frames cv::cuda::SparsePyrLK-
 * OpticalFlow takes (cudaoptflow/src/pyrlk.cpp:189-205; the CPU PyrLK has no
 * such path): the fp16 path's algorithm with fp32 levels (4 B per pixel) and
 * fp32 (Ix, Iy) derivative pairs (8 B per pixel), nothing rounded to fp16.
 * tbdk_pyr_build fills it from a u8 frame, tbdk_pyr_build_u16 from a u16
 * frame, tbdk_pyr_build_f32 from an fp32 frame (every conversion exact;
 * pitches in bytes); tbdk_lk_sparse on two such pyramids (impl 0).
 * Finite domain: the window sums hold squares of derivatives (16 times a pixel
 * step) over the window, so they stay finite for pixel values up to about
 * 1e16 (all of 16U is far inside); above that they overflow and, as on the
 * fp16 path, a point whose window position stops being finite gets status 0
 * through the bounds gate, never status 1 with a non-finite result.  Values so
 * small that the squares underflow (1e-30) fail the min-eigenvalue gate. */
int tbdk_pyr_create_f32(tbdk_ctx* ctx, int width, int height, int max_level,
                        int win_w, int win_h, tbdk_pyr* pyr);
int tbdk_pyr_build_u16(tbdk_ctx* ctx, const uint16_t* img, int pitch, tbdk_pyr* pyr, void* stream);
int tbdk_pyr_build_f32(tbdk_ctx* ctx, const float* img, int pitch, tbdk_pyr* pyr, void* stream);
/* The fp32 pixel path on cn = 2..4 interleaved channels: CV_16UC3/C4 and
 * CV_32FC3/C4 frames of cv::cuda::SparsePyrLKOpticalFlow (cudaoptflow/src/
 * pyrlk.cpp:197-205), computed as the CPU path handles channels
 * (lkpyramid.cpp:55-144, 178-695: windows of win_w * cn values, G and b over
 * all of them).  Levels hold cn fp32 values per pixel, the derivative planes
 * an (Ix, Iy) fp32 pair per value; tbdk_pyr_build / _build_u16 / _build_f32
 * take frames of cn interleaved u8 / u16 / fp32 values per pixel;
 * tbdk_lk_sparse (impl 0) tracks on two such pyramids.
 * Semantics are the CPU path's, not the CUDA class's: err is the L1 mean over
 * 32 * win_w * cn * win_h (lkpyramid.cpp:690; pyrlk.cu:555 divides by
 * min(cn, 3) * win_w * win_h instead, and reads 16U frames through normalised
 * [0, 1] textures), and the minEigThreshold gate applies to the raw values (the
 * CUDA class has none).  cn = 2 is accepted here, as buildOpticalFlowPyramid /
 * calcOpticalFlowPyrLK accept it; the typed-frame facades reject it as the
 * CUDA class does (pyrlk.cpp:142,228). */
int tbdk_pyr_create_f32_cn(tbdk_ctx* ctx, int width, int height, int cn, int max_level,
                           int win_w, int win_h, tbdk_pyr* pyr);

/* Synchronous copy of level `level` to host memory (GpuMat::download
 * analogue; not for the hot path).  with_border != 0 copies the padded frame
 * ((height+2*pad) rows of (width+2*pad) pixels), else the interior; rows of
 * width * cn * (1 or 2) bytes by depth (fp16 as raw bits). */
int tbdk_pyr_download(tbdk_ctx* ctx, const tbdk_pyr* pyr, int level, uint8_t* host, int host_pitch,
                      int with_border);
/* Same for the derivative plane of `level` (interior, CV_16SC(2cn) — fp16
 * pairs as raw bits for TBDK_DEPTH_16F — host_pitch in bytes). */
int tbdk_pyr_download_deriv(tbdk_ctx* ctx, const tbdk_pyr* pyr, int level, int16_t* host, int host_pitch);

/* Single-level cv::cuda::pyrDown replacement: dst = pyrDown(src),
 * dst size ((w+1)/2, (h+1)/2), plain (unpadded) device images: any pointers,
 * src_pitch >= w, dst_pitch >= (w+1)/2. */
int tbdk_pyr_down_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch,
                     uint8_t* dst, int dst_pitch, void* stream);

/* ---- sparse pyramidal Lucas-Kanade -------------------------------------- */

/* Replaces cv::cuda::SparsePyrLKOpticalFlow::calc
 * (modules/cudaoptflow/include/opencv2/cudaoptflow.hpp:160-180, impl
 * modules/cudaoptflow/src/pyrlk.cpp:326-349) with the numerics of the CPU
 * cv::calcOpticalFlowPyrLK (video/src/lkpyramid.cpp:1207-1377, 178-695).
 *   prev_pts / next_pts : n x float2 (x, y); next_pts is read as the initial
 *                         guess when TBDK_OPTFLOW_USE_INITIAL_FLOW is set
 *   status              : n x u8 (1 = tracked)
 *   err                 : n x f32 or NULL (L1 patch error / 32 at level 0; the
 *                         minimum eigenvalue with LK_GET_MIN_EIGENVALS; 0 where
 *                         status is 0 and the reference leaves it unset)
 *   iters               : n x i32 or NULL (Newton iterations over all levels)
 * All levels run in one launch.  prev and next must have the same depth; on
 * TBDK_DEPTH_16F / TBDK_DEPTH_32F pyramids the fp16 / fp32 pixel path runs
 * (impl must be 0). */
int tbdk_lk_sparse(tbdk_ctx* ctx, const tbdk_pyr* prev, const tbdk_pyr* next,
                   const float* prev_pts, float* next_pts, uint8_t* status, float* err,
                   int32_t* iters, int n, const tbdk_lk_params* params, void* stream);

/* tbdk_lk_sparse with the forward-backward check of the reference's KLT tracker
 * samples (samples/python/lk_track.py:57-60, checkedTrace in
 * samples/python/lk_homography.py:42-47): the points tracked prev -> next are
 * tracked back next -> prev by a second launch on the same stream (no host
 * synchronisation in between), and a point keeps status 1 iff the forward
 * status is 1, the backward status is 1 and
 *   d = max(|p0.x - p0r.x|, |p0.y - p0r.y|) < back_threshold     (float32)
 * with p0 its prev_pts entry and p0r the point tracked back.  (The samples
 * ignore both statuses; a lost point's coordinates are leftovers of a coarser
 * level, so here both gate the result.)
 *   The backward pass has the forward pass's window, max_level, criteria and
 * min_eig_threshold, flags 0 (it starts at the forward result whether or not
 * the forward pass took an initial flow, and computes no error), and skips the
 * points whose forward status is 0.  params->impl chooses the forward kernel
 * only.
 *   next_pts / err / iters : the forward pass's, bit for bit what tbdk_lk_sparse
 *                            gives, also for rejected points
 *   status                 : as above
 *   back_pts               : n x float2 or NULL: p0r where the forward status
 *                            is 1, the prev_pts entry elsewhere
 *   fb_err                 : n x f32 or NULL: d where both statuses are 1,
 *                            +inf elsewhere
 * back_threshold must be > 0 (+inf: only the statuses gate; NaN or <= 0 is
 * TBDK_EINVAL).  8-bit one-channel pyramids only (padded, with or without
 * derivative planes, or with a borrowed level 0): multi-channel, 16F and 32F
 * pyramids are TBDK_EINVAL.  n == 0 is a no-op.  Timed as "lk_sparse" and
 * "lk_sparse_back". */
int tbdk_lk_sparse_fb(tbdk_ctx* ctx, const tbdk_pyr* prev, const tbdk_pyr* next, const float* prev_pts,
                      float* next_pts, uint8_t* status, float* err, int32_t* iters, float* back_pts,
                      float* fb_err, int n, const tbdk_lk_params* params, float back_threshold, void* stream);

/* Replaces cv::cuda::DensePyrLKOpticalFlow::calc(I0, I1, flow)
 * (cudaoptflow/include/opencv2/cudaoptflow.hpp:182-208, impl cudaoptflow/src/pyrlk.cpp:238-299)
 * with the CPU calcOpticalFlowPyrLK numerics at every pixel (the point grid
 * (x, y) of level 0 through the tbdk_lk_sparse kernels):
 *   flow   : device CV_32FC2, (nextPt.x - x, nextPt.y - y) per pixel, flow_pitch in bytes
 *   status : device u8 plane (status_pitch bytes) or NULL
 * TBDK_OPTFLOW_USE_INITIAL_FLOW is ignored, as in the reference (dense() never
 * reads the incoming flow); win_w/win_h <= 2 is TBDK_EINVAL (pyrlk.cpp:243).
 * With 8-bit one-channel pyramids carrying derivative planes (pads >= win + 2)
 * and an odd square window of 7..31, the previous pyramid's windows come from
 * per-phase case images (8 B per level position and sub-pixel phase: about one
 * frame of entries per level, ~71 MB at 1080p, win 13, maxLevel 3); otherwise
 * per-pixel scratch (17 B per pixel).  Either buffer is owned by the context
 * and grown on demand (growth frees the old buffer, which waits for the
 * device), so dense calls on one context must not overlap on different
 * streams: order them, or give each stream its own context. */
int tbdk_lk_dense(tbdk_ctx* ctx, const tbdk_pyr* prev, const tbdk_pyr* next, float* flow, int flow_pitch,
                  uint8_t* status, int status_pitch, const tbdk_lk_params* params, void* stream);

/* ---- good features to track over box ROIs --------------------------------- */

typedef struct tbdk_roi {
    int32_t x, y, width, height;     /* must lie inside the image */
} tbdk_roi;

/* cv::cuda::createGoodFeaturesToTrackDetector(CV_8UC1, maxCorners, qualityLevel,
 * minDistance, blockSize=3, useHarrisDetector=false)
 * (modules/cudaimgproc/include/opencv2/cudaimgproc.hpp:603-604) */
typedef struct tbdk_gftt_params {
    int32_t max_corners;             /* > 0 */
    double quality_level;            /* > 0 */
    double min_distance;             /* >= 0 */
    int32_t block_size;              /* 1..63: cornerEigenValsVecs' box filter size */
    int32_t use_harris;              /* 0: cornerMinEigenVal, 1: cornerHarris */
    double harris_k;                 /* Harris k (cudaimgproc.hpp:604 default 0.04) */
} tbdk_gftt_params;

/* Replaces CornersDetector::detect (modules/cudaimgproc/src/gftt.cpp:98-213)
 * applied to each ROI as an isolated image, with the CPU goodFeaturesToTrack
 * semantics (imgproc/src/featureselect.cpp:361-516: max over the ROI,
 * deterministic value/address ordering, greedy min-distance) — all ROIs of a
 * frame in one batch and with no host synchronisation.
 *   img        : device u8 image (width x height, row pitch in bytes)
 *   rois       : HOST array of nroi ROIs (copied during the call)
 *   corners    : device, nroi x max_corners x float2, frame coordinates
 *   counts     : device, nroi int32: corners found, never negative here.  Any
 *                ROI size up to the whole frame and any max_corners: a ROI with
 *                more candidates than the on-chip buffer holds (16384 at most,
 *                fewer for a large max_corners), or with an accepted list that
 *                does not fit there, is selected by the wide path in global
 *                scratch, with the same corners (option "gftt_wide"; timing name
 *                "gftt_wide" for its launches, beside "gftt").  The value -1
 *                (candidate overflow, never a truncated list) stays reserved:
 *                the TBD loop's own GFTT still reports it, and
 *                tbdk_corner_sub_pix leaves such rows untouched.
 * Scratch grows on demand (tbdk_gftt_reserve avoids allocation in the call: it
 * covers the wide path too, 20 more bytes per ROI pixel, which a call otherwise
 * allocates when it first routes a ROI there); it is the context's: calls on
 * one context from different streams must be ordered by the caller (a TBD
 * loop has scratch of its own). */
int tbdk_gftt_rois(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch,
                   const tbdk_roi* rois, int nroi, const tbdk_gftt_params* params,
                   float* corners, int32_t* counts, void* stream);

/* tbdk_gftt_rois under an arbitrary 8-bit mask: goodFeaturesToTrack's `mask`
 * argument (featureselect.cpp:361-516; CornersDetector::detect's, gftt.cpp:98).
 *   mask       : device u8 plane, width x height in the image's coordinates,
 *                rows mask_pitch bytes apart (>= width), no alignment
 *                requirement on pointer or pitch; ROI r reads
 *                mask + r.y * mask_pitch + r.x.  NULL: tbdk_gftt_rois exactly.
 * Per ROI the result is the CPU goodFeaturesToTrack on the ROI as an isolated
 * image with the mask cropped to the same rectangle:
 *   - the response map does not depend on the mask;
 *   - maxVal is the maximum of the response over the ROI's pixels (border
 *     pixels included) whose mask byte is non-zero (any of 1..255), 0 when
 *     there is none (minMaxIdx under an empty mask) -- such a ROI has 0 corners;
 *   - the threshold at (float)(maxVal * quality_level) and the 3x3 dilation run
 *     over every pixel of the ROI: a masked-out neighbour with a larger
 *     response still suppresses a masked-in pixel;
 *   - a candidate is an interior pixel with val != 0, val == dilated and a
 *     non-zero mask byte; sort, min-distance walk and max_corners as unmasked;
 *   - when the candidates that pass the mask exceed the on-chip capacity the
 *     ROI goes through the wide path, as in tbdk_gftt_rois.
 * So the corners differ from those of an unmasked call filtered by the mask.
 * TBDK_EINVAL for mask != NULL && mask_pitch < width. */
int tbdk_gftt_rois_masked(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch,
                          const uint8_t* mask, int mask_pitch,
                          const tbdk_roi* rois, int nroi, const tbdk_gftt_params* params,
                          float* corners, int32_t* counts, void* stream);

/* cv::cuda::createMinEigenValCorner(CV_8UC1, blockSize 3, ksize 3,
 * BORDER_REFLECT_101)->compute(src, dst) (cudaimgproc/src/corners.cpp:150-189,
 * cudaimgproc.hpp:564): the minimum-eigenvalue map GFTT selects from, with
 * the CPU cornerMinEigenVal numerics (float Sobel, double box sums).
 * dst: device float plane, dst_pitch in bytes.  Uses the context's GFTT
 * scratch (one launch + one device copy on `stream`). */
int tbdk_corner_min_eig_val(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, float* dst,
                            int dst_pitch, void* stream);
/* The corner response map of any blockSize (ksize 3, BORDER_REFLECT_101):
 * cv::cuda::createMinEigenValCorner(CV_8UC1, blockSize, 3) (harris == 0) and
 * cv::cuda::createHarrisCorner(CV_8UC1, blockSize, 3, k) (harris != 0)
 * (cudaimgproc.hpp:548-566, corners.cpp:150-189), with the CPU
 * cornerMinEigenVal / cornerHarris numerics (corner.cpp:52-152,237-326;
 * Harris in the code paths an AVX x86-64 host runs).
 * block_size 3 without Harris is tbdk_corner_min_eig_val. */
int tbdk_corner_response(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, float* dst,
                         int dst_pitch, int block_size, int harris, double harris_k, void* stream);
int tbdk_gftt_reserve(tbdk_ctx* ctx, int max_rois, int64_t max_total_pixels);

/* GFTT and the corner response maps on 8U, 16U and 32F one-channel images.
 * cornerEigenValsVecs takes CV_8UC1 or CV_32FC1 (imgproc/src/corner.cpp:258), and
 * with it goodFeaturesToTrack, cornerMinEigenVal, cornerHarris and the
 * cv::cuda::create*Corner / createGoodFeaturesToTrackDetector(srcType, ...)
 * factories.  pix selects the pixel type of img: */
#define TBDK_PIX_U8  0
#define TBDK_PIX_U16 1
#define TBDK_PIX_F32 2
/* TBDK_PIX_U8 : tbdk_gftt_rois / tbdk_gftt_rois_masked / tbdk_corner_response
 *               themselves (identical outputs).
 * TBDK_PIX_F32: the reference's CV_32F path: the Sobel scale is
 *               1 / (4 * blockSize) (the x 255 of the 8-bit path is not applied)
 *               and the ksize-3 row filter is the float one (Dx row
 *               S[x+1] - S[x-1]; Dy row S[x]*k0 + (S[x-1] + S[x+1])*k1, unfused);
 *               everything from the column pass on is as for 8-bit images.
 * TBDK_PIX_U16: an extension (the reference rejects CV_16U): exactly the
 *               TBDK_PIX_F32 result on the image converted to float (the
 *               conversion is exact and happens in the kernels' loads).
 * pitch is in bytes.  Pixels must be finite: results equal the reference's
 * wherever the reference's own intermediates stay finite; NaN and Inf pixels,
 * and images whose covariances overflow, give unspecified values (never a
 * fault or a hang).  On float data with a wide exponent range the eigenvalue
 * walk's row segments rarely start on the reference's running sum; they are
 * then walked again in the reference's order, so the result stays exact and
 * the call takes up to a few times longer.
 * mask NULL: unmasked.  Scratch, the wide path for large ROIs, the
 * "gftt_compact" / "gftt_eig_redo" options and the timing names are those of
 * the 8-bit entries.
 * TBDK_EINVAL: an unknown pix; an F32 img pointer or pitch that is not a
 * multiple of 4; a U16 one that is not a multiple of 2; pitch below a row's
 * bytes; whatever the 8-bit entries reject. */
int tbdk_gftt_rois_px(tbdk_ctx* ctx, const void* img, int pix, int width, int height, int pitch,
                      const uint8_t* mask, int mask_pitch,
                      const tbdk_roi* rois, int nroi, const tbdk_gftt_params* params,
                      float* corners, int32_t* counts, void* stream);
int tbdk_corner_response_px(tbdk_ctx* ctx, const void* img, int pix, int width, int height, int pitch,
                            float* dst, int dst_pitch, int block_size, int harris, double harris_k, void* stream);

/* ---- sub-pixel corner refinement ----------------------------------------------- */

/* cv::cornerSubPix(image, corners, winSize, zeroZone, criteria)
 * (imgproc/include/opencv2/imgproc.hpp; imgproc/src/cornersubpix.cpp:44-156) */
typedef struct tbdk_subpix_params {
    int32_t win_w, win_h;        /* half sizes, 1..15 each (the window is 2*win+1) */
    int32_t zero_w, zero_h;      /* half sizes of the zero zone; (-1,-1): none */
    int32_t criteria;            /* 1 COUNT, 2 EPS, 3 both (cv::TermCriteria::Type) */
    int32_t max_count;
    double  epsilon;
} tbdk_subpix_params;
/* the call of the reference's KLT sample (samples/cpp/lkdemo.cpp:85):
 * (10,10), (-1,-1), COUNT|EPS, 20, 0.03 */
int tbdk_subpix_default_params(tbdk_subpix_params* p);
/* Replaces cv::cornerSubPix on a batch of point rows, on the device and with no
 * host synchronisation; the reference has a CPU implementation only, and every
 * refined point equals its result bit for bit (TBDK_PIX_U8 and TBDK_PIX_F32;
 * TBDK_PIX_U16, which the reference rejects, gives the F32 result of the same
 * pixel values).
 *   img      : device one-channel image (pix: TBDK_PIX_*; pitch in bytes)
 *   corners  : device, nrows x row_cap x float2, refined in place
 *   counts   : device, nrows int32, as tbdk_gftt_rois writes them: the first
 *              counts[r] points of row r are refined; counts[r] <= 0 (the -1
 *              overflow mark included) leaves the row untouched, larger values
 *              are clamped to row_cap.  NULL: every row is full (a flat list
 *              of n points is nrows = 1, row_cap = n).
 * A point outside the image is processed as the reference does (replicated
 * border).  The zero zone applies when both halves are >= 0 and smaller than
 * the window's, else it is ignored; max_count is clamped to 1..100 (100 without
 * COUNT), epsilon below 0 counts as 0.  NaN coordinates or pixels give
 * unspecified values, never a fault or a hang.
 * TBDK_EINVAL: win outside 1..15; an image smaller than 2*win + 5 in either
 * dimension; criteria outside 1..3; a non-finite epsilon; an unknown pix; the
 * pointer and pitch rules of tbdk_gftt_rois_px; nrows or row_cap below 0.
 * nrows * row_cap == 0 is a no-op.  The call allocates nothing and uses no
 * context scratch, so it may run on any stream.  Timed as "corner_sub_pix". */
int tbdk_corner_sub_pix(tbdk_ctx* ctx, const void* img, int pix, int width, int height, int pitch,
                        float* corners, const int32_t* counts, int nrows, int row_cap,
                        const tbdk_subpix_params* params, void* stream);
/* HOST only: the (2*win_h+1) x (2*win_w+1) window mask tbdk_corner_sub_pix uses
 * (cornersubpix.cpp:71-93: float products of glibc expf values, zero zone
 * applied), row-major into `mask`. */
int tbdk_corner_sub_pix_mask(const tbdk_subpix_params* params, float* mask);

/* ---- KLT box propagation ----------------------------------------------------- */

/* Result of fitting one box's tracked corners (prev -> next). */
typedef struct tbdk_box_fit {
    double m[6];                     /* 2x3 row-major [p -q tx; q p ty] */
    double cx, cy;                   /* the box's integer centre (x + w/2, y + h/2) mapped by m */
    int32_t npoints;                 /* correspondences used (status != 0) */
    int32_t valid;                   /* npoints >= min_points, non-singular, scale in (0.5, 2) */
} tbdk_box_fit;

/* Batched similarity fit per box: the non-full-affine getRTMatrix of
 * cv::estimateRigidTransform (video/src/lkpyramid.cpp:1398-1470) on each box's
 * corner pairs, then the box centre mapped through it — the Track::motionModel
 * (tbd.hpp:111) the TBD loop uses instead of constant velocity.
 *   prev_pts, next_pts : device float2 arrays (all boxes' points, concatenated)
 *   status             : device u8 per point (NULL = all used)
 *   offsets            : device int32, nboxes + 1: box i owns points [offsets[i], offsets[i+1])
 *   boxes              : device tbdk_roi per box
 *   out                : device tbdk_box_fit per box */
int tbdk_box_propagate(tbdk_ctx* ctx, const float* prev_pts, const float* next_pts, const uint8_t* status,
                       const int32_t* offsets, const tbdk_roi* boxes, int nboxes, int min_points,
                       tbdk_box_fit* out, void* stream);

/* RANSAC parameters of cv::estimateRigidTransform's 6-argument overload
 * (ransacMaxIters, ransacGoodRatio; ransacSize0 is 3). */
typedef struct tbdk_ransac_params {
    int32_t max_iters;               /* 1..10000, reference default 500 */
    double good_ratio;               /* [0, 1], reference default 0.5 */
} tbdk_ransac_params;
int tbdk_ransac_default_params(tbdk_ransac_params* p);

/* Batched cv::estimateRigidTransform(A, B, fullAffine = false) on point sets
 * (video/src/lkpyramid.cpp:1591-1688), one box per set: the consensus set is
 * found by the reference's RANSAC (its cv::RNG sequence, seeded per set, its
 * redraw and abandon rules, its inlier threshold from boundingRect(next)), then
 * getRTMatrix is fitted to the inliers and the box centre mapped through it.
 * Arguments as tbdk_box_propagate, plus:
 *   out[i].npoints : consensus size the final fit used (0 without consensus);
 *                    -1 if the box has more than 1024 status != 0 pairs (the
 *                    set is never truncated; valid = 0)
 *   out[i].valid   : consensus found, npoints >= min_points, non-singular,
 *                    scale in (0.5, 2), centre finite; without a transform
 *                    valid = 0 and m is the identity
 *   iters          : device int32 per box or NULL: the round k at which
 *                    consensus was reached, -1 if none
 *   inliers        : device u8 per point or NULL: 1 for consensus members, 0
 *                    for outliers, status == 0 points and boxes without consensus
 * The work per box is bounded by max_iters rounds of up to 2 * max_iters draws
 * (reached by coincident or collinear sets).  TBDK_EINVAL for parameters out
 * of range.  Timed as kernel "box_propagate_ransac". */
int tbdk_box_propagate_ransac(tbdk_ctx* ctx, const float* prev_pts, const float* next_pts, const uint8_t* status,
                              const int32_t* offsets, const tbdk_roi* boxes, int nboxes, int min_points,
                              const tbdk_ransac_params* params, tbdk_box_fit* out, int32_t* iters, uint8_t* inliers,
                              void* stream);

/* ---- findHomography --------------------------------------------------------- */

#define TBDK_HOMOGRAPHY_LSQ 0      /* method 0: all pairs */
#define TBDK_HOMOGRAPHY_RANSAC 8   /* cv::RANSAC */
#define TBDK_HOMOGRAPHY_MAX_PAIRS 4096  /* status != 0 pairs of one set the kernel holds */
typedef struct tbdk_homography_params {
    int32_t method;                /* 0 or 8; 4 (LMEDS) and 16 (RHO) are TBDK_EINVAL */
    double  reproj_threshold;      /* <= 0 means 3, as the reference */
    int32_t max_iters;             /* 1..10000, reference default 2000 */
    double  confidence;            /* (0, 1), reference default 0.995 */
    int32_t refine;                /* 1: the reference's LM step; 0: stop before it */
} tbdk_homography_params;
typedef struct tbdk_homography {
    double  h[9];                  /* row-major, h[8] == 1; identity when !valid */
    int32_t npoints;               /* status != 0 pairs; -1 over the cap */
    int32_t ninliers;              /* consensus size (npoints for method 0) */
    int32_t iters;                 /* RANSAC iterations the reference's loop would have run */
    int32_t valid;                 /* the reference returned a non-empty H */
} tbdk_homography;
/* method RANSAC, threshold 3, 2000 iterations, confidence 0.995, refine 1 */
int tbdk_homography_default_params(tbdk_homography_params* p);

/* Batched cv::findHomography(src, dst, method, reproj_threshold, mask, max_iters,
 * confidence) on point sets (calib3d/src/fundam.cpp:350-433), one workgroup
 * per set, nothing on the host: method 0 fits all pairs, RANSAC runs the
 * reference's loop (its cv::RNG sequence seeded per set, getSubset's redraws and
 * checkSubset, the normalised 4-point DLT with the reference's Jacobi, the float
 * reprojection error, the strict "first best model wins" rule and
 * RANSACUpdateNumIters), re-fits on the inliers in point order and, with
 * refine = 1, runs the reference's 10-iteration LM step.
 *   src_pts, dst_pts : device float pairs; set i is [offsets[i], offsets[i+1])
 *   status           : device u8 per pair or NULL; status == 0 pairs are dropped
 *                      by an in-order compaction before anything else
 *   offsets          : nsets + 1 device int32 values, as tbdk_box_propagate
 *   out[i]           : device; see tbdk_homography.  A set with fewer than 4
 *                      pairs, with no acceptable subset in iteration 0, or
 *                      without consensus has valid = 0 and the identity.  Method
 *                      0 with fewer than 4 pairs gives valid = 0 too (the
 *                      reference returns a meaningless matrix there).  A set
 *                      with more than TBDK_HOMOGRAPHY_MAX_PAIRS status != 0 pairs
 *                      is never truncated: npoints = -1, valid = 0
 *   mask             : device u8 per pair or NULL: 1 for the inliers (every
 *                      status != 0 pair for method 0 and for 4 pairs), 0 for
 *                      outliers, status == 0 pairs and sets without a result;
 *                      every byte is written once
 * With refine = 0, ninliers, iters, the mask and h are the reference's bit for
 * bit (RANSACUpdateNumIters' log and pow aside); the refined h
 * agrees with the reference's in what it does to the inlier points.  Points
 * that are NaN or infinite leave the call bounded; what h they give is
 * unspecified.  Asynchronous on `stream`, no allocation, no host
 * synchronisation; nsets == 0 is a no-op.  TBDK_EINVAL for parameters out of
 * range.  Timed as kernel "find_homography". */
int tbdk_find_homography(tbdk_ctx* ctx, const float* src_pts, const float* dst_pts, const uint8_t* status,
                         const int32_t* offsets, int nsets, const tbdk_homography_params* params,
                         tbdk_homography* out, uint8_t* mask, void* stream);

/* ---- estimateAffine2D / estimateAffinePartial2D ---------------------------------- */

#define TBDK_AFFINE2D_FULL 0      /* estimateAffine2D, 3-point model */
#define TBDK_AFFINE2D_PARTIAL 1   /* estimateAffinePartial2D, 2-point model */
#define TBDK_AFFINE2D_RANSAC 8    /* cv::RANSAC */
#define TBDK_AFFINE2D_LMEDS 4     /* cv::LMEDS */
#define TBDK_AFFINE2D_MAX_PAIRS 4096  /* status != 0 pairs of one set the kernel holds */
typedef struct tbdk_affine2d_params {
    int32_t model;                 /* TBDK_AFFINE2D_FULL or _PARTIAL */
    int32_t method;                /* TBDK_AFFINE2D_RANSAC or _LMEDS */
    double  reproj_threshold;      /* RANSAC only; taken as given (<= 0 is not defaulted, as the reference) */
    int32_t max_iters;             /* 1..10000, reference default 2000 */
    double  confidence;            /* (0, 1), reference default 0.99 */
    int32_t refine_iters;          /* 0..100 LM iterations, reference default 10; 0: stop before the LM step */
} tbdk_affine2d_params;
typedef struct tbdk_affine2d {
    double  m[6];                  /* 2x3 row-major; [1 0 0; 0 1 0] when !valid */
    int32_t npoints;               /* status != 0 pairs; -1 over the cap */
    int32_t ninliers;              /* pairs the mask marks */
    int32_t iters;                 /* RANSAC: iterations the reference's loop would have run; LMEDS: hypotheses
                                    * evaluated; 0 when npoints equals the model's point count */
    int32_t valid;                 /* the reference returned a non-empty matrix */
} tbdk_affine2d;
/* model FULL, method RANSAC, threshold 3, 2000 iterations, confidence 0.99, 10 refinement iterations */
int tbdk_affine2d_default_params(tbdk_affine2d_params* p);

/* Batched cv::estimateAffine2D / cv::estimateAffinePartial2D(from, to, inliers, method,
 * ransacReprojThreshold, maxIters, confidence, refineIters) on point sets
 * (calib3d/src/ptsetreg.cpp:821-980), one workgroup per set, nothing on the host: the
 * reference's cv::RNG sequence seeded per set, getSubset's redraws and checkSubset, the
 * closed-form 3-point or 2-point solver, the float error, RANSAC's strict "first best
 * model wins" rule with RANSACUpdateNumIters or LMEDS's least median and its sigma, then
 * the reference's LM refinement on the inliers in point order.
 *   src_pts, dst_pts, status, offsets : as tbdk_find_homography
 *   out[i]  : device; see tbdk_affine2d.  A set with fewer pairs than the model has
 *             points (3 or 2), with no acceptable subset in iteration 0 or without
 *             consensus has valid = 0 and the identity.  A set with exactly that many
 *             pairs gets the solver's matrix (it may be NaN for degenerate pairs, as in
 *             the reference).  More than TBDK_AFFINE2D_MAX_PAIRS status != 0 pairs: the
 *             set is never truncated, npoints = -1, valid = 0
 *   mask    : device u8 per pair or NULL: 1 for the inliers, 0 for outliers, status == 0
 *             pairs and sets without a result; every byte is written once
 * With refine_iters = 0, ninliers, iters, the mask and m are the reference's bit for bit
 * (RANSACUpdateNumIters' log and pow aside); the refined m agrees with the
 * reference's in what it does to the inlier points.  NaN or infinite points leave the
 * call bounded; what m they give is unspecified.  Asynchronous on `stream`, no
 * allocation, no host synchronisation; nsets == 0 is a no-op.  TBDK_EINVAL for max_iters
 * outside 1..10000, confidence outside (0, 1), refine_iters outside 0..100, an unknown
 * model or method, a non-finite threshold.  Timed as kernel "estimate_affine2d". */
int tbdk_estimate_affine_2d(tbdk_ctx* ctx, const float* src_pts, const float* dst_pts, const uint8_t* status,
                            const int32_t* offsets, int nsets, const tbdk_affine2d_params* params,
                            tbdk_affine2d* out, uint8_t* mask, void* stream);

/* ---- affine warp ------------------------------------------------------------ */

/* interpolation flags / border modes: the reference's values
 * (imgproc/include/opencv2/imgproc.hpp INTER_*, WARP_INVERSE_MAP;
 *  core/include/opencv2/core/base.hpp BORDER_*) */
#define TBDK_INTER_NEAREST 0
#define TBDK_INTER_LINEAR 1
#define TBDK_INTER_CUBIC 2            /* remapBicubic, BicubicTab_i (imgwarp.cpp:152-268, 860-958) */
#define TBDK_INTER_AREA 3            /* treated as INTER_LINEAR, as cv::warpAffine does */
#define TBDK_WARP_INVERSE_MAP 16
#define TBDK_BORDER_CONSTANT 0
#define TBDK_BORDER_REPLICATE 1
#define TBDK_BORDER_REFLECT 2
#define TBDK_BORDER_WRAP 3
#define TBDK_BORDER_REFLECT_101 4
#define TBDK_BORDER_TRANSPARENT 5

/* Replaces cv::cuda::warpAffine(src, dst, M, dsize, flags, borderMode, borderValue, stream)
 * (modules/cudawarping/include/opencv2/cudawarping.hpp:126; impl cudawarping/src/warp.cpp:183-320)
 * for CV_8UC1, with the numerics of the CPU cv::warpAffine
 * (imgproc/src/imgwarp.cpp:2572-2682: 10-bit fixed-point map, 5-bit sub-pixel
 * table, 15-bit bilinear weights) — bit-exact with it.
 *   src, dst : device u8 images (row pitch in bytes; any pointers, any pitches
 *              >= the widths; bytes of dst beyond dst_width in a row are not
 *              written); dst must not alias src
 *   M        : HOST 2x3 row-major double matrix (dst <- src unless
 *              TBDK_WARP_INVERSE_MAP, then dst -> src, as in the reference)
 *   flags    : TBDK_INTER_NEAREST / LINEAR / CUBIC / AREA | TBDK_WARP_INVERSE_MAP
 *   border   : TBDK_BORDER_*; border_value used by BORDER_CONSTANT */
int tbdk_warp_affine_u8(tbdk_ctx* ctx, const uint8_t* src, int src_width, int src_height, int src_pitch,
                        uint8_t* dst, int dst_width, int dst_height, int dst_pitch, const double* M,
                        int flags, int border, int border_value, void* stream);

/* tbdk_warp_affine_u8 with the matrix in DEVICE memory, for a matrix an earlier call on the same
 * stream produced (&out[i].m[0] of tbdk_estimate_affine_2d): no host round trip between the two.
 *   M     : device pointer to 6 doubles, 8-byte aligned; read when the kernel runs.  It is inverted
 *           on the device with tbdk_warp_affine_u8's arithmetic unless TBDK_WARP_INVERSE_MAP, so
 *           for the same matrix the result is byte-identical to tbdk_warp_affine_u8
 *   valid : device int32 or NULL (&out[i].valid).  Where it reads 0, or an entry of M is not
 *           finite, dst is left untouched
 * Timing name "warp_affine_dev". */
int tbdk_warp_affine_u8_dev(tbdk_ctx* ctx, const uint8_t* src, int src_width, int src_height, int src_pitch,
                            uint8_t* dst, int dst_width, int dst_height, int dst_pitch, const double* M,
                            const int32_t* valid, int flags, int border, int border_value, void* stream);

/* ---- remap, warpPerspective, warp by a dense flow --------------------------- */

/* map kinds of tbdk_remap (cv::remap's map1 / map2 types) */
#define TBDK_MAP_32FC2 0             /* map1: CV_32FC2 (x, y); map2 unused */
#define TBDK_MAP_32FC1 1             /* map1: CV_32FC1 x, map2: CV_32FC1 y */
#define TBDK_MAP_16SC2 2             /* map1: CV_16SC2 (x, y); map2: CV_16UC1 fraction words (convertMaps' form),
                                      * or NULL: whole-pixel positions, TBDK_INTER_NEAREST only */

/* Replaces cv::cuda::remap(src, dst, xmap, ymap, interpolation, borderMode, borderValue, stream)
 * (modules/cudawarping/include/opencv2/cudawarping.hpp) with the numerics of the CPU cv::remap
 * (imgproc/src/imgwarp.cpp:1664-1830: 5-bit sub-pixel positions, 15-bit fixed-point weights for 8U,
 * the float weight table for 32F): bit-exact with it, whatever the map holds.  NaN, +-inf and values
 * far outside the image are valid map entries (cvRound gives 0x80000000 for them, which saturates
 * to -32768); no map value makes the kernel read outside the source.
 *   src, dst : device images of `cn` (1..4) channels, pix TBDK_PIX_U8 or TBDK_PIX_F32, pitches in
 *              bytes (F32: pointers and pitches multiples of 4); every side below 32767, as the
 *              reference asserts; dst must not alias src or a map; an empty dst is a no-op
 *   map1/2   : device maps of dst's size (map_kind above; float maps 4-byte, short maps 2-byte
 *              aligned).  A fraction word is taken & 1023, as the reference does.  With
 *              TBDK_INTER_NEAREST a fraction plane moves the position by the reference's
 *              NNDeltaTab_i (plus one where the fraction is below one half, imgwarp.cpp:237-238).
 *              TBDK_MAP_16SC2 without map2 and an interpolating mode is TBDK_EINVAL (the reference
 *              reads the shorts as floats there)
 *   interpolation : TBDK_INTER_NEAREST / LINEAR / AREA (= LINEAR), and CUBIC for TBDK_PIX_U8
 *              (TBDK_PIX_F32 with CUBIC is TBDK_EINVAL)
 *   border   : TBDK_BORDER_*; border_value[4], each saturated to the pixel type per channel
 * Asynchronous on `stream`; no host synchronisation, no allocation.  Timing name "remap". */
int tbdk_remap(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height, int src_pitch,
               void* dst, int dst_width, int dst_height, int dst_pitch, const void* map1, int map1_pitch,
               const void* map2, int map2_pitch, int map_kind, int interpolation, int border,
               const double* border_value, void* stream);

/* tbdk_remap by the map grid + sign * flow, formed in registers and never stored:
 * mapx = (float)x + sign * flow.x, mapy = (float)y + sign * flow.y (one float32 addition each),
 * decoded as a CV_32FC2 map.  Equal, byte for byte, to tbdk_remap with that map.
 *   flow : device CV_32FC2 (dx, dy) per destination pixel, as tbdk_farneback and tbdk_lk_dense
 *          write it; flow_pitch in bytes
 *   sign : +1 samples at p + flow (warps frame B onto frame A, given the flow A -> B);
 *          -1 samples at p - flow (warp_flow of samples/python/opt_flow.py)
 * Timing name "remap_flow". */
int tbdk_remap_flow(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height, int src_pitch,
                    void* dst, int dst_width, int dst_height, int dst_pitch, const float* flow, int flow_pitch,
                    int sign, int interpolation, int border, const double* border_value, void* stream);

/* Replaces cv::cuda::warpPerspective(src, dst, M, dsize, flags, borderMode, borderValue, stream)
 * with the numerics of the CPU cv::warpPerspective (imgwarp.cpp:2706-2797, 2881-2990): the
 * projective map in double, formed from each 64-column block's origin as the reference forms it
 * (wider blocks for destinations of fewer than 16 rows), then tbdk_remap's sampling.
 *   M     : HOST 3x3 row-major double matrix, src -> dst unless TBDK_WARP_INVERSE_MAP; inverted on
 *           the host as cv::invert does (a singular matrix gives the zero matrix: every pixel then
 *           samples (0, 0)).  All nine entries must be finite, otherwise TBDK_EINVAL
 *   flags : TBDK_INTER_* | TBDK_WARP_INVERSE_MAP
 * Not equal to tbdk_warp_affine_u8 for an affine M: the two round differently, as the
 * reference's two functions do.  Timing name "warp_perspective". */
int tbdk_warp_perspective(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height,
                          int src_pitch, void* dst, int dst_width, int dst_height, int dst_pitch, const double* M,
                          int flags, int border, const double* border_value, void* stream);

/* tbdk_warp_perspective with the matrix in DEVICE memory, for a matrix an earlier call on the same
 * stream produced (&out[i].h[0] of tbdk_find_homography): no host round trip between the two.
 *   M     : device pointer to 9 doubles, 8-byte aligned; read when the kernel runs.  It is inverted
 *           on the device with tbdk_warp_perspective_invert's arithmetic, so for the same matrix
 *           the result is byte-identical to tbdk_warp_perspective
 *   valid : device int32 or NULL (&out[i].valid).  Where it reads 0, or an entry of M is not
 *           finite (tbdk_warp_perspective returns TBDK_EINVAL there; this call cannot know), dst
 *           is left untouched
 * Timing name "warp_perspective_dev". */
int tbdk_warp_perspective_dev(tbdk_ctx* ctx, const void* src, int pix, int cn, int src_width, int src_height,
                              int src_pitch, void* dst, int dst_width, int dst_height, int dst_pitch, const double* M,
                              const int32_t* valid, int flags, int border, const double* border_value, void* stream);

/* The host-side inverse tbdk_warp_perspective takes (cv::invert's 3x3 CV_64F branch), exported
 * for the tests; host only, needs no GPU */
int tbdk_warp_perspective_invert(const double* M, double* out);

/* ---- image front end: cvtColor, resize ------------------------------------- */

/* colour conversion codes: the reference's values (imgproc.hpp ColorConversionCodes) */
#define TBDK_COLOR_BGR2BGRA 0        /* alpha 255 */
#define TBDK_COLOR_BGR2GRAY 6
#define TBDK_COLOR_RGB2GRAY 7
#define TBDK_COLOR_GRAY2BGR 8
#define TBDK_COLOR_BGRA2GRAY 10
#define TBDK_COLOR_RGBA2GRAY 11

/* Replaces cv::cuda::cvtColor(src, dst, code) (cudaimgproc.hpp) for 8-bit
 * images and the codes above, with the bits of the CPU cv::cvtColor the sample
 * calls (samples/gpu/tbd.cpp:573-574): gray is RGB2Gray<uchar>
 * (imgproc/src/color_rgb.simd.hpp:647), (B*1868 + G*9617 + R*4899 + 8192) >> 14.
 *   src, dst : device u8 images of width x height pixels (interleaved channels,
 *              row pitch in bytes); dst must not alias src
 * TBDK_EINVAL for any other code. */
int tbdk_cvt_color_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, uint8_t* dst,
                      int dst_pitch, int code, void* stream);
/* Replaces cv::cuda::resize(src, dst, Size(dst_width, dst_height), 0, 0, INTER_LINEAR)
 * (cudawarping.hpp) for 8-bit images of cn = 1, 3 or 4 channels, bit-exact
 * with the CPU cv::resize of samples/gpu/tbd.cpp:578 (imgproc/src/resize.cpp:
 * 11-bit fixed-point coefficients; both scales exactly 2 is INTER_AREA,
 * equal sizes a copy).  The per-axis coefficient tables are made on the host
 * and cached in the context by (source, destination) size: a repeated size
 * allocates, uploads and waits for nothing.  A new size synchronises `stream`
 * once and uploads its tables; once the cache's 8 slots are taken it replaces
 * the least recently used size and waits for the whole device first, since
 * kernels of earlier calls, on any stream, may still read those tables: calls
 * of one context on different streams need no ordering by the caller.
 * dst must not alias src. */
int tbdk_resize_linear_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, int cn,
                          uint8_t* dst, int dst_width, int dst_height, int dst_pitch, void* stream);
/* tbdk_cvt_color_u8 (one of the four *2GRAY codes) followed by
 * tbdk_resize_linear_u8 of the gray image, in one pass with the same bits:
 * every source tap is converted to gray, then interpolated. */
int tbdk_cvt_resize_gray_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int src_pitch, int code,
                            uint8_t* dst, int dst_width, int dst_height, int dst_pitch, void* stream);

/* ---- dense Farneback optical flow ------------------------------------------ */

/* flag value of the reference (video/include/opencv2/video/tracking.hpp:58) */
#define TBDK_OPTFLOW_FARNEBACK_GAUSSIAN 256

/* cv::cuda::FarnebackOpticalFlow::create(numLevels, pyrScale, fastPyramids,
 * winSize, numIters, polyN, polySigma, flags)
 * (modules/cudaoptflow/include/opencv2/cudaoptflow.hpp:210-252) */
typedef struct tbdk_farneback_params {
    int32_t num_levels;              /* 5 */
    double pyr_scale;                /* 0.5; < 1 (CV_Assert, optflowgf.cpp:1113-1114) */
    int32_t fast_pyramids;           /* 0; the CUDA-only pyrDown pyramids are not provided (TBDK_EINVAL) */
    int32_t win_size;                /* 13; 1..21 */
    int32_t num_iters;               /* 10 */
    int32_t poly_n;                  /* 5; 1..15 */
    double poly_sigma;               /* 1.1 */
    int32_t flags;                   /* 0 | TBDK_OPTFLOW_FARNEBACK_GAUSSIAN | TBDK_OPTFLOW_USE_INITIAL_FLOW */
} tbdk_farneback_params;

int tbdk_farneback_default_params(tbdk_farneback_params* p);
/* level count and sizes calc uses for a width x height frame
 * (optflowgf.cpp:1125-1144): *nlevels = levels + 1, sizes[2*k] = width of level k,
 * sizes[2*k+1] = height (sizes may be NULL; else room for 2 * (num_levels + 1)) */
int tbdk_farneback_levels(int width, int height, const tbdk_farneback_params* p, int* nlevels, int32_t* sizes);

/* Replaces cv::cuda::FarnebackOpticalFlow::calc(I0, I1, flow, stream)
 * (cudaoptflow/src/farneback.cpp:164-196) with the numerics of the CPU
 * cv::calcOpticalFlowFarneback (video/src/optflowgf.cpp:1096-1190).
 *   prev, next : device u8 frames (width x height) sharing one row pitch in
 *                bytes: any pointers, any pitch >= width
 *   flow       : device CV_32FC2 output, interleaved (dx, dy) per pixel,
 *                8-byte aligned, flow_pitch in bytes (a multiple of 8, >=
 *                8 * width; bytes beyond a row are not written); with
 *                TBDK_OPTFLOW_USE_INITIAL_FLOW also the input: the coarsest
 *                level starts from its INTER_AREA resize times the level scale
 *                (optflowgf.cpp:1151-1157)
 * Scratch (15 float planes of the frame size + the blur buffer) is owned by
 * the context and grown on demand; the call is asynchronous on `stream`. */
int tbdk_farneback(tbdk_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width, int height, int pitch,
                   float* flow, int flow_pitch, const tbdk_farneback_params* params, void* stream);

/* Stage entry points of tbdk_farneback (parity tests):
 * level image = resize(GaussianBlur(float(img), (smooth_size, smooth_size), sigma),
 * (dst_width, dst_height), INTER_LINEAR) (optflowgf.cpp:1170-1172); img: any
 * pointer, pitch >= width; dst device float plane, dst_pitch in bytes (a
 * multiple of 4, >= 4 * dst_width). */
int tbdk_fb_level_image(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int dst_width,
                        int dst_height, int smooth_size, double sigma, float* dst, int dst_pitch, void* stream);
/* FarnebackPolyExp (optflowgf.cpp:116-202): src device float plane; dst = 5
 * device float planes (plane c at byte offset c * height * dst_pitch) holding
 * the reference's CV_32FC5 channels c = 0..4. */
int tbdk_fb_poly_exp(tbdk_ctx* ctx, const float* src, int width, int height, int src_pitch, int poly_n,
                     double poly_sigma, float* dst, int dst_pitch, void* stream);

/* ---- HOG people detector (cv::cuda::HOG / cv::HOGDescriptor) -------------- */

/* cv::cuda::HOG::create(win_size, block_size, block_stride, cell_size, nbins) and
 * its setters (cudaobjdetect/include/opencv2/cudaobjdetect.hpp:95-180, defaults of
 * cudaobjdetect/src/hog.cpp:230-250), computed with the CPU HOGDescriptor's
 * numerics (objdetect/src/hog.cpp) that the sample's CPU mode runs. */
typedef struct tbdk_hog_params {
    int32_t win_w, win_h;                   /* 64 x 128 (48 x 96: the Daimler detector) */
    int32_t block_w, block_h;               /* 16 x 16 */
    int32_t block_stride_x, block_stride_y; /* 8, 8 */
    int32_t cell_w, cell_h;                 /* 8, 8 */
    int32_t nbins;                          /* 9 (2..32) */
    double win_sigma;                       /* -1: (block_w + block_h) / 8 */
    double l2hys_threshold;                 /* 0.2 */
    int32_t gamma_correction;               /* 1 */
    int32_t signed_gradient;                /* 0 */
    int32_t nlevels;                        /* 64 */
    double hit_threshold;                   /* 0 */
    int32_t win_stride_x, win_stride_y;     /* 8, 8 (= block stride) */
    double scale0;                          /* 1.05 */
    int32_t group_threshold;                /* 2 */
} tbdk_hog_params;

int tbdk_hog_default_params(tbdk_hog_params* p);
/* descriptor length nbins * cells/block * blocks/window (HOGDescriptor::getDescriptorSize,
 * hog.cpp:87-99); an SVM detector has this many coefficients, or one more (the bias) */
int tbdk_hog_descriptor_size(const tbdk_hog_params* p, int* size);

/* Replaces cv::cuda::HOG::detectMultiScale(img, found_locations, confidences)
 * (cudaobjdetect/src/hog.cpp:415-470) with HOGDescriptor::detectMultiScale(img,
 * rects, weights, hit_threshold, win_stride, Size(), scale0, group_threshold)
 * (objdetect/src/hog.cpp:2051-2105), the CPU call of samples/gpu/tbd.cpp:603-605.
 *   img     : device u8 image, cn 1 (gray), 3 (BGR) or 4 (BGRA, alpha ignored);
 *             any pointer, any pitch >= width * cn (tbdk_hog_detect, _resize and
 *             _gradient alike)
 *   svm     : host float coefficients, svm_len = descriptor size (+ 1 bias)
 *   rects   : host int32 (x, y, w, h) x max_rects; weights: host double x max_rects
 *   nrects  : number of grouped, clipped detections (<= max_rects)
 * Synchronous: returns when the results are in the host buffers. */
int tbdk_hog_detect_multiscale(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int cn,
                               const tbdk_hog_params* params, const float* svm, int svm_len, int32_t* rects,
                               double* weights, int max_rects, int* nrects, void* stream);
/* One level, no resize and no grouping (HOGDescriptor::detect, hog.cpp:1655-1767):
 * window corners (x, y) and scores in window order; synchronous. */
int tbdk_hog_detect(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int cn,
                    const tbdk_hog_params* params, const float* svm, int svm_len, int32_t* xy, double* scores,
                    int max_hits, int* nhits, void* stream);
/* The HOG calls of one context share its scratch (cell table, level image,
 * gradients, hits). A call on a different stream than the context's previous HOG
 * call first synchronises that previous stream.
 * Stage entry points (parity tests).  resize(src, dst, (dw, dh), INTER_LINEAR_EXACT)
 * of a u8 image (imgproc/src/resize.cpp:732-891); dst: any pointer, dst_pitch >=
 * dst_width * cn, bytes beyond a row not written: */
int tbdk_hog_resize(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int pitch, int cn, uint8_t* dst,
                    int dst_width, int dst_height, int dst_pitch, void* stream);
/* HOGDescriptor::computeGradient (hog.cpp:239-550): grad = 2 floats per pixel
 * (grad_pitch bytes per row: a multiple of 8, >= 8 * width, grad 8-byte
 * aligned), qangle = 2 bytes per pixel (qangle_pitch: even, >= 2 * width,
 * qangle 2-byte aligned); bytes beyond a row are not written. */
int tbdk_hog_gradient(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int cn,
                      const tbdk_hog_params* params, float* grad, int grad_pitch, uint8_t* qangle,
                      int qangle_pitch, void* stream);
/* normalized block histograms (HOGCache::getBlock + normalizeBlockHistogram,
 * hog.cpp:860-1248) at every block position of the gcd(win stride, block stride)
 * grid: blocks[(by * nbx + bx) * hist_size + k], hist_size = nbins * cells/block. */
int tbdk_hog_blocks(tbdk_ctx* ctx, const float* grad, int grad_pitch, const uint8_t* qangle, int qangle_pitch,
                    int width, int height, const tbdk_hog_params* params, float* blocks, void* stream);

/* ---- tracking-by-detection loop (one video stream per context) ------------ */

/* Per-stream TBD loop: pyramid -> (GFTT on new / re-detect tracks) -> PyrLK over
 * every track's corners -> per-track similarity fit (KLT box propagation, the
 * Track::motionModel hook of modules/trackingbydetection/include/opencv2/tbd.hpp:111)
 * -> cv::tbd::Tracker::performTrackingStep (modules/trackingbydetection/src/tbd.cpp:210-286)
 * restated natively.  Replaces the tracking section of samples/gpu/tbd.cpp:624-706. */
typedef struct tbdk_tbd tbdk_tbd;

/* Accepted ranges (tbdk_tbd_create returns TBDK_EINVAL outside them and
 * creates nothing):
 *   width, height          > 0
 *   win                    3..31; odd 7..31 run the several-points-per-wave
 *                          PyrLK kernel, the others the generic one
 *   max_level              >= 0; levels stop early on a frame too small for
 *                          them (cv::buildOpticalFlowPyramid's rule)
 *   lk_iters, lk_epsilon   any; used as min(max(lk_iters, 0), 100) and
 *                          min(max(lk_epsilon, 0), 10) (lkpyramid.cpp:1332-1339)
 *   min_eig_threshold      any (a point whose minimum eigenvalue is below it is lost)
 *   max_corners            1..256
 *   quality_level          > 0, finite
 *   min_distance           >= 0, finite
 *   redetect_every         >= 1
 *   min_points, min_fit_points  any (a set with fewer points left is
 *                          refreshed / gives no prediction)
 *   time_window_size       1..64
 *   max_tracks             >= 1 */
typedef struct tbdk_tbd_config {
    int32_t width, height;
    /* PyrLK (cv::calcOpticalFlowPyrLK defaults except maxLevel: "3-level" = 2) */
    int32_t win, max_level, lk_iters;
    double lk_epsilon;
    float min_eig_threshold;
    /* GFTT per track box */
    int32_t max_corners;             /* <= 256 */
    double quality_level, min_distance;
    int32_t redetect_every;          /* re-detect corners every N frames (5) */
    int32_t min_points;              /* ... or when fewer points survive (32) */
    int32_t min_fit_points;          /* points needed for the box fit (4) */
    /* cv::tbd::TbdArgs (samples/gpu/tbd.cpp:249-254 defaults) */
    double cost_of_non_assignment;
    int32_t time_window_size, track_age_threshold;
    double track_visibility_threshold, track_confidence_threshold;
    /* filterTracksOutOfBounds window; the reference hard-codes 0,1280,0,720 */
    int32_t bounds_xmin, bounds_xmax, bounds_ymin, bounds_ymax;
    int32_t max_tracks;              /* point-set slots on the device */
    int32_t use_klt;                 /* 0: reference constant-velocity prediction only */
} tbdk_tbd_config;

typedef struct tbdk_detection {      /* cv::tbd::Detection (tbd.hpp:69-83) */
    int32_t id, x, y, width, height;
    double confidence;
} tbdk_detection;

typedef struct tbdk_frame_metrics {  /* per-frame TP/FN/FP/GT/c/sum d (tbd.hpp:145-151) */
    int32_t tp, fn, fp, gt, matches;
    double bbox_overlap;
    int32_t ntracks;
    int32_t lk_points;               /* corners that entered PyrLK this frame */
    int32_t klt_points;              /* ... of which tracked (status 1) */
    int32_t klt_predicted;           /* tracks predicted by the KLT fit */
    int32_t redetected;              /* point sets refreshed by GFTT this frame */
    int32_t early_gftt;              /* ... of which served by the early GFTT (tbd_loop.hip) */
    int64_t lk_iters;                /* Newton iterations over all levels (flop accounting) */
    float host_wait_us;              /* host time blocked on the device this step */
    float host_tracker_us;           /* host time in the tracker step (assignment + bookkeeping) */
    float host_step_us;              /* host time in tbdk_tbd_step, end to end */
    float host_launch_us;            /* host time issuing the pyramid / LK / fit work (before the sync) */
} tbdk_frame_metrics;

typedef struct tbdk_track_info {
    uint32_t id;
    int32_t x, y, width, height;             /* last box */
    int32_t pred_x, pred_y, pred_w, pred_h;  /* predPosition */
    int32_t age, total_visible;
    int32_t npoints;                         /* tracked corners after this frame */
    double max_confidence, bbox_overlap;
} tbdk_track_info;

/* ---- the tracker alone (host only; no device, no context) ------------------
 * cv::tbd::Tracker (modules/trackingbydetection/include/opencv2/tbd.hpp:119-184,
 * src/tbd.cpp:182-1106) as a drop-in: performTrackingStep with an optional
 * per-track predicted centroid that replaces Track::motionModel (tbd.hpp:111)
 * for the tracks it names (the KLT box-propagation hook). */
typedef struct tbdk_tracker tbdk_tracker;

typedef struct tbdk_tracker_args {   /* cv::tbd::TbdArgs (tbd.hpp:25-41) + the bounds filter */
    double cost_of_non_assignment;
    int32_t time_window_size, track_age_threshold;   /* time_window_size <= 64 */
    double track_visibility_threshold, track_confidence_threshold;
    int32_t bounds_xmin, bounds_xmax, bounds_ymin, bounds_ymax;  /* reference: 0,1280,0,720 */
} tbdk_tracker_args;

typedef struct tbdk_prediction {
    uint32_t track_id;
    int32_t valid;                   /* 0: ignored (motion model used) */
    double cx, cy;                   /* predicted box centre */
} tbdk_prediction;

/* defaults of samples/gpu/tbd.cpp:249-254 and the hard-coded filter (tbd.cpp:218) */
int tbdk_tracker_default_args(tbdk_tracker_args* args);
int tbdk_tracker_create(const tbdk_tracker_args* args, tbdk_tracker** out);
int tbdk_tracker_destroy(tbdk_tracker* t);
/* Tracker::performTrackingStep (tbd.cpp:210-286); metrics: tp, fn, fp, gt,
 * matches, bbox_overlap and ntracks are filled, the KLT fields are 0. */
int tbdk_tracker_step(tbdk_tracker* t, const tbdk_detection* dets, int ndets, int frame_id,
                      const tbdk_prediction* preds, int npreds, tbdk_frame_metrics* metrics);
/* current tracks in the tracker's order (npoints = 0); *n = number of tracks */
int tbdk_tracker_tracks(const tbdk_tracker* t, tbdk_track_info* out, int cap, int* n);

/* ---- the sample's tracking driver (host only) -------------------------------
 * samples/gpu/tbd.cpp feeds the tracker ground-truth or external detections
 * from bbox files and writes MOT metrics.  Restated natively (tbd_app.cpp). */

/* Tracker::reset (tbd.cpp:197-208) */
int tbdk_tracker_reset(tbdk_tracker* t);
/* tbdk_tracker_step that also records the tracking result of every detection
 * carrying a ground-truth id into `traj` (performTrackingStep's trajectoryMap
 * argument, tbd.cpp:236-265); traj may be NULL. */
typedef struct tbdk_trajectories tbdk_trajectories;
int tbdk_tracker_step_traj(tbdk_tracker* t, const tbdk_detection* dets, int ndets, int frame_id,
                           const tbdk_prediction* preds, int npreds, tbdk_trajectories* traj,
                           tbdk_frame_metrics* metrics);

/* glibc rand() restated with private state (srand(seed); the sample's rand()
 * is never seeded = seed 1).  Attached to a tracker, each new track draws its
 * display colour from it (3 calls, tbd.cpp:71-73), as the reference does from
 * the global rand(); the sample's history draw shares the sequence. */
typedef struct tbdk_rand tbdk_rand;
int tbdk_rand_create(uint32_t seed, tbdk_rand** out);
int tbdk_rand_destroy(tbdk_rand* r);
int tbdk_rand_next(tbdk_rand* r, int32_t* out);
int tbdk_tracker_set_rand(tbdk_tracker* t, tbdk_rand* r);   /* r NULL: colours not drawn */
/* Args::parseHistoryDistribution (samples/gpu/tbd.cpp:258-291): "7,3" -> normalised floats */
int tbdk_parse_history_distribution(const char* s, float* out, int cap, int* n);
/* one history-age draw (samples/gpu/tbd.cpp:656-671): 1 + index of the first
 * cumulative float weight above rand()/RAND_MAX, else n */
int tbdk_history_age(tbdk_rand* r, const float* dist, int n, uint32_t* age);

/* Parsed bbox files (parseBboxFile, samples/gpu/tbd.cpp:1163-1295): per class
 * (0 pedestrians, 1 vehicles) the per-frame rows of one file; camera poses
 * (object id -1 rows) and a "history|a,b,..." line shared, as in the sample.
 * Lines "frame|id|x1|x2|y1|y2[|wx|wy[|wz]]" are ground truth (more than four
 * separators, frames offset by the first frame number), "frame|x1|x2|y1|y2"
 * external detections (id -2, frames from 0). */
typedef struct tbdk_sequence tbdk_sequence;
int tbdk_sequence_create(tbdk_sequence** out);
int tbdk_sequence_destroy(tbdk_sequence* s);
/* TBDK_EINVAL where the sample's stoi/stoul/stod throw (message: tbdk_sequence_error) */
int tbdk_sequence_parse_bbox_file(tbdk_sequence* s, int cls, const char* path, uint32_t num_frames);
const char* tbdk_sequence_error(const tbdk_sequence* s);
int tbdk_sequence_info(const tbdk_sequence* s, int cls, int32_t* nframes, int32_t* nposes, int32_t* nhistory);
int tbdk_sequence_history(const tbdk_sequence* s, uint32_t* out, int cap, int* n);
int tbdk_sequence_camera_pose(const tbdk_sequence* s, int index, double* out, int cap, int* n);
/* parseDetections (samples/gpu/tbd.cpp:1297-1340): frame `frame`'s detections
 * (confidence 1.0); ground-truth rows also add their position to traj (may be NULL) */
int tbdk_sequence_detections(const tbdk_sequence* s, int cls, int frame, tbdk_trajectories* traj,
                             tbdk_detection* out, int cap, int* n);

/* std::map<int, Trajectory> (tbd.hpp:46-80) */
int tbdk_trajectories_create(tbdk_trajectories** out);
int tbdk_trajectories_destroy(tbdk_trajectories* t);
int tbdk_trajectories_add_position(tbdk_trajectories* t, int id, int frame, int x, int y, int w, int h);
int tbdk_trajectories_count(const tbdk_trajectories* t, int* n);

/* the sample's per-history-age output buffers of tracks (samples/gpu/tbd.cpp:524-531, 679-704):
 * store = buffer[slot] = getTracks(); load = setTracks(buffer[slot]) (slot < 0: empty) */
typedef struct tbdk_track_buffer tbdk_track_buffer;
int tbdk_track_buffer_create(int nslots, tbdk_track_buffer** out);
int tbdk_track_buffer_destroy(tbdk_track_buffer* b);
int tbdk_tracker_store_tracks(tbdk_tracker* t, tbdk_track_buffer* b, int slot);
int tbdk_tracker_load_tracks(tbdk_tracker* t, const tbdk_track_buffer* b, int slot);

typedef struct tbdk_scenario_metrics {  /* the "scenario|" line + totals */
    int32_t mt, pt, ml;              /* mostly tracked / partially / mostly lost trajectories */
    int32_t idsw, fm;                /* ID switches, fragmentations (sums) */
    int32_t frames;                  /* "frame|" lines */
    double mota, amota, motp;
} tbdk_scenario_metrics;

/* App::writeTrackingOutputToFile (samples/gpu/tbd.cpp:946-1120): appends the
 * history / object / frame / scenario lines to `path` (NULL or "": metrics
 * only).  frame_count = frames processed; log_switches prints the sample's
 * "[frame f] target ... switched" lines to stdout. */
int tbdk_tracking_write(const tbdk_tracker* t, const uint32_t* history_ages, int nages, int frame_count,
                        tbdk_trajectories* traj, const char* path, int log_switches, tbdk_scenario_metrics* out);

typedef struct tbdk_app_args {       /* the sample's tracking flags (samples/gpu/tbd.cpp:221-257, 293-331) */
    const char* pedestrian_bbox_filename;
    const char* vehicle_bbox_filename;
    const char* pedestrian_tracking_filepath;
    const char* vehicle_tracking_filepath;
    const char* history_distribution;   /* "--history_distribution", NULL = "1" */
    int32_t write_tracking;
    int32_t num_tracking_iters;         /* 1 */
    int32_t num_tracking_frames;        /* 100 */
    uint32_t rand_seed;                 /* 1 = the sample's unseeded rand() */
    int32_t verbose;                    /* print ID-switch lines / errors to stdout */
    tbdk_tracker_args tracker;          /* TbdArgs defaults (samples/gpu/tbd.cpp:249-254) */
} tbdk_app_args;

typedef struct tbdk_app_result {
    int64_t frames, detections;         /* over all iterations */
    tbdk_scenario_metrics scenario[2];  /* last iteration, pedestrians / vehicles */
} tbdk_app_result;

int tbdk_app_default_args(tbdk_app_args* args);
/* App::run's tracking loop (samples/gpu/tbd.cpp:479-706, 823-841) over the
 * bbox files: history-age draw, setTracks from the output buffer,
 * performTrackingStep per class, tracking output per iteration. */
int tbdk_app_run(const tbdk_app_args* args, tbdk_app_result* result);

int tbdk_tbd_default_config(int width, int height, tbdk_tbd_config* cfg);
/* Loops on one context share the context's three side streams (post-tracker
 * GFTT, look-ahead PyrLK, early GFTT), created by its first loop: loops
 * stepped concurrently from different host threads on one context serialise
 * their off-critical work on them, and tbdk_tbd_destroy / tbdk_tbd_tracks
 * synchronise those streams, so they also wait for the other loops' work.
 * Use one context per concurrently stepped loop (the bench runs one loop per
 * GPU and process), and destroy every loop before its context. */
int tbdk_tbd_create(tbdk_ctx* ctx, const tbdk_tbd_config* cfg, tbdk_tbd** out);
int tbdk_tbd_destroy(tbdk_tbd* tbd);
/* A static corner mask for the loop's GFTT launches (tbdk_gftt_rois_masked's
 * semantics): a device u8 plane of the loop's frame size (cfg.width x
 * cfg.height), rows mask_pitch bytes apart, which the caller keeps alive and
 * unchanged for the loop's life.  NULL clears it.  Only before the loop's
 * first step: afterwards TBDK_EINVAL, because the GFTT launched a frame ahead
 * would have run under the old mask.  TBDK_EINVAL also for mask_pitch < width. */
int tbdk_tbd_set_corner_mask(tbdk_tbd* tbd, const uint8_t* mask, int mask_pitch);
/* One frame through the loop.  frame: device u8 (width x height, pitch);
 * dets: HOST array.  Synchronises the stream once (predictions -> host tracker). */
int tbdk_tbd_step(tbdk_tbd* tbd, const uint8_t* frame, int pitch, int frame_id, const tbdk_detection* dets,
                  int ndets, tbdk_frame_metrics* metrics, void* stream);
/* tbdk_tbd_step when the next frame is already on the device (a decode
 * pipeline, or a clip): the next frame's pyramid is enqueued behind this
 * frame's fit (the device builds it while the host tracks), and the next
 * frame's PyrLK of every point set this step leaves unchanged behind the
 * post-tracker GFTT, without returning to the caller in between.
 * next_frame must keep its pixels until the next step, which must pass the
 * same pointer, pitch and stream to use that work (otherwise it is redone).
 * Per-frame results are identical to tbdk_tbd_step's. */
int tbdk_tbd_step_ahead(tbdk_tbd* tbd, const uint8_t* frame, int pitch, int frame_id, const tbdk_detection* dets,
                        int ndets, const uint8_t* next_frame, int next_pitch, tbdk_frame_metrics* metrics,
                        void* stream);
/* The loop of samples/gpu/tbd.cpp:624-706 over nframes resident frames:
 * frames = host array of device pointers (same pitch), frame ids
 * first_frame_id + i, frame i's detections dets[det_offsets[i] ..
 * det_offsets[i+1]) (host), metrics = nframes entries or NULL.  Equivalent to
 * tbdk_tbd_step_ahead over the sequence. */
int tbdk_tbd_run(tbdk_tbd* tbd, const uint8_t* const* frames, int pitch, int first_frame_id,
                 const tbdk_detection* dets, const int32_t* det_offsets, int nframes, tbdk_frame_metrics* metrics,
                 void* stream);
/* tbdk_tbd_run over frames in HOST memory (the sample's frame source,
 * samples/gpu/tbd.cpp:568-599: a decoded frame is uploaded, then processed):
 * frames = host pointers (same pitch; page-locked memory lets the uploads
 * overlap the loop).  Each frame is uploaded into a ring of three device
 * frames on a copy stream two frames ahead of its use, so frame i+2's upload
 * runs during frame i's work; results are identical to tbdk_tbd_run's. */
int tbdk_tbd_run_host(tbdk_tbd* tbd, const uint8_t* const* frames, int pitch, int first_frame_id,
                      const tbdk_detection* dets, const int32_t* det_offsets, int nframes,
                      tbdk_frame_metrics* metrics, void* stream);
int tbdk_tbd_tracks(tbdk_tbd* tbd, tbdk_track_info* out, int cap, int* n);
/* Attach a trajectory map (NULL detaches): every later step records, for each
 * detection with a ground-truth id (id >= 0), its position (parseDetections,
 * samples/gpu/tbd.cpp:1327-1338) and its tracking result (tbd.cpp:236-265). */
int tbdk_tbd_set_trajectories(tbdk_tbd* tbd, tbdk_trajectories* traj);
/* tbdk_tracking_write for the loop's tracker and attached trajectories */
int tbdk_tbd_tracking_write(tbdk_tbd* tbd, const uint32_t* history_ages, int nages, int frame_count,
                            const char* path, int log_switches, tbdk_scenario_metrics* out);
/* The KLT predictions the last tbdk_tbd_step handed to the tracker (one per
 * track with a valid box fit, in track order); *n = their number. */
int tbdk_tbd_predictions(const tbdk_tbd* tbd, tbdk_prediction* out, int cap, int* n);

/* ---- detection-driven step: colour frame in, HOG detections, tracks out ----
 * The per-frame path of samples/gpu/tbd.cpp:568-622 in front of the loop:
 * cvtColor -> optional resize -> HOG detectMultiScale -> one Detection per
 * rect -> tbdk_tbd_step. */
typedef struct tbdk_tbd_detector tbdk_tbd_detector;

typedef struct tbdk_tbd_detect_config {
    int32_t width, height;           /* the loop's frame size: its tbdk_tbd_config width x height */
    int32_t src_width, src_height;   /* the colour frames handed to tbdk_tbd_step_image */
    int32_t src_cn;                  /* 3 or 4 (alpha ignored) */
    int32_t rgb_order;               /* 0: BGR(A) (the sample's frames), 1: RGB(A) */
    int32_t make_gray;               /* 1: HOG runs on the gray image (the sample's default); 0: on the colour image */
    int32_t resize;                  /* 1: resize to width x height (--resize_src); 0: the sizes must be equal */
    int32_t confidence_mode;         /* 0: every detection's confidence is -1.0, as the sample's (tbd.cpp:619);
                                        1: the HOG weight of the grouped rect (the sample's TODO) */
    int32_t max_detections;          /* per frame; more is TBDK_ENOMEM */
    tbdk_hog_params hog;
} tbdk_tbd_detect_config;

/* the sample's settings (samples/gpu/tbd.cpp:436-443: 15 levels, hit threshold
 * 0.45, the detector's other defaults), gray, no resize, BGR frames of the
 * loop's size, confidence -1.0, 4096 detections */
int tbdk_tbd_detect_default_config(int width, int height, tbdk_tbd_detect_config* cfg);
/* ctx: the context `tbd` was created on; svm: host coefficients (descriptor
 * size, or one more for the bias), copied.  The detector owns the working
 * images (the gray frame; with make_gray = 0 the resized colour frame too).
 * Destroy it before the loop. */
int tbdk_tbd_detector_create(tbdk_ctx* ctx, tbdk_tbd* tbd, const tbdk_tbd_detect_config* cfg, const float* svm,
                             int svm_len, tbdk_tbd_detector** out);
int tbdk_tbd_detector_destroy(tbdk_tbd_detector* det);
/* One colour frame (device u8, src_width x src_height x src_cn, pitch bytes):
 *   1. make_gray = 1: cvtColor(*2GRAY) -> resize (one fused pass when both apply);
 *      make_gray = 0: the colour image is resized, HOG runs on it, and the loop's
 *      frame is its *2GRAY conversion;
 *   2. detectMultiScale (tbdk_hog_detect_multiscale) with cfg.hog;
 *   3. rect i becomes {id -1, rect, confidence by mode}, in the reference's
 *      output order: levels ascending, windows row-major within a level, then
 *      groupRectangles' class order (track ids and assignment ties depend on it);
 *   4. tbdk_tbd_step on the gray frame with those detections.
 * dets_out (host, cap entries; may be NULL with cap 0) receives the detections
 * used, *ndets their number (all of them are used even when cap is smaller).
 * Synchronous, as HOG is. */
int tbdk_tbd_step_image(tbdk_tbd_detector* det, const uint8_t* frame, int pitch, int frame_id,
                        tbdk_detection* dets_out, int cap, int* ndets, tbdk_frame_metrics* metrics, void* stream);

/* The sample's loop over an image sequence with no bbox file
 * (samples/gpu/tbd.cpp:568-706 with HOG detections).  image_list_filename: a
 * text file with one path per line (relative paths: to the list's directory)
 * of binary PNM frames, P6 (BGR order is NOT assumed: P6 is RGB) or P5 gray,
 * maxval 255, all of one size. */
typedef struct tbdk_app_image_args {
    const char* image_list_filename;
    const char* tracking_filepath;      /* the history|object|frame|scenario output (NULL or "": none) */
    int32_t num_tracking_frames;        /* 100 */
    int32_t make_gray;                  /* 1 */
    int32_t resize_src, width, height;  /* 0, 640 x 480 (--resize_src, --width, --height) */
    int32_t confidence_mode;            /* tbdk_tbd_detect_config.confidence_mode */
    int32_t device;                     /* 0 */
    int32_t verbose;
    tbdk_hog_params hog;                /* the sample's settings */
    const float* svm;                   /* HOST detector coefficients */
    int32_t svm_len;
    tbdk_tracker_args tracker;          /* TbdArgs defaults; the bounds filter */
} tbdk_app_image_args;

typedef struct tbdk_app_image_result {
    int64_t frames, detections;
    tbdk_scenario_metrics scenario;
} tbdk_app_image_result;

int tbdk_app_image_default_args(tbdk_app_image_args* args);
/* Every listed file is opened and its header checked before any GPU work: a
 * missing or malformed file is TBDK_EINVAL with nothing run. */
int tbdk_app_run_images(const tbdk_app_image_args* args, tbdk_app_image_result* result);

/* ---- KLT point tracker (the reference samples' lk_track loop) --------------
 * samples/python/lk_track.py App.run (lines 48-86, minus the drawing) with
 * samples/cpp/lkdemo.cpp's cornerSubPix (:84-85) and click-to-add: a long-lived,
 * ordered set of point tracks that is tracked, pruned, masked and topped up
 * frame after frame, entirely in device memory.  A step only enqueues work on
 * the caller's stream: the host never reads the live count.
 *
 * Per step(frame):
 *   1. the frame's pyramid is built;
 *   2. with a previous frame, every track's last position is tracked prev -> cur
 *      with tbdk_lk_sparse_fb's forward-backward check (both statuses gate and
 *      max(|dx|, |dy|) < back_threshold in float32; lk_track.py:57-60 ignores
 *      the statuses, the tracker does not).  Tracks that fail are removed, the
 *      survivors keep their order, get the new position appended and drop their
 *      oldest one beyond track_len;
 *   3. if frame_idx % detect_interval == 0 or TBDK_KLT_DETECT_NOW: the mask is
 *      255 with a filled circle of mask_radius zeroed at ((int)x, (int)y) of
 *      every live track's last position (casts toward zero; the shape of
 *      cv::circle(mask, c, r, 0, -1), clipped; mask_radius < 0: no mask);
 *      goodFeaturesToTrack(frame, max_corners, quality_level, min_distance, mask,
 *      block_size, use_harris, harris_k) on the whole frame; with subpix_win > 0
 *      cornerSubPix((win, win), (-1, -1), COUNT|EPS 20, 0.03) on its corners;
 *      every corner, in goodFeaturesToTrack's order, starts a track of length 1
 *      with the next id (0, 1, 2, ... in creation order).  Beyond max_tracks the
 *      strongest corners that fit are appended, the others counted as dropped;
 *   4. frame_idx++, cur becomes prev.
 * Frames are 8-bit, one channel. */
typedef struct tbdk_klt_tracker tbdk_klt_tracker;

typedef struct tbdk_klt_tracker_config {
    int32_t width, height;
    int32_t win, max_level, lk_iters;       /* PyrLK: window side, levels, criteria COUNT */
    double  lk_epsilon;                     /* ... and EPS */
    float   min_eig_threshold;
    float   back_threshold;                 /* the check's distance bound, > 0 */
    int32_t max_corners;                    /* goodFeaturesToTrack */
    double  quality_level, min_distance;
    int32_t block_size, use_harris;
    double  harris_k;
    int32_t detect_interval;                /* detection on frames 0, N, 2N, ... */
    int32_t track_len;                      /* positions kept per track, 1..64 */
    int32_t mask_radius;                    /* 0..64; < 0: detection without a mask */
    int32_t subpix_win;                     /* cornerSubPix half window 1..15; 0: off */
    int32_t max_tracks;                     /* capacity, 1..65536 */
} tbdk_klt_tracker_config;

/* statistics of the last step (plus the tbdk_klt_tracker_add_points calls since) */
typedef struct tbdk_klt_tracker_stats {
    int32_t tracks_in;   /* live tracks when the step began */
    int32_t kept;        /* ... that passed the check (= tracks_in on the first frame) */
    int32_t detected;    /* corners goodFeaturesToTrack returned (0 without detection) */
    int32_t appended;    /* new tracks, detected or added */
    int32_t dropped;     /* corners / added points beyond max_tracks */
    int32_t next_id;     /* the id the next new track gets */
    int32_t frame_idx;   /* index of the step's frame (-1 before the first step) */
} tbdk_klt_tracker_stats;

#define TBDK_KLT_DETECT_NOW 1

/* lk_track.py's parameters: win 15, max_level 2, criteria (10, 0.03),
 * min_eig_threshold 1e-4, back_threshold 1; goodFeaturesToTrack (500, 0.3, 7,
 * blockSize 7); detect_interval 5, track_len 10, mask_radius 5; subpix_win 0;
 * max_tracks 8192 */
int tbdk_klt_tracker_default_config(int width, int height, tbdk_klt_tracker_config* cfg);
/* Allocates everything a step needs (two pyramids, the two copies of the track
 * state, the mask plane, the detector's output row and GFTT scratch of its own),
 * so that steps allocate nothing.  TBDK_EINVAL: whatever tbdk_lk_sparse_fb,
 * tbdk_gftt_rois_masked and tbdk_corner_sub_pix refuse for these parameters;
 * track_len outside 1..64; detect_interval < 1; mask_radius > 64; subpix_win
 * below 0; max_corners > max_tracks; max_tracks outside 1..65536. */
int tbdk_klt_tracker_create(tbdk_ctx* ctx, const tbdk_klt_tracker_config* cfg, tbdk_klt_tracker** out);
int tbdk_klt_tracker_destroy(tbdk_klt_tracker* tr);
/* Empties the tracker: no tracks, ids from 0, frame_idx 0, no previous frame.
 * Waits for the last step's stream. */
int tbdk_klt_tracker_reset(tbdk_klt_tracker* tr);
/* One frame (device, 8-bit one channel, pitch in bytes, read until the enqueued
 * work is done).  flags: 0 or TBDK_KLT_DETECT_NOW.  TBDK_EINVAL (nothing
 * enqueued, state unchanged): a null frame, pitch < width, unknown flags.
 * Steps, add_points and reads of one tracker belong on one stream: a step on
 * another stream than the previous one's without synchronising in between is
 * the caller's error.  Timed as "pyr_build", "lk_sparse", "lk_sparse_back",
 * "gftt", "gftt_wide", "corner_sub_pix" and the tracker's own "klt_compact",
 * "klt_mask", "klt_append". */
int tbdk_klt_tracker_step(tbdk_klt_tracker* tr, const uint8_t* frame, int pitch, int flags, void* stream);
/* Appends n caller-supplied points (device, n x float2) as new tracks of length
 * 1 under the capacity rule of detection (lkdemo's click-to-add; seeding from
 * one's own detector).  The points are read when the stream gets there. */
int tbdk_klt_tracker_add_points(tbdk_klt_tracker* tr, const float* device_pts, int n, void* stream);
/* HOST outputs, any may be NULL: the live tracks in order, the first
 * min(*n, cap) of them: ids, last_pts (float2), lens, hist (track_len float2
 * per track, oldest first, zero beyond the track's length); *n: the live count;
 * *stats: see above.  Synchronises the stream of the last step. */
int tbdk_klt_tracker_read(tbdk_klt_tracker* tr, int32_t* ids, float* last_pts, int32_t* lens, float* hist, int cap,
                          int* n, tbdk_klt_tracker_stats* stats);
/* The device pointers of the state, for consumers that stay on the GPU (any may
 * be NULL): count (one int32), ids, last_pts, lens and hist as in
 * tbdk_klt_tracker_read, max_tracks entries each.  Valid until the next step;
 * read them on the step's stream or after synchronising it. */
int tbdk_klt_tracker_device_state(tbdk_klt_tracker* tr, const int32_t** count, const int32_t** ids,
                                  const float** last_pts, const int32_t** lens, const float** hist);
/* The tracker's detection mask on its own: writes `value` into the filled circle
 * of `radius` (0..64) around ((int)x, (int)y) of each of the first
 * min(*count_dev, n) points (count_dev NULL: n) and leaves the rest of the mask
 * alone.  mask: device u8, width x height, pitch in bytes; pts: device, n x
 * float2; count_dev: device int32 or NULL.  The circle is the one
 * cv::circle(mask, c, radius, value, -1) draws (imgproc/src/drawing.cpp:1486-1628),
 * clipped to the mask; centres may lie anywhere, a point that is not finite or
 * beyond +-1e9 draws nothing.  Timed as "klt_mask". */
int tbdk_mask_circles_u8(tbdk_ctx* ctx, uint8_t* mask, int width, int height, int pitch, const float* pts,
                         const int32_t* count_dev, int n, int radius, int value, void* stream);

/* ---- background subtraction ------------------------------------------------ */

/* cv::BackgroundSubtractorMOG2 (video/src/bgfg_gaussmix2.cpp) with its model resident on the
 * device: per pixel up to `nmixtures` Gaussian modes (weight, variance, mean per channel) and
 * the count of modes in use.  One kernel per frame classifies every pixel and updates its
 * model in place, with the reference's scalar float arithmetic operation for operation: the
 * mask, the background image and the model are the reference's bit for bit.
 * Frames: TBDK_DEPTH_8U or TBDK_DEPTH_32F, 1 or 3 channels, pitched, any alignment (32F: pointer
 * and pitch multiples of 4). */
typedef struct tbdk_mog2 tbdk_mog2;

typedef struct tbdk_mog2_config {
    int32_t width, height, depth, channels;  /* fixed at creation */
    int32_t history;                /* 500 */
    int32_t nmixtures;              /* 5; 1..8, fixed at creation */
    int32_t detect_shadows;         /* 1 */
    int32_t shadow_value;           /* 127; 0..255 */
    double  var_threshold;          /* 16 (Tb; the reference holds it as a double) */
    float   var_threshold_gen;      /* 9 (Tg) */
    float   var_init, var_min, var_max;  /* 15, 4, 75; the smaller of var_min / var_max is the lower clamp */
    float   background_ratio;       /* 0.9 (TB) */
    float   complexity_reduction;   /* 0.05 (CT) */
    float   shadow_threshold;       /* 0.5 (tau) */
    int32_t reserved;               /* 0 */
} tbdk_mog2_config;

/* the reference's defaults for a frame of this size and type */
int tbdk_mog2_config_default(int width, int height, int depth, int channels, tbdk_mog2_config* cfg);
/* Allocates the model (nothing is allocated afterwards).  TBDK_EINVAL: a depth other than 8U / 32F,
 * channels other than 1 / 3, nmixtures outside 1..8, width or height outside 1..65535, history < 1,
 * shadow_value outside 0..255. */
int tbdk_mog2_create(tbdk_ctx* ctx, const tbdk_mog2_config* cfg, tbdk_mog2** out);
int tbdk_mog2_destroy(tbdk_mog2* m);
/* The next apply starts from an empty model (frames() becomes 0).  No device work. */
int tbdk_mog2_reset(tbdk_mog2* m);
/* The reference's setters, all at once: takes every field of cfg but the fixed ones, which must
 * equal the object's (TBDK_EINVAL otherwise, nothing changed).  Holds from the next apply on. */
int tbdk_mog2_set_params(tbdk_mog2* m, const tbdk_mog2_config* cfg);
/* apply(frame, fgmask, learningRate): fgmask (device, 8-bit, width x height, mask_pitch bytes a
 * row) gets 0 (background), shadow_value (shadow) or 255 per pixel, and the model is updated.
 * The schedule is the reference's, kept on the host: the model is cleared (on the stream) on the
 * first call, after tbdk_mog2_reset and when learning_rate >= 1; the frame count is then
 * incremented, and the rate is learning_rate if it is >= 0 and this is not the first frame, else
 * 1 / min(2 * frames, history).  Asynchronous on `stream`, no allocation, no host
 * synchronisation; calls on one object are ordered by the caller's stream(s).  TBDK_EINVAL
 * (nothing enqueued, nothing changed): a null pointer, a pitch below a row, a 32F frame whose
 * pointer or pitch is no multiple of 4, a learning rate that is NaN.  Timed as "mog2_apply". */
int tbdk_mog2_apply(tbdk_mog2* m, const void* frame, int pitch, uint8_t* fgmask, int mask_pitch,
                    double learning_rate, void* stream);
/* getBackgroundImage: the weighted mean of each pixel's background modes, in the frame's type
 * (8-bit: rounded half to even and clamped), 0 where a pixel has no mode.  img: device, pitch in
 * bytes (32F: as for the frame).  Timed as "mog2_background". */
int tbdk_mog2_get_background(tbdk_mog2* m, void* img, int pitch, void* stream);
/* The model in the reference's layout, for tests and checkpoints (device pointers, any may be
 * NULL): weight[h][w][K], variance[h][w][K], mean[h][w][K][channels] (float32) and
 * modes_used[h][w] (uint8), K = nmixtures, all tight.  Modes at and above modes_used hold
 * whatever they last held, as in the reference.  Timed as "mog2_model". */
int tbdk_mog2_get_model(tbdk_mog2* m, float* weight, float* variance, float* mean, uint8_t* modes_used,
                        void* stream);
/* frames applied since the model was last cleared */
int tbdk_mog2_frames(tbdk_mog2* m, int* nframes);

/* cv::BackgroundSubtractorKNN, the CPU class of video/src/bgfg_KNN.cpp (not its OpenCL twin, whose
 * samples are floats), with its model resident on the device: per pixel 3 * nsamples samples of
 * `channels` bytes and an include flag in three circular lists (short, mid, long), an index byte
 * and a "next update" byte per list.  One kernel per frame classifies every pixel and updates its
 * model; the next-update planes are redrawn on the device by cv::randu's own generator, with the
 * reference's sequence and its count of consumed steps (blocks of 1024 values, started by
 * jump-ahead).  Mask, background image, model, counters and RNG state are the reference's bit for
 * bit.  Frames: 8-bit, 1 or 3 channels, pitched, any alignment.  The reference reads a frame of
 * another depth as raw bytes; that is not reproduced, and neither are four channels. */
typedef struct tbdk_knn tbdk_knn;

typedef struct tbdk_knn_config {
    int32_t width, height, channels;  /* fixed at creation */
    int32_t history;                /* 500 */
    int32_t nsamples;               /* 7 (nN); 1..16, fixed at creation */
    int32_t knn_samples;            /* 2 (nkNN): MAX(1, cvRound(0.1 * nN * 3 + 0.40)) of the default nN;
                                       as in the reference, another nsamples does not change it */
    int32_t detect_shadows;         /* 1 */
    int32_t shadow_value;           /* 127; 0..255 */
    float   dist2_threshold;        /* 400 (fTb) */
    float   shadow_threshold;       /* 0.5 (fTau) */
    uint64_t rng_state;             /* 0xffffffff, a fresh thread's cv::theRNG(); read at creation only */
} tbdk_knn_config;

/* the reference's defaults for a frame of this size and channel count */
int tbdk_knn_config_default(int width, int height, int channels, tbdk_knn_config* cfg);
/* Allocates the model (nothing is allocated afterwards; nothing is copied or synchronised: the
 * first fill takes rng_state as an argument).  TBDK_EINVAL:
 * channels other than 1 / 3, nsamples outside 1..16, width or height outside 1..65535, history < 1,
 * shadow_value outside 0..255, a NaN threshold. */
int tbdk_knn_create(tbdk_ctx* ctx, const tbdk_knn_config* cfg, tbdk_knn** out);
int tbdk_knn_destroy(tbdk_knn* m);
/* The next apply starts from an empty model (frames() becomes 0).  The RNG state stays.  No
 * device work. */
int tbdk_knn_reset(tbdk_knn* m);
/* The reference's setters, all at once: takes every field of cfg but the fixed ones, which must
 * equal the object's (TBDK_EINVAL otherwise, nothing changed), and rng_state, which is ignored.
 * Holds from the next apply on. */
int tbdk_knn_set_params(tbdk_knn* m, const tbdk_knn_config* cfg);
/* apply(frame, fgmask, learningRate): fgmask (device, 8-bit, width x height, mask_pitch bytes a
 * row) gets 0 (background), shadow_value (shadow) or 255 per pixel, and the model is updated.
 * The schedule is the reference's, kept on the host: model, indices, next-update planes and the
 * three counters are zeroed (on the stream; the RNG is not touched) on the first call, after
 * tbdk_knn_reset and when learning_rate >= 1; the rate is learning_rate if it is >= 0 and this is
 * not the first frame, else 1 / min(2 * frames, history); the update periods come from the rate
 * by double log; after the kernel each counter that reached its period is zeroed and its plane
 * redrawn, in the order short, mid, long.  Asynchronous on `stream`, no allocation, no host
 * synchronisation; calls on one object are ordered by the caller's stream(s).
 * TBDK_EINVAL (nothing enqueued, nothing changed): a null pointer, a pitch below a row, and the
 * learning rates for which the reference converts an infinite, NaN or out-of-range double to int,
 * which is undefined: NaN, exactly 0, above 1, and a rate so small that a period's quotient
 * (log(0.1) / log(1 - rate) and its kin) does not fit an int with the increments that follow.
 * (On a first frame the reference would not look at the given rate; here it is rejected all the
 * same.)  A rate of exactly 1 is defined: it initialises the model and every quotient is 0.
 * Timed as "knn_apply", the fills as "knn_randu". */
int tbdk_knn_apply(tbdk_knn* m, const uint8_t* frame, int pitch, uint8_t* fgmask, int mask_pitch,
                   double learning_rate, void* stream);
/* getBackgroundImage: per pixel the first sample, in the order short, mid, long, whose flag is
 * set (gray: its channel 0), 0 where there is none.  img: device, 8-bit, the frames' channels,
 * pitch in bytes.  Timed as "knn_background". */
int tbdk_knn_get_background(tbdk_knn* m, uint8_t* img, int pitch, void* stream);
/* The model in the reference's layout, for tests and checkpoints (device pointers, any may be
 * NULL): samples[h][w][3 * nsamples][channels + 1] (uint8), index3[3][h][w] and next3[3][h][w]
 * (uint8; short, mid, long), counters[3] (int32; short, mid, long) and the RNG state after every
 * fill enqueued so far (uint64), all tight.  Timed as "knn_model". */
int tbdk_knn_get_model(tbdk_knn* m, uint8_t* samples, uint8_t* index3, uint8_t* next3, int32_t* counters,
                       uint64_t* rng_state, void* stream);
/* frames applied since the model was last cleared */
int tbdk_knn_frames(tbdk_knn* m, int* nframes);

/* ---- morphology and connected components ----------------------------------- */

/* cv::MorphTypes (the four built) and cv::MorphShapes */
#define TBDK_MORPH_ERODE 0
#define TBDK_MORPH_DILATE 1
#define TBDK_MORPH_OPEN 2
#define TBDK_MORPH_CLOSE 3
#define TBDK_MORPH_RECT 0
#define TBDK_MORPH_CROSS 1
#define TBDK_MORPH_ELLIPSE 2

/* cv::getStructuringElement (imgproc/src/morph.dispatch.cpp:135-186), host only: out gets
 * kw x kh bytes, rows first, 1 = in.  CROSS uses the anchor, (-1, -1) is the centre; a 1 x 1
 * element is a RECT; ELLIPSE rounds its half width half to even, in double.  TBDK_EINVAL: another
 * shape, a size below 1, an anchor outside, out NULL. */
int tbdk_structuring_element(int shape, int kw, int kh, int anchor_x, int anchor_y, uint8_t* out);

/* cv::erode / cv::dilate / cv::morphologyEx(MORPH_OPEN, MORPH_CLOSE) on an 8-bit one-channel device
 * image, 1..65535 a side, pitched, any alignment: per pixel the min (erode) or max (dilate) of the
 * border-extended image over the element's non-zero positions, gray levels included.  OPEN is erode
 * then dilate, CLOSE the reverse, each with the full `iterations`.  src == dst is allowed.
 *   element  : host, kw x kh bytes, non-zero = in, read before the call returns; NULL: the
 *              reference's 3 x 3 rectangle (kw, kh ignored)
 *   anchor   : inside the element, or (-1, -1) for its centre
 *   iterations, as morphOp (:952-972) applies them: 0, or a 1 x 1 element, copies src to dst; a NULL
 *              element is one pass of the (1 + 2 it)-square rectangle anchored at (it, it); an
 *              element without a zero and it > 1 is one pass of the k + (it - 1)(k - 1) rectangle
 *              with the anchor times it, whatever the border (with an explicit border value this
 *              differs from iterating; the reference's result is the one returned); any other
 *              element runs it passes, each on the previous result
 *   border_type  : TBDK_BORDER_CONSTANT, _REPLICATE, _REFLECT or _REFLECT_101, for images smaller
 *              than the element too
 *   border_value : -1 for morphologyDefaultBorderValue (under BORDER_CONSTANT the outside is
 *              ignored), or 0..255, what a pixel outside counts as under BORDER_CONSTANT
 * A rectangle runs as a row pass then a column pass, any other element as one 2-D pass per
 * iteration; the element travels in the kernel arguments.  Enqueues its kernels on `stream` and
 * returns: no upload, no host synchronisation, and no allocation unless the context's intermediate
 * planes (up to two, width x height bytes each; calls on one context are ordered by the caller) have
 * to grow.  TBDK_EINVAL, with nothing enqueued and dst untouched: a null image, an op other than
 * the four (GRADIENT, TOPHAT, BLACKHAT and HITMISS are not built), a size outside 1..65535, a pitch
 * below a row, BORDER_WRAP or any other border, a border value outside -1..255, negative
 * iterations, an anchor outside, an element with no non-zero entry, an effective element (after the
 * rules above) of more than 31 a side, more than 64 passes.  Timed as "morph". */
int tbdk_morph_u8(tbdk_ctx* ctx, int op, const uint8_t* src, int width, int height, int src_pitch, uint8_t* dst,
                  int dst_pitch, const uint8_t* element, int kw, int kh, int anchor_x, int anchor_y, int iterations,
                  int border_type, int border_value, void* stream);

/* cv::ConnectedComponentsAlgorithmsTypes and the columns of a stats row */
#define TBDK_CCL_WU 0
#define TBDK_CCL_DEFAULT (-1)
#define TBDK_CCL_GRANA 1
#define TBDK_CC_STAT_LEFT 0
#define TBDK_CC_STAT_TOP 1
#define TBDK_CC_STAT_WIDTH 2
#define TBDK_CC_STAT_HEIGHT 3
#define TBDK_CC_STAT_AREA 4

/* cv::connectedComponentsWithStats (imgproc/src/connectedcomponents.cpp), ltype CV_32S, everything
 * on the device.  img: 8-bit, width x height (width * height < 2^31), pitch in bytes; every non-zero
 * pixel is foreground.  labels: int32, labels_pitch bytes a row (a multiple of 4), always complete:
 * 0 for background, 1..N-1 for the components, numbered as the reference numbers them, by the raster
 * position of a component's first pixel (TBDK_CCL_WU, and connectivity 4 whatever the type) or of
 * its first 2 x 2 block (TBDK_CCL_GRANA / TBDK_CCL_DEFAULT at connectivity 8).  n_labels (device
 * int32) gets N, the reference's return value.  stats (int32 [cap][5]: LEFT, TOP, WIDTH, HEIGHT,
 * AREA) and centroids (double [cap][2]: double(sum x) / double(area) from 64-bit sums), either may be
 * NULL: rows l < min(N, cap) are written, label 0's too, rows from N on are left untouched.  An
 * image with no background pixel gives row 0 as the reference leaves it: INT_MAX, INT_MAX, the
 * wrapped extents 2, 2, area 0 and a NaN centroid.  Enqueues seven to nine kernels on `stream` and
 * returns: no host synchronisation, and no allocation unless the context's scratch (8 to 9 bytes a
 * pixel plus 40 a stats row; calls on one context are ordered by the caller) has to grow.
 * TBDK_EINVAL, nothing enqueued: a null img, labels or n_labels, a size below 1 or of 2^31 pixels
 * or more, a pitch below a row, a labels pointer or pitch that is no multiple of 4, a connectivity
 * other than 4 or 8, another ccltype, cap < 0, or cap < 1 with stats or centroids given.  Timed as
 * "cc". */
int tbdk_connected_components(tbdk_ctx* ctx, const uint8_t* img, int width, int height, int pitch, int32_t* labels,
                              int labels_pitch, int connectivity, int ccltype, int32_t* stats, double* centroids,
                              int cap, int32_t* n_labels, void* stream);

/* ---- GaussianBlur (8-bit, fixed point) and threshold ------------------------ */

/* cv::ThresholdTypes */
#define TBDK_THRESH_BINARY 0
#define TBDK_THRESH_BINARY_INV 1
#define TBDK_THRESH_TRUNC 2
#define TBDK_THRESH_TOZERO 3
#define TBDK_THRESH_TOZERO_INV 4
#define TBDK_THRESH_MASK 7
#define TBDK_THRESH_OTSU 8
#define TBDK_THRESH_TRIANGLE 16 /* not built */

/* The n 8.8 fixed-point coefficients cv::GaussianBlur uses on 8-bit images
 * (getFixedpointGaussianKernel<ufixedpoint16>, imgproc/src/smooth.dispatch.cpp:124-169), host only:
 * the literal tables for n = 1, 3, 5, 7 at sigma <= 0, otherwise exp(-x^2 / (2 sigma^2)) normalised
 * and rounded to 1/256 in the reference's softdouble arithmetic, its own exp included; sigma <= 0 is
 * 0.15 n + 0.35.  They need not sum to 256.  TBDK_EINVAL: n < 1, out NULL. */
int tbdk_gaussian_kernel_u8(int n, double sigma, uint16_t* out);

/* The threshold stage tbdk_gaussian_blur_u8 can apply to every output byte before it is stored:
 * cv::threshold(blurred, dst, thresh, maxval, type) with one of the five plain types. */
typedef struct tbdk_thresh_params {
    double thresh, maxval;
    int32_t type;
    int32_t reserved;
} tbdk_thresh_params;

/* cv::GaussianBlur(src, dst, Size(kw, kh), sigma_x, sigma_y, border_type | BORDER_ISOLATED) on an
 * 8-bit device image of cn = 1, 3 or 4 interleaved channels, 1..65535 a side, pitched, any
 * alignment; every output byte is the reference's (GaussianBlurFixedPoint, imgproc/src/smooth.simd.hpp):
 * a row pass H = min(65535, sum kx[i] s[i]) in 8.8 fixed point, a column pass
 * min(255, (sum ky[j] H[j] + 32768) >> 16), terms outside the image fetched by borderInterpolate, or
 * left out under BORDER_CONSTANT.
 *   kw, kh   : odd, 1..31; <= 0 with a positive sigma is the reference's automatic size for 8-bit
 *              images, cvRound(6 sigma + 1) | 1; sigma_y <= 0 means sigma_x; a one-row or one-column
 *              image under a border other than CONSTANT collapses that dimension to 1; 1 x 1 copies
 *   border_type : TBDK_BORDER_CONSTANT (zero), _REPLICATE, _REFLECT, _WRAP or _REFLECT_101, for
 *              images smaller than the kernel too
 *   fused    : NULL, or the threshold applied to every output byte: the result is that of
 *              tbdk_threshold on the blurred image, with no intermediate image
 * One launch: a workgroup stages its source tile and halo in LDS, writes the row pass there as
 * 16-bit words and reads the column pass from them; the coefficients travel in the kernel
 * arguments.  Where src and dst overlap the blur goes to the context's intermediate plane
 * (tbdk_morph_u8's; calls on one context are ordered by the caller) and is copied out by a second
 * launch, as the reference clones its source.  Enqueues on `stream` and returns: no upload, no host
 * synchronisation, no allocation unless that plane has to grow.  TBDK_EINVAL, with nothing enqueued
 * and dst untouched: a null image, cn other than 1, 3, 4, a size outside 1..65535, a pitch below a
 * row, BORDER_TRANSPARENT or an unknown border, an even size, a size above 31 (given or automatic),
 * a size <= 0 without a positive sigma, a NaN sigma, a fused type other than the five plain ones
 * (THRESH_OTSU needs the whole blurred image first).  Timed as "blur". */
int tbdk_gaussian_blur_u8(tbdk_ctx* ctx, const uint8_t* src, int width, int height, int cn, int src_pitch,
                          uint8_t* dst, int dst_pitch, int kw, int kh, double sigma_x, double sigma_y,
                          int border_type, const tbdk_thresh_params* fused, void* stream);

/* cv::threshold(src, dst, thresh, maxval, type) on a device image, pitched (bytes), any alignment for
 * 8-bit images; src == dst is allowed.
 *   pix      : TBDK_PIX_U8 with any cn >= 1 (the image is width * cn bytes a row), or TBDK_PIX_F32
 *              with cn >= 1 (pointers and pitches multiples of 4)
 *   8-bit    : thresh.cpp:1556-1585: the threshold is cvFloor(thresh), maxval
 *              saturate_cast<uchar>(cvRound(maxval)), for TRUNC the threshold; thresholds below 0 and
 *              from 255 on give the reference's constant fills and copies
 *   32F      : the comparisons of the reference's vector body, in float: a NaN pixel is neither above
 *              nor at-or-below the threshold, and TRUNC returns the threshold for it (the reference's
 *              scalar remainder, the last w h mod 8 elements of a continuous image, returns the NaN)
 *   type     : one of the five, or with TBDK_THRESH_OTSU on a one-channel 8-bit image: a device
 *              histogram, getThreshVal_Otsu_8u's scan over it in double on one lane, in the
 *              reference's operation order, and an apply pass that reads the threshold on the
 *              device; thresh is ignored
 *   thresh_used : optional host double: the value the reference returns (the floored threshold for
 *              8-bit images); NaN with OTSU, whose value exists only on the device
 *   otsu_dev : required with OTSU, ignored otherwise: a device int32 that receives the chosen
 *              threshold, in stream order
 * Enqueues on `stream` and returns: no host synchronisation; OTSU uses 1 KB of the context's
 * intermediate plane.  TBDK_EINVAL, nothing enqueued: a null image, another pix, a size below 1 or
 * above 65535 a side, a pitch below a row, THRESH_TRIANGLE or an unknown type, OTSU on anything but
 * one-channel 8-bit or without otsu_dev, a NaN thresh or maxval.  Timed as "threshold". */
int tbdk_threshold(tbdk_ctx* ctx, const void* src, int pix, int width, int height, int cn, int src_pitch, void* dst,
                   int dst_pitch, double thresh, double maxval, int type, double* thresh_used, int32_t* otsu_dev,
                   void* stream);

/* ---- synthetic sequences (bench / test input) ----------------------------- */

/* Renders frames [t0, t0+nframes) of the deterministic synthetic sequence of
 * opencv_amd/csrc/synth_spec.h into `out` (device, nframes x height x pitch).
 * gt_boxes (host, may be NULL): nframes x nobj x 5 int32 {valid, x, y, w, h}. */
int tbdk_synth_render(tbdk_ctx* ctx, uint32_t seed, int width, int height, int nobj,
                      int t0, int nframes, uint8_t* out, int pitch, int32_t* gt_boxes,
                      void* stream);

/* ---- measurement ---------------------------------------------------------- */

/* Copies `bytes` (a multiple of 16; dst and src 16-byte aligned, not
 * overlapping) device to device with a hand-written 16-byte-per-lane stream
 * copy (global_load_dwordx4 / global_store_dwordx4), asynchronously on
 * `stream`; timed as kernel "hbm_copy".  bench.py's measured HBM copy peak
 * (SURVEY.md §8(d)); no reference counterpart. */
int tbdk_hbm_copy(tbdk_ctx* ctx, void* dst, const void* src, int64_t bytes, void* stream);

/* Library version string */
const char* tbdk_version(void);
/* TBDK_ABI_VERSION of the library (struct layouts of this header) */
int tbdk_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TBDK_H */
