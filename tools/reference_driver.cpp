// reference_driver.cpp — records the reference's CPU functions on raw files for
// tests/golden/reference_<op>.npz (see tools/record_reference_cases.md).
// Links against a scratch build of the reference's core, imgproc, video,
// objdetect and calib3d modules; nothing in the test suite builds or runs it.
//
//   reference_driver <op> <out-prefix> key=value ...
//
// Images are raw 8-bit files (rows of w * cn bytes), or, for gftt and cmap with
// depth=32f, raw float32 files of one channel (remap and warpperspective:
// depth=32f with cn channels, and raw maps); every output goes to
// <out-prefix>.<name> as raw little-endian data.  The first line printed is the
// runtime dispatch state, "SSE4_1=. AVX=. AVX2=. FMA3=."; the caller checks it.
//
//   pyr   a= w= h= cn= winw= winh= maxl=           -> L<i> (u8), D<i> (i16, 2cn per pixel); prints the level sizes
//   lk    a= b= w= h= cn= winw= winh= maxl= flags= pts= n= [init=] err=0|1
//                                                  -> q (f32 pairs), st (u8), err (f32, if err=1)
//   gftt  a= w= h= maxc= ql= md= block= harris= k= [mask=] [depth=8u|32f] -> c (f32 pairs); prints the count
//                                                  (mask: raw u8, w x h, goodFeaturesToTrack's mask)
//   cmap  a= w= h= block= harris= k= [depth=8u|32f] -> e (f32): cornerMinEigenVal / cornerHarris, ksize 3
//   subpix a= w= h= [depth=8u|32f] pts= n= winw= winh= zw= zh= ctype= cmax= ceps= -> c (f32 pairs): cornerSubPix;
//                                                  prints "expf w bits..." for w = 1..15: expf(-(k/w)^2), k = 0..w
//   warp  a= w= h= m= (6 doubles, raw) dst= dw= dh= flags= border= bval=   -> w (u8)
//   fb    a= b= w= h= ps= lv= ws= it= pn= sg= flags= [init=]               -> f (f32 pairs)
//   hoggrad a= w= h= cn= gamma= signed=            -> g (f32 pairs), qa (u8 pairs)
//   hogdet  a= w= h= cn= win=64|48 hit= group=     -> loc (i32 pairs), wt (f64), r (i32 x4), rw (f64), svm (f32)
//   remap a= w= h= cn= depth=8u|32f dst= dw= dh= kind=32fc2|32fc1|16sc2 m1= [m2=] inter= border= bv0= bv1= bv2= bv3=
//                                                  -> w (the image's type): remap into the pre-filled destination.
//                                                  m1: CV_32FC2, CV_32FC1 or CV_16SC2; m2: CV_32FC1 or CV_16UC1.  A 1x1
//                                                  INTER_LINEAR remap runs first: initInterTab2D fills NNDeltaTab_i on the
//                                                  first interpolating call of a process, and INTER_NEAREST with a
//                                                  fraction plane reads it
//   warpperspective a= w= h= cn= depth= m= (9 doubles, raw) dst= dw= dh= flags= border= bv0..bv3=
//                                                  -> w (the image's type), minv (9 doubles): invert(M)
//   circle  w= h= cx= cy= r=                       -> m (u8): circle(img, (cx, cy), r, Scalar(0), -1) on a 255-filled
//                                                  CV_8UC1 image (no input image)
//   homography src= dst= (f32 pairs, raw) n= method= thr= iters= conf=
//                                                  -> h (9 doubles; nothing for an empty result), mask (n u8):
//                                                  findHomography(src, dst, method, thr, mask, iters, conf); prints
//                                                  "valid 0|1" (0 also where the reference throws, as it does for n = 0)
//   affine2d src= dst= (f32 pairs, raw) n= model=0|1 method= thr= iters= conf= refine=
//                                                  -> m (6 doubles; nothing for an empty result), mask (n u8):
//                                                  estimateAffine2D (model 0) or estimateAffinePartial2D (model 1)
//                                                  (src, dst, mask, method, thr, iters, conf, refine); prints "valid 0|1"
//   mog2  a= (n frames, raw) w= h= cn= depth=8u|32f n= rates= (n doubles, raw) bg= (n bytes, raw) history= nmix=
//         shadows= sval= vt= vtg= vinit= vmin= vmax= bgr= ct= tau=
//                                                  -> masks (n x h x w u8), bg (the frame's type, one image per
//                                                  non-zero byte of bg=): createBackgroundSubtractorMOG2, every
//                                                  setter, apply(frame, mask, rates[t]) per frame and
//                                                  getBackgroundImage after the marked ones
//   knn   a= (n 8-bit frames, raw) w= h= cn= n= rates= (n doubles, raw) bg= (n bytes, raw) seed= (decimal uint64)
//         history= nsamples= knn= shadows= sval= d2t= tau=
//                                                  -> masks (n x h x w u8), bg (one image per non-zero byte of bg=),
//                                                  periods (n x 3 i32), state (1 u64): theRNG().state = seed on the
//                                                  calling thread, createBackgroundSubtractorKNN, every setter,
//                                                  apply(frame, mask, rates[t]) per frame, getBackgroundImage after
//                                                  the marked ones, and theRNG().state after the last frame, which
//                                                  pins the number of steps the fills consumed; periods are apply()'s
//                                                  nShortUpdate / nMidUpdate / nLongUpdate expressions evaluated here
//                                                  with this build's log
//   morph a= w= h= mop=0..3 [elem= kw= kh=] ax= ay= it= border= bval= inplace=0|1
//                                                  -> d (u8): erode / dilate (mop 0 / 1) or morphologyEx (mop 2 / 3)
//                                                  with the element (raw kw x kh bytes; absent: an empty Mat),
//                                                  anchor, iterations, border type and border value (-1:
//                                                  morphologyDefaultBorderValue()); inplace=1: dst is src
//   cc    a= w= h= conn= type=                     -> labels (i32), stats (i32 x5), cent (f64 x2); prints "n N":
//                                                  connectedComponentsWithStats(a, labels, stats, centroids, conn,
//                                                  CV_32S, type)
//   strel shape= kw= kh= ax= ay=                   -> e (u8, kw x kh): getStructuringElement (no input image)
//   blur  a= w= h= cn= kw= kh= sx= sy= border= inplace=0|1
//                                                  -> d (u8): GaussianBlur(a, d, Size(kw, kh), sx, sy, border |
//                                                  BORDER_ISOLATED); inplace=1: dst is src
//   blurk a= w= pairs= n=                          -> resp (u8, n rows of w): the one-row image a through
//                                                  GaussianBlur(a, d, Size(k, k), sigma) for each of the n (k, sigma)
//                                                  pairs (f64) of the file pairs, in one process
//   threshold a= w= h= cn= depth=8u|32f thresh= maxval= type=
//                                                  -> d (the source's type), t (f64): threshold(a, d, thresh, maxval,
//                                                  type) and the value it returns
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/calib3d.hpp>
#include <opencv2/core.hpp>
#include <opencv2/imgproc.hpp>
#include <opencv2/objdetect.hpp>
#include <opencv2/video/background_segm.hpp>
#include <opencv2/video/tracking.hpp>

using namespace cv;

static std::map<std::string, std::string> g_args;

static const std::string& arg(const std::string& k)
{
    std::map<std::string, std::string>::const_iterator it = g_args.find(k);
    if (it == g_args.end()) throw std::runtime_error("missing argument " + k);
    return it->second;
}
static bool has(const std::string& k) { return g_args.count(k) != 0; }
static int iarg(const std::string& k) { return std::atoi(arg(k).c_str()); }
static double darg(const std::string& k) { return std::strtod(arg(k).c_str(), NULL); }

static void rd(const std::string& path, void* dst, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(dst, 1, bytes, f) != bytes) throw std::runtime_error("short read of " + path);
    std::fclose(f);
}

static void wr(const std::string& out, const char* name, const void* src, size_t bytes)
{
    FILE* f = std::fopen((out + "." + name).c_str(), "wb");
    if (!f || std::fwrite(src, 1, bytes, f) != bytes) throw std::runtime_error("cannot write " + out + "." + name);
    std::fclose(f);
}

static void wr(const std::string& out, const std::string& name, const Mat& m)
{
    Mat c = m.isContinuous() ? m : m.clone();
    wr(out, name.c_str(), c.data, c.total() * c.elemSize());
}

static Mat image(const std::string& key, int w, int h, int cn)
{
    Mat m(h, w, CV_8UC(cn));
    rd(arg(key), m.data, (size_t)w * h * cn);
    return m;
}

// the source image of gftt / cmap: CV_8UC1, or CV_32FC1 with depth=32f
static Mat image_depth(const std::string& key, int w, int h)
{
    if (!has("depth") || arg("depth") == "8u") return image(key, w, h, 1);
    if (arg("depth") != "32f") throw std::runtime_error("depth must be 8u or 32f");
    Mat m(h, w, CV_32FC1);
    rd(arg(key), m.data, (size_t)w * h * 4);
    return m;
}

// the source or destination of remap / warpperspective: CV_8UC(cn) or CV_32FC(cn)
static Mat image_typed(const std::string& key, int w, int h, int cn)
{
    const bool f32 = has("depth") && arg("depth") == "32f";
    Mat m(h, w, f32 ? CV_32FC(cn) : CV_8UC(cn));
    rd(arg(key), m.data, (size_t)w * h * m.elemSize());
    return m;
}

static Mat raw_mat(const std::string& key, int w, int h, int type)
{
    Mat m(h, w, type);
    rd(arg(key), m.data, (size_t)w * h * m.elemSize());
    return m;
}

static int run_warps(const std::string& op, const std::string& out)
{
    const int w = iarg("w"), h = iarg("h"), cn = iarg("cn"), dw = iarg("dw"), dh = iarg("dh");
    Mat a = image_typed("a", w, h, cn), d = image_typed("dst", dw, dh, cn);
    const uchar* before = d.data;
    const Scalar bv(darg("bv0"), darg("bv1"), darg("bv2"), darg("bv3"));
    if (op == "remap") {
        const std::string kind = arg("kind");
        Mat m1, m2;
        if (kind == "32fc2") {
            m1 = raw_mat("m1", dw, dh, CV_32FC2);
        } else if (kind == "32fc1") {
            m1 = raw_mat("m1", dw, dh, CV_32FC1);
            m2 = raw_mat("m2", dw, dh, CV_32FC1);
        } else if (kind == "16sc2") {
            m1 = raw_mat("m1", dw, dh, CV_16SC2);
            if (has("m2")) m2 = raw_mat("m2", dw, dh, CV_16UC1);
        } else {
            throw std::runtime_error("unknown map kind " + kind);
        }
        {
            Mat s1(1, 1, CV_8UC1, Scalar(0)), d1, mm(1, 1, CV_32FC2, Scalar(0, 0));
            remap(s1, d1, mm, noArray(), INTER_LINEAR);
        }
        remap(a, d, m1, m2, iarg("inter"), iarg("border"), bv);
    } else {
        double m[9], mi[9];
        rd(arg("m"), m, sizeof m);
        Mat M(3, 3, CV_64F, m), Mi(3, 3, CV_64F, mi);
        invert(M, Mi);
        if (Mi.data != (uchar*)mi) throw std::runtime_error("invert reallocated its destination");
        wr(out, "minv", mi, sizeof mi);
        warpPerspective(a, d, M, Size(dw, dh), iarg("flags"), iarg("border"), bv);
    }
    if (d.data != before) throw std::runtime_error(op + " reallocated the destination");
    wr(out, "w", d);
    return 0;
}

static int run_homography(const std::string& out)
{
    const int n = iarg("n");
    std::vector<Point2f> p(n), q(n);
    if (n) {
        rd(arg("src"), p.data(), sizeof(Point2f) * n);
        rd(arg("dst"), q.data(), sizeof(Point2f) * n);
    }
    Mat H, mask;
    try {
        H = findHomography(p, q, iarg("method"), darg("thr"), mask, iarg("iters"), darg("conf"));
    } catch (const cv::Exception&) {
        H.release();
    }
    const bool valid = !H.empty();
    std::printf("valid %d\n", (int)valid);
    std::vector<uchar> m(n, 0);
    if (valid) {
        if (H.type() != CV_64F || H.total() != 9 || (int)mask.total() != n || mask.type() != CV_8U)
            throw std::runtime_error("findHomography: unexpected result type");
        wr(out, "h", H);
        if (n) std::memcpy(m.data(), mask.data, n);
    }
    wr(out, "mask", m.data(), n);
    return 0;
}

static int run_affine2d(const std::string& out)
{
    const int n = iarg("n");
    std::vector<Point2f> p(n), q(n);
    if (n) {
        rd(arg("src"), p.data(), sizeof(Point2f) * n);
        rd(arg("dst"), q.data(), sizeof(Point2f) * n);
    }
    Mat M, mask;
    try {
        if (iarg("model") == 0)
            M = estimateAffine2D(p, q, mask, iarg("method"), darg("thr"), (size_t)iarg("iters"), darg("conf"),
                                 (size_t)iarg("refine"));
        else
            M = estimateAffinePartial2D(p, q, mask, iarg("method"), darg("thr"), (size_t)iarg("iters"), darg("conf"),
                                        (size_t)iarg("refine"));
    } catch (const cv::Exception&) {
        M.release();
    }
    const bool valid = !M.empty();
    std::printf("valid %d\n", (int)valid);
    std::vector<uchar> m(n, 0);
    if (valid) {
        if (M.type() != CV_64F || M.total() != 6 || (int)mask.total() != n || mask.type() != CV_8U)
            throw std::runtime_error("estimateAffine2D: unexpected result type");
        wr(out, "m", M);
        if (n) std::memcpy(m.data(), mask.data, n);
    }
    wr(out, "mask", m.data(), n);
    return 0;
}

static int run_mog2(const std::string& out)
{
    const int w = iarg("w"), h = iarg("h"), cn = iarg("cn"), n = iarg("n");
    const int type = arg("depth") == "32f" ? CV_32FC(cn) : CV_8UC(cn);
    Mat all(n * h, w, type);
    rd(arg("a"), all.data, all.total() * all.elemSize());
    std::vector<double> rates(n);
    std::vector<uchar> want(n);
    rd(arg("rates"), rates.data(), sizeof(double) * n);
    rd(arg("bg"), want.data(), n);
    Ptr<BackgroundSubtractorMOG2> m = createBackgroundSubtractorMOG2(iarg("history"), darg("vt"), iarg("shadows") != 0);
    m->setHistory(iarg("history"));
    m->setNMixtures(iarg("nmix"));
    m->setDetectShadows(iarg("shadows") != 0);
    m->setShadowValue(iarg("sval"));
    m->setVarThreshold(darg("vt"));
    m->setVarThresholdGen(darg("vtg"));
    m->setVarInit(darg("vinit"));
    m->setVarMin(darg("vmin"));
    m->setVarMax(darg("vmax"));
    m->setBackgroundRatio(darg("bgr"));
    m->setComplexityReductionThreshold(darg("ct"));
    m->setShadowThreshold(darg("tau"));
    Mat masks(n * h, w, CV_8UC1);
    std::vector<uchar> bgs;
    for (int t = 0; t < n; ++t) {
        Mat mask;
        m->apply(all.rowRange(t * h, (t + 1) * h), mask, rates[t]);
        if (mask.type() != CV_8UC1 || mask.rows != h || mask.cols != w) throw std::runtime_error("mog2: mask type");
        mask.copyTo(masks.rowRange(t * h, (t + 1) * h));
        if (want[t]) {
            Mat bg;
            m->getBackgroundImage(bg);
            if (bg.type() != type || bg.rows != h || bg.cols != w) throw std::runtime_error("mog2: background type");
            Mat c = bg.isContinuous() ? bg : bg.clone();
            bgs.insert(bgs.end(), c.data, c.data + c.total() * c.elemSize());
        }
    }
    wr(out, "masks", masks);
    wr(out, "bg", bgs.data(), bgs.size());
    return 0;
}

static int run_knn(const std::string& out)
{
    const int w = iarg("w"), h = iarg("h"), cn = iarg("cn"), n = iarg("n");
    const int type = CV_8UC(cn);
    Mat all(n * h, w, type);
    rd(arg("a"), all.data, all.total() * all.elemSize());
    std::vector<double> rates(n);
    std::vector<uchar> want(n);
    rd(arg("rates"), rates.data(), sizeof(double) * n);
    rd(arg("bg"), want.data(), n);
    theRNG().state = std::strtoull(arg("seed").c_str(), NULL, 10);
    const int history = iarg("history"), nN = iarg("nsamples");
    Ptr<BackgroundSubtractorKNN> m = createBackgroundSubtractorKNN(history, darg("d2t"), iarg("shadows") != 0);
    m->setHistory(history);
    m->setNSamples(nN);
    m->setkNNSamples(iarg("knn"));
    m->setDist2Threshold(darg("d2t"));
    m->setDetectShadows(iarg("shadows") != 0);
    m->setShadowValue(iarg("sval"));
    m->setShadowThreshold(darg("tau"));
    Mat masks(n * h, w, CV_8UC1);
    std::vector<uchar> bgs;
    std::vector<int> periods;
    int nframes = 0;
    for (int t = 0; t < n; ++t) {
        Mat mask;
        m->apply(all.rowRange(t * h, (t + 1) * h), mask, rates[t]);
        if (mask.type() != CV_8UC1 || mask.rows != h || mask.cols != w) throw std::runtime_error("knn: mask type");
        mask.copyTo(masks.rowRange(t * h, (t + 1) * h));
        if (nframes == 0 || rates[t] >= 1) nframes = 0;
        ++nframes;
        const double rate = rates[t] >= 0 && nframes > 1 ? rates[t] : 1. / std::min(2 * nframes, history);
        const int Kshort = (int)(log(0.7) / log(1 - rate)) + 1;
        const int Kmid = (int)(log(0.4) / log(1 - rate)) - Kshort + 1;
        const int Klong = (int)(log(0.1) / log(1 - rate)) - Kshort - Kmid + 1;
        periods.push_back(Kshort / nN + 1);
        periods.push_back(Kmid / nN + 1);
        periods.push_back(Klong / nN + 1);
        if (want[t]) {
            Mat bg;
            m->getBackgroundImage(bg);
            if (bg.type() != type || bg.rows != h || bg.cols != w) throw std::runtime_error("knn: background type");
            Mat c = bg.isContinuous() ? bg : bg.clone();
            bgs.insert(bgs.end(), c.data, c.data + c.total() * c.elemSize());
        }
    }
    const uint64 state = theRNG().state;
    wr(out, "masks", masks);
    wr(out, "bg", bgs.data(), bgs.size());
    wr(out, "periods", periods.data(), periods.size() * sizeof(int));
    wr(out, "state", &state, sizeof(state));
    return 0;
}

// erode / dilate / morphologyEx, connectedComponentsWithStats, getStructuringElement
static int run_blobs(const std::string& op, const std::string& out)
{
    if (op == "strel") {
        Mat e = getStructuringElement(iarg("shape"), Size(iarg("kw"), iarg("kh")), Point(iarg("ax"), iarg("ay")));
        if (e.type() != CV_8UC1) throw std::runtime_error("getStructuringElement: not CV_8UC1");
        wr(out, "e", e);
        return 0;
    }
    const int w = iarg("w"), h = iarg("h");
    Mat a = image("a", w, h, 1);
    if (op == "cc") {
        Mat labels, stats, cent;
        const int n = connectedComponentsWithStats(a, labels, stats, cent, iarg("conn"), CV_32S, iarg("type"));
        if (labels.type() != CV_32SC1 || stats.type() != CV_32SC1 || cent.type() != CV_64FC1 || stats.rows != n ||
            stats.cols != 5 || cent.rows != n || cent.cols != 2)
            throw std::runtime_error("connectedComponentsWithStats: unexpected output layout");
        std::printf("n %d\n", n);
        wr(out, "labels", labels);
        wr(out, "stats", stats);
        wr(out, "cent", cent);
        return 0;
    }
    Mat elem;
    if (has("elem")) {
        elem.create(iarg("kh"), iarg("kw"), CV_8UC1);
        rd(arg("elem"), elem.data, (size_t)elem.rows * elem.cols);
    }
    const Point anchor(iarg("ax"), iarg("ay"));
    const int mop = iarg("mop"), it = iarg("it"), border = iarg("border"), bval = iarg("bval");
    const Scalar bv = bval < 0 ? morphologyDefaultBorderValue() : Scalar::all(bval);
    Mat d;
    if (iarg("inplace")) d = a;
    const uchar* before = a.data;
    if (mop == MORPH_ERODE)
        erode(a, d, elem, anchor, it, border, bv);
    else if (mop == MORPH_DILATE)
        dilate(a, d, elem, anchor, it, border, bv);
    else
        morphologyEx(a, d, mop, elem, anchor, it, border, bv);
    if (iarg("inplace") && d.data != before) throw std::runtime_error("the in-place call reallocated its image");
    wr(out, "d", d);
    return 0;
}

// GaussianBlur on 8-bit images, the coefficient sweep, threshold
static int run_smooth(const std::string& op, const std::string& out)
{
    const int w = iarg("w");
    if (op == "blurk") {
        const int n = iarg("n");
        Mat a = image("a", w, 1, 1);
        std::vector<double> pairs((size_t)n * 2);
        rd(arg("pairs"), pairs.data(), pairs.size() * sizeof(double));
        Mat resp(n, w, CV_8UC1);
        for (int i = 0; i < n; ++i) {
            Mat d;
            const int k = (int)pairs[2 * i];
            GaussianBlur(a, d, Size(k, k), pairs[2 * i + 1]);
            if (d.type() != CV_8UC1 || d.rows != 1 || d.cols != w) throw std::runtime_error("blurk: unexpected output");
            d.copyTo(resp.row(i));
        }
        wr(out, "resp", resp);
        return 0;
    }
    const int h = iarg("h"), cn = iarg("cn");
    if (op == "blur") {
        Mat a = image("a", w, h, cn), d;
        if (iarg("inplace")) d = a;
        const uchar* before = a.data;
        GaussianBlur(a, d, Size(iarg("kw"), iarg("kh")), darg("sx"), darg("sy"), iarg("border") | BORDER_ISOLATED);
        if (iarg("inplace") && d.data != before) throw std::runtime_error("the in-place call reallocated its image");
        if (d.type() != a.type() || d.size() != a.size()) throw std::runtime_error("blur: unexpected output");
        wr(out, "d", d);
        return 0;
    }
    Mat a = image_typed("a", w, h, cn), d;
    const double t = threshold(a, d, darg("thresh"), darg("maxval"), iarg("type"));
    if (d.type() != a.type() || d.size() != a.size()) throw std::runtime_error("threshold: unexpected output");
    wr(out, "d", d);
    wr(out, "t", &t, sizeof t);
    return 0;
}

static int run(const std::string& op, const std::string& out)
{
    if (op == "blur" || op == "blurk" || op == "threshold") return run_smooth(op, out);
    if (op == "morph" || op == "cc" || op == "strel") return run_blobs(op, out);
    if (op == "mog2") return run_mog2(out);
    if (op == "knn") return run_knn(out);
    if (op == "homography") return run_homography(out);
    if (op == "affine2d") return run_affine2d(out);
    const int w = iarg("w"), h = iarg("h"), cn = has("cn") ? iarg("cn") : 1;
    if (op == "remap" || op == "warpperspective") return run_warps(op, out);
    if (op == "circle") {
        Mat m(h, w, CV_8UC1, Scalar(255));
        circle(m, Point(iarg("cx"), iarg("cy")), iarg("r"), Scalar(0), -1);
        wr(out, "m", m);
        return 0;
    }
    Mat a = op == "gftt" || op == "cmap" || op == "subpix" ? image_depth("a", w, h) : image("a", w, h, cn);
    if (op == "pyr") {
        std::vector<Mat> pyr;
        int top = buildOpticalFlowPyramid(a, pyr, Size(iarg("winw"), iarg("winh")), iarg("maxl"), true);
        std::printf("levels %d\n", top + 1);
        for (int i = 0; i <= top; ++i) {
            std::printf("%d %d\n", pyr[2 * i].cols, pyr[2 * i].rows);
            wr(out, "L" + std::to_string(i), pyr[2 * i]);
            wr(out, "D" + std::to_string(i), pyr[2 * i + 1]);
        }
    } else if (op == "lk") {
        Mat b = image("b", w, h, cn);
        const int n = iarg("n"), flags = iarg("flags");
        std::vector<Point2f> p(n), q;
        rd(arg("pts"), p.data(), sizeof(Point2f) * n);
        if (has("init")) {
            q.resize(n);
            rd(arg("init"), q.data(), sizeof(Point2f) * n);
        }
        std::vector<uchar> st;
        std::vector<float> err;
        const Size win(iarg("winw"), iarg("winh"));
        const TermCriteria crit(TermCriteria::COUNT + TermCriteria::EPS, 30, 0.01);
        if (iarg("err"))
            calcOpticalFlowPyrLK(a, b, p, q, st, err, win, iarg("maxl"), crit, flags, 1e-4);
        else
            calcOpticalFlowPyrLK(a, b, p, q, st, noArray(), win, iarg("maxl"), crit, flags, 1e-4);
        wr(out, "q", q.data(), sizeof(Point2f) * n);
        wr(out, "st", st.data(), n);
        if (iarg("err")) wr(out, "err", err.data(), sizeof(float) * n);
    } else if (op == "gftt") {
        std::vector<Point2f> c;
        if (has("mask"))
            goodFeaturesToTrack(a, c, iarg("maxc"), darg("ql"), darg("md"), image("mask", w, h, 1), iarg("block"),
                                iarg("harris") != 0, darg("k"));
        else
            goodFeaturesToTrack(a, c, iarg("maxc"), darg("ql"), darg("md"), noArray(), iarg("block"),
                                iarg("harris") != 0, darg("k"));
        std::printf("corners %d\n", (int)c.size());
        wr(out, "c", c.data(), sizeof(Point2f) * c.size());
    } else if (op == "cmap") {
        Mat e;
        if (iarg("harris"))
            cornerHarris(a, e, iarg("block"), 3, darg("k"));
        else
            cornerMinEigenVal(a, e, iarg("block"), 3);
        wr(out, "e", e);
    } else if (op == "subpix") {
        const int n = iarg("n");
        std::vector<Point2f> c(n);
        rd(arg("pts"), c.data(), sizeof(Point2f) * n);
        cornerSubPix(a, c, Size(iarg("winw"), iarg("winh")), Size(iarg("zw"), iarg("zh")),
                     TermCriteria(iarg("ctype"), iarg("cmax"), darg("ceps")));
        wr(out, "c", c.data(), sizeof(Point2f) * n);
        // the window mask's exponentials, expf(-(k/w)^2), as float bits: one line per w = 1..15, k = 0..w
        for (int ww = 1; ww <= 15; ++ww) {
            std::printf("expf %d", ww);
            for (int k = 0; k <= ww; ++k) {
                const float x = (float)k / ww, e = expf(-x * x);
                unsigned bits;
                std::memcpy(&bits, &e, 4);
                std::printf(" %08x", bits);
            }
            std::printf("\n");
        }
    } else if (op == "warp") {
        double m[6];
        rd(arg("m"), m, sizeof m);
        const int dw = iarg("dw"), dh = iarg("dh");
        Mat M(2, 3, CV_64F, m), d(dh, dw, CV_8UC1);
        rd(arg("dst"), d.data, (size_t)dw * dh);
        const uchar* before = d.data;
        warpAffine(a, d, M, Size(dw, dh), iarg("flags"), iarg("border"), Scalar(iarg("bval")));
        if (d.data != before) throw std::runtime_error("warpAffine reallocated the destination");
        wr(out, "w", d);
    } else if (op == "fb") {
        Mat b = image("b", w, h, 1), flow;
        if (has("init")) {
            flow.create(h, w, CV_32FC2);
            rd(arg("init"), flow.data, (size_t)w * h * 8);
        }
        calcOpticalFlowFarneback(a, b, flow, darg("ps"), iarg("lv"), iarg("ws"), iarg("it"), iarg("pn"), darg("sg"),
                                 iarg("flags"));
        wr(out, "f", flow);
    } else if (op == "hoggrad") {
        HOGDescriptor hog;
        hog.gammaCorrection = iarg("gamma") != 0;
        hog.signedGradient = iarg("signed") != 0;
        Mat grad, qa;
        hog.computeGradient(a, grad, qa, Size(), Size());
        wr(out, "g", grad);
        wr(out, "qa", qa);
    } else if (op == "hogdet") {
        const bool small = iarg("win") == 48;
        HOGDescriptor hog(small ? Size(48, 96) : Size(64, 128), Size(16, 16), Size(8, 8), Size(8, 8), 9);
        std::vector<float> svm = small ? HOGDescriptor::getDaimlerPeopleDetector()
                                       : HOGDescriptor::getDefaultPeopleDetector();
        hog.gammaCorrection = true;  // the default constructor's value; this constructor's default is false
        hog.setSVMDetector(svm);
        std::vector<Point> loc;
        std::vector<double> wt, rw;
        std::vector<Rect> r;
        hog.detect(a, loc, wt, darg("hit"), Size(8, 8), Size(0, 0));
        hog.detectMultiScale(a, r, rw, darg("hit"), Size(8, 8), Size(), 1.05, iarg("group"));
        std::printf("windows %d rects %d\n", (int)loc.size(), (int)r.size());
        wr(out, "loc", loc.data(), sizeof(Point) * loc.size());
        wr(out, "wt", wt.data(), sizeof(double) * wt.size());
        wr(out, "r", r.data(), sizeof(Rect) * r.size());
        wr(out, "rw", rw.data(), sizeof(double) * rw.size());
        wr(out, "svm", svm.data(), sizeof(float) * svm.size());
    } else {
        throw std::runtime_error("unknown operation " + op);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    for (int i = 3; i < argc; ++i) {
        std::string kv = argv[i];
        size_t eq = kv.find('=');
        if (eq == std::string::npos) return 2;
        g_args[kv.substr(0, eq)] = kv.substr(eq + 1);
    }
    setNumThreads(1);
    std::printf("SSE4_1=%d AVX=%d AVX2=%d FMA3=%d\n", (int)checkHardwareSupport(CV_CPU_SSE4_1),
                (int)checkHardwareSupport(CV_CPU_AVX), (int)checkHardwareSupport(CV_CPU_AVX2),
                (int)checkHardwareSupport(CV_CPU_FMA3));
    try {
        return run(argv[1], argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "reference_driver: %s\n", e.what());
        return 1;
    }
}
