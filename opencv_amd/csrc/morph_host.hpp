// morph_host.hpp — the host side of cv::erode / cv::dilate / cv::morphologyEx:
// getStructuringElement (imgproc/src/morph.dispatch.cpp:135-186), normalizeAnchor
// and morphOp's iteration rules (:952-972), restated.  morph.hip plans its
// launches with it; tests/cpp/blobs_host_check.cpp runs the same text under the
// sanitizers, which is why this file includes nothing of HIP.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

namespace tbdk {
namespace morph_host {

enum { kRect = 0, kCross = 1, kEllipse = 2 };  // cv::MorphShapes
constexpr int kMaxSide = 31;                    // one 32-bit row mask per element row

// normalizeAnchor (imgproc/src/filterengine.hpp): (-1, -1) is the centre, any
// other anchor must lie inside.  false: outside.
inline bool normalize_anchor(int kw, int kh, int* ax, int* ay)
{
    if (*ax == -1) *ax = kw / 2;
    if (*ay == -1) *ay = kh / 2;
    return *ax >= 0 && *ax < kw && *ay >= 0 && *ay < kh;
}

// getStructuringElement: out is kw x kh bytes, rows first, 1 = in.  false: a
// shape other than RECT / CROSS / ELLIPSE, a size below 1 or an anchor outside
// (the reference throws).  Any size: the 31 limit is the kernels', not this
// function's.
inline bool structuring_element(int shape, int kw, int kh, int ax, int ay, uint8_t* out)
{
    if (!out || kw < 1 || kh < 1 || (shape != kRect && shape != kCross && shape != kEllipse)) return false;
    if (!normalize_anchor(kw, kh, &ax, &ay)) return false;
    if (kw == 1 && kh == 1) shape = kRect;
    int r = 0, c = 0;
    double inv_r2 = 0;
    if (shape == kEllipse) {
        r = kh / 2;
        c = kw / 2;
        inv_r2 = r ? 1. / ((double)r * r) : 0;
    }
    for (int i = 0; i < kh; ++i) {
        uint8_t* row = out + (size_t)i * kw;
        int j1 = 0, j2 = 0;
        if (shape == kRect || (shape == kCross && i == ay))
            j2 = kw;
        else if (shape == kCross)
            j1 = ax, j2 = j1 + 1;
        else {
            const int dy = i - r;
            if (dy >= -r && dy <= r) {
                // saturate_cast<int>(double) is cvRound: round half to even (the default rounding mode)
                const double v = c * sqrt((double)(r * r - dy * dy) * inv_r2);
                const int dx = v >= 2147483647.0 ? 2147483647 : (int)lrint(v);
                j1 = c - dx > 0 ? c - dx : 0;
                j2 = c + dx + 1 < kw ? c + dx + 1 : kw;
            }
        }
        for (int j = 0; j < kw; ++j) row[j] = j >= j1 && j < j2;
    }
    return true;
}

// One erode or dilate call as the kernels run it.
struct Plan {
    bool copy;     // iterations == 0 or a 1x1 element: dst = src
    bool rect;     // every entry non-zero: a row pass, then a column pass
    int kw, kh, ax, ay;
    int passes;    // times the element is applied, each on the previous result
    uint32_t rows[kMaxSide];  // bit j of rows[i]: element(i, j) is in (rect: all kw bits)
};

// morphOp's rules.  element: kw x kh bytes or NULL (the 3x3 rectangle).  false
// (the caller returns TBDK_EINVAL): a size below 1, an anchor outside, negative
// iterations, an element with no entry, an effective side above kMaxSide.
inline bool make_plan(const uint8_t* element, int kw, int kh, int ax, int ay, int iterations, Plan* p)
{
    memset(p, 0, sizeof(*p));
    if (iterations < 0) return false;
    if (!element) kw = kh = 3;
    if (kw < 1 || kh < 1 || kw > 65535 || kh > 65535) return false;
    if (!normalize_anchor(kw, kh, &ax, &ay)) return false;
    int64_t nz = 0;
    if (element)
        for (int64_t i = 0; i < (int64_t)kw * kh; ++i) nz += element[i] != 0;
    if (iterations == 0 || (element && kw * kh == 1)) {  // tested first, as in the reference
        p->copy = true;
        p->kw = p->kh = 1;
        p->rows[0] = 1;
        return true;
    }
    if (element && nz == 0) return false;  // the reference's filter asserts a non-empty element
    p->passes = iterations;
    p->rect = !element || nz == (int64_t)kw * kh;
    if (!element) {  // the (1 + 2 it)-square rectangle, anchored at its centre, once
        if (iterations > (kMaxSide - 1) / 2) return false;
        kw = kh = 1 + 2 * iterations;
        ax = ay = iterations;
        p->passes = 1;
    } else if (iterations > 1 && p->rect) {  // one pass of the grown rectangle, whatever the border
        const int64_t gw = kw + (int64_t)(iterations - 1) * (kw - 1), gh = kh + (int64_t)(iterations - 1) * (kh - 1);
        if (gw > kMaxSide || gh > kMaxSide) return false;
        ax *= iterations;
        ay *= iterations;
        kw = (int)gw;
        kh = (int)gh;
        p->passes = 1;
    }
    if (kw > kMaxSide || kh > kMaxSide) return false;
    p->kw = kw;
    p->kh = kh;
    p->ax = ax;
    p->ay = ay;
    for (int i = 0; i < kh; ++i) {
        uint32_t m = 0;
        for (int j = 0; j < kw; ++j)
            if (p->rect || element[(size_t)i * kw + j]) m |= 1u << j;
        p->rows[i] = m;
    }
    return true;
}

}  // namespace morph_host
}  // namespace tbdk
