"""cv::cornerSubPix restated in numpy (imgproc/src/cornersubpix.cpp:44-156 on
getRectSubPix, imgproc/src/samplers.cpp:129-268), for the tests of
tbdk_corner_sub_pix.  Every operation is a float32 or float64 numpy operation in
the reference's order, none fused; tests/test_subpix_oracle.py pins it to the
real function's recorded outputs (tests/golden/reference_subpix.npz), word for
word.  The points of a call are carried together (arrays over the points still
iterating); each point's arithmetic is its own.

What a straightforward restatement gets wrong:

  window mask : float products of two expf values; numpy's float32 exp is not
                glibc's expf, so expf comes from libm through ctypes
  patch       : three code paths with different bits: the 8-bit inside path with
                its running `prev` (prev = (float)(t * s), s a double), the
                generic path inside and at the border (replicated rows and
                columns); 32F images always take the generic one
  sums        : a, b, c, bb1, bb2 are double chains in raster order; np.sum is
                pairwise, np.cumsum is the sequential chain

A uint16 image is the float32 image of the same values."""
import ctypes as C
import ctypes.util

import numpy as np

import _oracle as O

F32, F64 = np.float32, np.float64
DBL_EPSILON = np.finfo(np.float64).eps

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def expf(x):
    """glibc's expf of a float32 value, as float32"""
    return F32(_libm.expf(C.c_float(float(F32(x)))))


def exp_axis(win):
    """expf(-x*x), x = (float)(j - win) / win, j = 0 .. 2*win (cornersubpix.cpp:71-80)"""
    out = np.empty(2 * win + 1, F32)
    for j in range(2 * win + 1):
        x = F32(j - win) / F32(win)
        out[j] = expf(-x * x)
    return out


def window_mask(win, zero=(-1, -1)):
    """the (2*win_h+1, 2*win_w+1) float32 mask, zero zone applied where the reference applies it"""
    ww, wh = 2 * win[0] + 1, 2 * win[1] + 1
    m = (exp_axis(win[1])[:, None] * exp_axis(win[0])[None, :]).astype(F32)
    if zero[0] >= 0 and zero[1] >= 0 and zero[0] * 2 + 1 < ww and zero[1] * 2 + 1 < wh:
        m[win[1] - zero[1]:win[1] + zero[1] + 1, win[0] - zero[0]:win[0] + zero[0] + 1] = 0
    return m


def limits(criteria):
    """(max_iters, eps squared) of a (type, maxCount, epsilon) criteria (cornersubpix.cpp:52-54)"""
    typ, count, epsilon = criteria
    max_iters = min(max(int(count), 1), 100) if typ & 1 else 100
    eps = max(float(epsilon), 0.0) if typ & 2 else 0.0
    return max_iters, eps * eps


def rect_sub_pix(S, is_u8, cI, pw, ph):
    """getRectSubPix(src, (pw, ph), cI[k]) -> float32 patches (n, ph, pw), and per
    point whether the rectangle lay strictly inside the image.  S: the image as
    float32 (exact for 8-bit and 16-bit pixels)."""
    H, W = S.shape
    n = len(cI)
    cx = cI[:, 0] - F32(pw - 1) * F32(0.5)
    cy = cI[:, 1] - F32(ph - 1) * F32(0.5)
    fx, fy = np.floor(cx), np.floor(cy)
    ipx, ipy = fx.astype(np.int64), fy.astype(np.int64)
    a, b = (cx - fx).astype(F32), (cy - fy).astype(F32)
    inside = (0 <= ipx) & (ipx < W - pw) & (0 <= ipy) & (ipy < H - ph)
    out = np.empty((n, ph, pw), F32)
    one = F32(1)

    fast = inside if is_u8 else np.zeros(n, bool)
    if fast.any():  # getRectSubPix_8u32f's own loop (samplers.cpp:232-262)
        k = np.flatnonzero(fast)
        af = np.maximum(a[k], F32(0.0001))[:, None, None]
        bf = b[k][:, None, None]
        a12, a22, b1, b2 = af * (one - bf), af * bf, one - bf, bf
        s = (1.0 - af.astype(F64)) / af.astype(F64)
        ys = ipy[k][:, None, None] + np.arange(ph)[None, :, None]
        xs = ipx[k][:, None, None] + np.arange(pw + 1)[None, None, :]
        r0, r1 = S[ys, xs], S[ys + 1, xs]
        t = a12 * r0[:, :, 1:] + a22 * r1[:, :, 1:]
        prev = np.empty_like(t)
        prev[:, :, 0] = ((one - af) * (b1 * r0[:, :, :1] + b2 * r1[:, :, :1]))[:, :, 0]
        prev[:, :, 1:] = (t[:, :, :-1].astype(F64) * s).astype(F32)
        out[k] = prev + t

    if (~fast).any():  # getRectSubPix_Cn_<T, float, float> (samplers.cpp:129-216)
        k = np.flatnonzero(~fast)
        ak, bk = a[k][:, None, None], b[k][:, None, None]
        a11, a12, a21, a22 = (one - ak) * (one - bk), ak * (one - bk), (one - ak) * bk, ak * bk
        b1, b2 = one - bk, bk
        ix, iy = ipx[k], ipy[k]
        # adjustRect (samplers.cpp:48-102), columns: src advanced to `base`, rect.x = rx, rect.width = rw
        base = np.where(ix >= 0, ix, 0)
        rx = np.where(ix >= 0, 0, np.minimum(-ix, pw))
        rw = np.where(ix < W - pw, pw, W - ix - 1)
        base = base + np.minimum(rw, 0)
        rw = np.maximum(rw, 0)
        base = (base - rx)[:, None]
        rx, rw = rx[:, None], rw[:, None]
        j = np.arange(pw)[None, :]
        interp = (j >= rx) & (j < rw)
        x0 = np.where(interp, base + j, base + np.where(j >= rw, rw, rx))
        x1 = np.where(interp, x0 + 1, x0)
        # rows: src stays on row 0 while i < rect.y and on the last row from rect.height on
        i = np.arange(ph)[None, :]
        y0 = np.clip(iy[:, None] + i, 0, H - 1)
        y1 = np.clip(iy[:, None] + i + 1, 0, H - 1)
        assert x0.min() >= 0 and x1.max() <= W - 1
        Y0, Y1, X0, X1 = y0[:, :, None], y1[:, :, None], x0[:, None, :], x1[:, None, :]
        four = S[Y0, X0] * a11 + S[Y0, X1] * a12 + S[Y1, X0] * a21 + S[Y1, X1] * a22
        two = S[Y0, X0] * b1 + S[Y1, X0] * b2
        out[k] = np.where(interp[:, None, :], four, two)
    return out, inside


def corner_sub_pix(img, pts, win=(10, 10), zero=(-1, -1), criteria=(3, 20, 0.03), info=None):
    """cv::cornerSubPix(img, pts, win, zero, TermCriteria(*criteria)) -> refined (n, 2) float32.
    info (a dict, optional) receives per-point arrays: `iters` (updates made),
    `det` (stopped on the determinant), `left` (left the image), `capped` (stopped
    by the iteration limit with err still above eps), `reverted`, `border8` (an
    8-bit patch touched the border in some iteration)."""
    img = np.asarray(img)
    is_u8 = img.dtype == np.uint8
    assert img.ndim == 2 and img.dtype in (np.uint8, np.uint16, np.float32)
    S = np.ascontiguousarray(img, dtype=F32)
    H, W = S.shape
    cT = np.ascontiguousarray(pts, dtype=F32).reshape(-1, 2)
    n = len(cT)
    ww, wh = 2 * win[0] + 1, 2 * win[1] + 1
    assert win[0] > 0 and win[1] > 0 and W >= ww + 4 and H >= wh + 4
    max_iters, eps = limits(criteria)
    m = window_mask(win, zero).astype(F64)[None]
    px = (np.arange(ww) - win[0]).astype(F64)[None, None, :]
    py = (np.arange(wh) - win[1]).astype(F64)[None, :, None]

    cI = cT.copy()
    iters = np.zeros(n, np.int64)
    det_stop, left, capped, border8 = (np.zeros(n, bool) for _ in range(4))
    active = np.ones(n, bool)
    while active.any():
        k = np.flatnonzero(active)
        patch, inside = rect_sub_pix(S, is_u8, cI[k], ww + 2, wh + 2)
        if is_u8:
            border8[k] |= ~inside
        tgx = (patch[:, 1:-1, 2:] - patch[:, 1:-1, :-2]).astype(F64)
        tgy = (patch[:, 2:, 1:-1] - patch[:, :-2, 1:-1]).astype(F64)
        gxx, gxy, gyy = tgx * tgx * m, tgx * tgy * m, tgy * tgy * m
        terms = (gxx, gxy, gyy, gxx * px + gxy * py, gxy * px + gyy * py)
        with np.errstate(all="ignore"):
            a, b, c, bb1, bb2 = (np.cumsum(t.reshape(len(k), -1), axis=1)[:, -1] for t in terms)  # raster-order chains
            det = a * c - b * b
            ok = ~(np.abs(det) <= DBL_EPSILON * DBL_EPSILON)
            det_stop[k[~ok]] = True
            scale = 1.0 / np.where(ok, det, 1.0)
            x, y = cI[k, 0], cI[k, 1]
            nx = (x.astype(F64) + c * scale * bb1 - b * scale * bb2).astype(F32)
            ny = (y.astype(F64) - b * scale * bb1 + a * scale * bb2).astype(F32)
            err = ((nx - x) * (nx - x) + (ny - y) * (ny - y)).astype(F64)
        ko = k[ok]
        cI[ko, 0], cI[ko, 1] = nx[ok], ny[ok]
        iters[ko] += 1
        out = ok & ((nx < 0) | (nx >= W) | (ny < 0) | (ny >= H))
        left[k[out]] = True
        go = ok & ~out & (iters[k] < max_iters) & (err > eps)
        capped[k[ok & ~out & (iters[k] >= max_iters) & (err > eps)]] = True
        active[k] = go
    rev = (np.abs(cI[:, 0] - cT[:, 0]) > win[0]) | (np.abs(cI[:, 1] - cT[:, 1]) > win[1])
    cI[rev] = cT[rev]
    if info is not None:
        info.update(iters=iters, det=det_stop, left=left, capped=capped, reverted=rev, border8=border8)
    return cI


def refine_rows(img, corners, counts, win=(10, 10), zero=(-1, -1), criteria=(3, 20, 0.03)):
    """tbdk_corner_sub_pix on rows: corners (rows, cap, 2), counts (rows,) or None;
    row r's first counts[r] points (clamped to cap) are refined, everything else kept"""
    out = np.array(corners, dtype=F32, copy=True)
    rows, cap = out.shape[:2]
    for r in range(rows):
        c = cap if counts is None else min(int(counts[r]), cap)
        if c > 0:
            out[r, :c] = corner_sub_pix(img, out[r, :c], win, zero, criteria)
    return out


def gftt_rois_subpix(frame, rois, max_corners=256, quality=0.01, min_distance=3.0, win=(10, 10), **kw):
    """O.gftt_rois followed by cornerSubPix of every ROI's corners on the whole
    frame (window `win`, no zero zone, criteria (COUNT|EPS, 20, 0.03)): what the
    TBD loop does under ctx option tbd_subpix"""
    res = _gftt_rois(frame, rois, max_corners, quality, min_distance, **kw)
    return [corner_sub_pix(frame, c, win) if len(c) else c for c in res]


_gftt_rois = O.gftt_rois  # the unrefined one, whatever O.gftt_rois is patched to later
