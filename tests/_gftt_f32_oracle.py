"""cornerMinEigenVal / cornerHarris / goodFeaturesToTrack on a CV_32F image,
restated in numpy for the 32F and 16U GFTT tests (tbdk_gftt_rois_px,
tbdk_corner_response_px).  Every operation is a float32 or float64 numpy
operation in the reference's order, none fused: the `noavx2` dispatch state
recorded in tests/golden/reference_gftt_f32.npz.

What differs from the 8-bit path (oracle/gftt_oracle.c):

  scale    = 1 / (4 * blockSize): the x 255 is CV_8U's (corner.cpp:250-256);
             k1 = (float)(1.0 * scale), k0 = (float)(2.0 * scale) (deriv.cpp:429-436)
  row pass : SymmRowSmallFilter<float, float> for ksize 3 (filter.simd.hpp:2893-2895):
             Dx row  S[x+1] - S[x-1]
             Dy row  S[x]*k0 + (S[x-1] + S[x+1])*k1

and what does not:

  column pass: Dx (R0 + R2)*k1 + (R1*k0 + 0), Dy (R2 - R0) + 0
  cov = (Dx*Dx, Dx*Dy, Dy*Dy); boxFilter in double: RowSum (ksize 3 and 5 tap by
  tap, other sizes the running form) and the running ColumnSum, carried row by
  row; calcMinEigenVal / calcHarris; then goodFeaturesToTrack's selection
  (_gftt_mask_oracle.select).

A uint16 image is the float32 image of the same values (the conversion is exact).
Pixels must be finite."""
import numpy as np

import _gftt_mask_oracle as MO

F32 = np.float32
STRIP = 56  # output columns per workgroup of the eigenvalue walk (kGfttStrip)


def refl_index(n, lo, hi):
    """BORDER_REFLECT_101 source indices of positions lo .. hi-1 of an axis of length n"""
    p = np.arange(lo, hi)
    if n == 1:
        return np.zeros_like(p)
    p = np.abs(p) % (2 * n - 2)
    return np.where(p >= n, 2 * n - 2 - p, p)


def as_f32(img):
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype in (np.float32, np.uint16), img.dtype
    return np.ascontiguousarray(img, dtype=F32)


def cov(img, block=3):
    """(3, h, w) float32: Dx*Dx, Dx*Dy, Dy*Dy"""
    img = as_f32(img)
    h, w = img.shape
    scale = 1.0 / (float(1 << 2) * block)
    k1, k0 = F32(1.0 * scale), F32(2.0 * scale)
    P = img[refl_index(h, -1, h + 1)][:, refl_index(w, -1, w + 1)]
    L, C, R = P[:, :-2], P[:, 1:-1], P[:, 2:]
    rx = R - L
    ry = C * k0 + (L + R) * k1
    dx = (rx[:-2] + rx[2:]) * k1 + (rx[1:-1] * k0 + F32(0))
    dy = (ry[2:] - ry[:-2]) + F32(0)
    out = np.stack([dx * dx, dx * dy, dy * dy])
    assert out.dtype == F32
    return out


def row_sums(c, block=3):
    """boxFilter's RowSum over cov: (3, h, w) float64"""
    _, h, w = c.shape
    anc = block // 2
    B = c.astype(np.float64)[:, :, refl_index(w, -anc, w - anc + block - 1)]  # the bordered rows
    if block in (3, 5):
        s = B[:, :, 0:w] + B[:, :, 1:w + 1]
        for t in range(2, block):
            s = s + B[:, :, t:w + t]
        return s
    out = np.empty((3, h, w), np.float64)
    s = np.zeros((3, h), np.float64)
    for t in range(block):
        s = s + B[:, :, t]
    out[:, :, 0] = s
    for x in range(w - 1):
        s = s + (B[:, :, x + block] - B[:, :, x])
        out[:, :, x + 1] = s
    return out


def column_sums(rs, block=3):
    """the running ColumnSum over the row sums.  Returns (box, before): box
    (3, h, w) float32, the filter's output; before (3, h, w) float64, SUM as it
    stands when row y is entered"""
    _, h, w = rs.shape
    anc = block // 2
    rows = refl_index(h, -anc, h - anc + block - 1)  # bordered row r -> source row
    S = np.zeros((3, w), np.float64)
    for r in range(block - 1):
        S = S + rs[:, rows[r]]
    box = np.empty((3, h, w), F32)
    before = np.empty((3, h, w), np.float64)
    for y in range(h):
        before[:, y] = S
        s0 = S + rs[:, rows[y + block - 1]]
        box[:, y] = s0.astype(F32)
        S = s0 - rs[:, rows[y]]
    return box, before


def response(img, block=3, harris=False, k=0.04):
    """cornerMinEigenVal(img, block, 3) / cornerHarris(img, block, 3, k), BORDER_REFLECT_101"""
    box, _ = column_sums(row_sums(cov(img, block), block), block)
    h, w = box.shape[1:]
    if not harris:
        a, b, c = box[0] * F32(0.5), box[1], box[2] * F32(0.5)
        t = a - c
        return (a + c) - np.sqrt(b * b + t * t)
    # calcHarris over the flattened map: AVX lines, one SSE block, the scalar double tail
    a, b, c = box[0].ravel(), box[1].ravel(), box[2].ravel()
    acbb, ac = a * c - b * b, a + c
    n = a.size
    avx_end = n & ~7
    sse_end = avx_end + (4 if n - avx_end >= 4 else 0)
    kf = F32(k)
    out = np.empty(n, F32)
    out[:avx_end] = acbb[:avx_end] - kf * (ac[:avx_end] * ac[:avx_end])
    out[avx_end:sse_end] = acbb[avx_end:sse_end] - (kf * ac[avx_end:sse_end]) * ac[avx_end:sse_end]
    t = ac[sse_end:].astype(np.float64)
    out[sse_end:] = (acbb[sse_end:].astype(np.float64) - float(k) * t * t).astype(F32)
    return out.reshape(h, w)


def gftt(img, mask, maxc, q, md, block=3, harris=False, k=0.04):
    """goodFeaturesToTrack(img, maxc, q, md, mask, block, harris, k) on an isolated image"""
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.shape == np.asarray(img).shape and mask.dtype == np.uint8
    with np.errstate(over="ignore", invalid="ignore"):
        return MO.select(response(img, block, harris, k), mask, maxc, q, md)


def gftt_rois(frame, mask, rois, maxc=256, q=0.01, md=3.0, block=3, harris=False, k=0.04):
    """per-ROI gftt on isolated ROIs (the mask cropped alike); corners in frame coordinates"""
    res = []
    for (x, y, w, h) in rois:
        m = None if mask is None else mask[y:y + h, x:x + w]
        res.append(gftt(frame[y:y + h, x:x + w], m, maxc, q, md, block, harris, k) + F32([x, y]))
    return res


def fresh_start_mismatch(img):
    """(strips, h) bool for blockSize 3: at row y of the aligned 56-column strip
    s, does a row segment's fresh start (0 + rs(y-1)) + rs(y) differ from the
    running ColumnSum as it stands there, in any channel, at a column whose sum
    reaches one of the strip's outputs (the strip's own columns and one more on
    each side, inside the image)?  Row 0 starts as the reference does."""
    rs = row_sums(cov(img, 3), 3)
    _, before = column_sums(rs, 3)
    h, w = rs.shape[1:]
    prev = rs[:, refl_index(h, -1, h - 1)]
    diff = (((0.0 + prev) + rs) != before).any(0)  # (h, w)
    n = (w + STRIP - 1) // STRIP
    out = np.zeros((n, h), bool)
    for s in range(n):
        out[s] = diff[:, max(s * STRIP - 1, 0):min(s * STRIP + STRIP + 1, w)].any(1)
    return out
