"""numpy restatement of cv::GaussianBlur on 8-bit images (GaussianBlurFixedPoint, imgproc/src/smooth.simd.hpp, with
the 8.8 coefficients of getFixedpointGaussianKernel<ufixedpoint16>, smooth.dispatch.cpp:124-169) and of cv::threshold
on 8U and 32F images with THRESH_OTSU (imgproc/src/thresh.cpp).  tests/test_blur_oracle.py holds it to the recordings
(tests/golden/reference_blur.npz, reference_threshold.npz) bit for bit; the kernels are then held to it.

Python floats are IEEE doubles and nothing here is contracted, so the coefficient arithmetic has the reference's
softdouble bits; its one mulAdd is evaluated exactly with fractions."""
import struct
from fractions import Fraction

import numpy as np

CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
BORDER_NAMES = {CONSTANT: "constant", REPLICATE: "replicate", REFLECT: "reflect", WRAP: "wrap", REFLECT_101: "reflect101"}
BINARY, BINARY_INV, TRUNC, TOZERO, TOZERO_INV, OTSU, TRIANGLE = 0, 1, 2, 3, 4, 8, 16
TYPE_NAMES = {BINARY: "binary", BINARY_INV: "binary_inv", TRUNC: "trunc", TOZERO: "tozero", TOZERO_INV: "tozero_inv"}
MAXK = 31


def _d(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _round_even(v):
    return float(round(v))  # Python rounds a float half to even


_C0 = _d(0x3f83ce0f3e46f431)
_A = [_d(b) / _C0 for b in (0x3f55e7aa1566c2a4, 0x3f83b2a72b4f3cd3, 0x3fac6b08d81fec75, 0x3fcebfbdff82a45a,
                            0x3fe62e42fefa39f1)] + [1.0 / _C0]
_PRESCALE = _d(0x3ff71547652b82fe) * 64.0
# 2^(k/64) as the reference's table holds it: the correctly rounded double, which the exact root confirms
_TAB = []
for _k in range(64):
    # the double nearest to 2^(k/64): search the neighbours of the float power for the one whose 64th power is nearest 2^k
    _g = 2.0 ** (_k / 64.0)
    _best = min((_g, np.nextafter(_g, 0.0), np.nextafter(_g, 4.0)),
                key=lambda c: abs(Fraction(float(c)) ** 64 - Fraction(2) ** _k))
    _TAB.append(float(_best))


def sd_exp(x):
    """f64_exp (core/src/softfloat.cpp), for finite x"""
    x0 = (-192000.0 if x < 0 else 192000.0) if abs(x) >= 2048.0 else x * _PRESCALE
    r = _round_even(x0)
    val0 = int(r)
    t = min(max((val0 >> 6) + 1023, 0), 2047)
    buf = _d(t << 52)
    x0 = (x0 - r) * (1.0 / 64.0)
    a0, a1, a2, a3, a4, a5 = _A
    return buf * _C0 * _TAB[val0 & 63] * (((((a0 * x0 + a1) * x0 + a2) * x0 + a3) * x0 + a4) * x0 + a5)


_SMALL = {1: [256], 3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [8, 28, 56, 72, 56, 28, 8]}


def gaussian_kernel_u8(n, sigma):
    """the n 8.8 coefficients, uint16"""
    if sigma <= 0 and n in _SMALL:
        return np.array(_SMALL[n], np.uint16)
    sg = sigma if sigma > 0 else float(Fraction(n) * Fraction(0.15) + Fraction(0.35))  # mulAdd: one rounding
    scale = (-0.5 * 0.25) / (sg * sg)
    vals = [sd_exp(float(x * x) * scale) for x in range(1 - n, n, 2)]
    s = 0.0
    for v in vals:
        s += v
    s = 1.0 / s
    return np.array([0 if v * s < 0 else int(_round_even(v * s * 256.0)) & 0xFFFF for v in vals], np.uint16)


def cv_round(v):
    return int(_round_even(v))


def plan(w, h, ksize, sigma_x, sigma_y, border):
    """(kx, ky) as the call uses them, None for the copy; ValueError where the entry point refuses"""
    kw, kh = int(ksize[0]), int(ksize[1])
    if border != CONSTANT:
        if h == 1:
            kh = 1
        if w == 1:
            kw = 1
    if kw == 1 and kh == 1:
        return None
    if sigma_y <= 0:
        sigma_y = sigma_x
    if kw <= 0 and sigma_x > 0:
        kw = cv_round(sigma_x * 3 * 2 + 1) | 1
    if kh <= 0 and sigma_y > 0:
        kh = cv_round(sigma_y * 3 * 2 + 1) | 1
    if kw <= 0 or kh <= 0 or kw % 2 != 1 or kh % 2 != 1 or kw > MAXK or kh > MAXK:
        raise ValueError("kernel size")
    return gaussian_kernel_u8(kw, max(sigma_x, 0.0)), gaussian_kernel_u8(kh, max(sigma_y, 0.0))


def border_interp(p, n, border):
    """cv::borderInterpolate on an index array; -1 where BORDER_CONSTANT leaves the term out"""
    p = np.asarray(p, np.int64)
    inside = (p >= 0) & (p < n)
    if border == CONSTANT:
        return np.where(inside, p, -1)
    if border == REPLICATE:
        return np.clip(p, 0, n - 1)
    if border == WRAP:
        return p % n
    if n == 1:
        return np.zeros_like(p)
    delta = int(border == REFLECT_101)
    period = 2 * n - 2 * delta
    q = p % period
    return np.where(q < n, q, period - 1 + delta - q)


def new_counts():
    return dict(sat_h=0, clipped=0, border_terms={b: 0 for b in BORDER_NAMES}, ithresh_special=0)


def gaussian_blur(img, ksize, sigma_x, sigma_y=0, border=REFLECT_101, counts=None, threshold=None):
    """cv::GaussianBlur(img, ksize, sigma_x, sigma_y, border | BORDER_ISOLATED) on an H x W or H x W x C uint8 array.
    threshold: (thresh, maxval, type) applied to every output byte (the fused stage)"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8
    h, w = img.shape[:2]
    k = plan(w, h, ksize, sigma_x, sigma_y, border)
    if k is None:
        out = img.copy()
    else:
        kx, ky = (a.astype(np.int64) for a in k)
        s = img.reshape(h, w, -1).astype(np.int64)
        xs = border_interp(np.arange(w)[:, None] + np.arange(len(kx))[None, :] - len(kx) // 2, w, border)  # (w, kw)
        ys = border_interp(np.arange(h)[:, None] + np.arange(len(ky))[None, :] - len(ky) // 2, h, border)  # (h, kh)
        # row pass: H = min(65535, sum kx[i] s[i]), out-of-image terms left out under BORDER_CONSTANT
        taps = np.where((xs >= 0)[None, :, :, None], s[:, np.maximum(xs, 0), :], 0)  # (h, w, kw, c)
        hsum = (taps * kx[None, None, :, None]).sum(2)
        H = np.minimum(hsum, 65535)
        # column pass on the rows of H
        rows = np.where((ys >= 0)[:, :, None, None], H[np.maximum(ys, 0)], 0)  # (h, kh, w, c)
        vsum = np.minimum((rows * ky[None, :, None, None]).sum(1), 2 ** 32 - 1)
        o = (vsum + 32768) >> 16
        if counts is not None:
            counts["sat_h"] += int((hsum > 65535).sum())
            counts["clipped"] += int((o > 255).sum())
            if border != CONSTANT:
                far_x = ((np.arange(w)[:, None] + np.arange(len(kx))[None, :] - len(kx) // 2) != xs).sum()
                far_y = ((np.arange(h)[:, None] + np.arange(len(ky))[None, :] - len(ky) // 2) != ys).sum()
                counts["border_terms"][border] += int(far_x) * h + int(far_y) * w
            else:
                counts["border_terms"][border] += int((xs < 0).sum()) * h + int((ys < 0).sum()) * w
        out = np.minimum(o, 255).astype(np.uint8).reshape(img.shape)
    if threshold is not None:
        out = threshold_u8(out, *threshold)[1]
    return out


def cv_floor(v):
    i = int(v)
    return i - (i > v)


def threshold_u8(img, thresh, maxval, type_, counts=None):
    """cv::threshold on uint8 (any channel count); type_ may carry OTSU on a one-channel image.
    Returns (the threshold used, dst)"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8
    if type_ & OTSU:
        assert img.ndim == 2
        thresh = otsu(img)
    t = type_ & 7
    ithresh = cv_floor(thresh)
    imaxval = ithresh if t == TRUNC else cv_round(maxval)
    imaxval = min(max(imaxval, 0), 255)
    if counts is not None and (ithresh < 0 or ithresh >= 255):
        counts["ithresh_special"] += 1
    above = img.astype(np.int64) > ithresh
    if t == BINARY:
        out = np.where(above, imaxval, 0)
    elif t == BINARY_INV:
        out = np.where(above, 0, imaxval)
    elif t == TRUNC:
        out = np.where(above, imaxval, img)
    elif t == TOZERO:
        out = np.where(above, img, 0)
    elif t == TOZERO_INV:
        out = np.where(above, 0, img)
    else:
        raise ValueError("type")
    return float(ithresh), out.astype(np.uint8)


def threshold_f32(img, thresh, maxval, type_):
    """cv::threshold on float32, the comparisons of thresh_32f's vector body: `thresh < v` and `v <= thresh` are
    both false for a NaN pixel, and TRUNC's min returns thresh for one"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.float32
    th, mv = np.float32(thresh), np.float32(maxval)
    zero = np.float32(0)
    with np.errstate(invalid="ignore"):
        gt, le = th < img, img <= th
    if type_ == BINARY:
        out = np.where(gt, mv, zero)
    elif type_ == BINARY_INV:
        out = np.where(le, mv, zero)
    elif type_ == TRUNC:
        out = np.where(img < th, img, th)  # minps(v, thresh): thresh unless v < thresh
    elif type_ == TOZERO:
        out = np.where(gt, img, zero)
    elif type_ == TOZERO_INV:
        out = np.where(le, img, zero)
    else:
        raise ValueError("type")
    return float(th), out.astype(np.float32)


FLT_EPSILON = float(np.finfo(np.float32).eps)


def otsu(img):
    """getThreshVal_Otsu_8u (thresh.cpp:1143-1220): the scan over the 256 bins in double, in its operation order"""
    hist = np.bincount(np.ascontiguousarray(img).reshape(-1), minlength=256)
    scale = 1.0 / img.size
    mu = 0.0
    for i in range(256):
        mu += i * float(hist[i])
    mu *= scale
    mu1 = q1 = 0.0
    max_sigma = max_val = 0.0
    for i in range(256):
        p_i = float(hist[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, float(i)
    return max_val
