"""numpy restatement of the image front end: cv::cvtColor (the six 8-bit codes
the loop needs) and cv::resize(INTER_LINEAR) on 8-bit images.

  * cvt_color     <- imgproc/src/color_rgb.simd.hpp:647 (RGB2Gray<uchar>, the
                     fixed-point form of color.simd_helpers.hpp:16-20), RGB2RGB
                     (alpha 255) and Gray2RGB
  * resize_linear <- imgproc/src/resize.cpp: coefficient generation :3582-3702
                     (float fx, cvFloor, the sx clamps, saturate_cast<short>(c*2048)),
                     HResizeLinear :1492, the uchar VResizeLinear :1578, the row
                     clip of resizeGeneric_Invoker :1825, the exact-2 INTER_AREA
                     switch :3523 (ResizeAreaFastVec :2534) and the equal-size copy

tests/test_frontend_oracle.py pins both to the real functions' recorded outputs
(tests/golden/frontend_cases.npz); the GPU tests compare the kernels with them.
"""
import numpy as np

# cv::ColorConversionCodes
COLOR_BGR2BGRA = 0
COLOR_BGR2GRAY = 6
COLOR_RGB2GRAY = 7
COLOR_GRAY2BGR = 8
COLOR_BGRA2GRAY = 10
COLOR_RGBA2GRAY = 11
CODES = {"BGR2BGRA": COLOR_BGR2BGRA, "BGR2GRAY": COLOR_BGR2GRAY, "RGB2GRAY": COLOR_RGB2GRAY,
         "GRAY2BGR": COLOR_GRAY2BGR, "BGRA2GRAY": COLOR_BGRA2GRAY, "RGBA2GRAY": COLOR_RGBA2GRAY}
# code -> source channels
SRC_CN = {COLOR_BGR2BGRA: 3, COLOR_BGR2GRAY: 3, COLOR_RGB2GRAY: 3, COLOR_GRAY2BGR: 1, COLOR_BGRA2GRAY: 4,
          COLOR_RGBA2GRAY: 4}

B2Y, G2Y, R2Y, YUV_SHIFT = 1868, 9617, 4899, 14


def pattern(w, h, cn, seed):
    """A reproducible u8 noise image from integer hashing alone (no generator
    state): the recorded cases' inputs, regenerated wherever they are needed."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64),
                          np.arange(cn, dtype=np.uint64), indexing="ij")
    v = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ (c * np.uint64(83492791)) ^ np.uint64(seed * 2654435761)
    v &= np.uint64(0xFFFFFFFF)
    v = (v ^ (v >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    v = (v ^ (v >> np.uint64(12))) * np.uint64(0x297A2D39) & np.uint64(0xFFFFFFFF)
    v = v ^ (v >> np.uint64(15))
    out = ((v >> np.uint64(8)) & np.uint64(255)).astype(np.uint8)
    return out[:, :, 0] if cn == 1 else out


def cvt_color(src, code):
    src = np.asarray(src)
    if code not in SRC_CN:
        raise ValueError("unknown colour code")
    cn = 1 if src.ndim == 2 else src.shape[2]
    if src.dtype != np.uint8 or cn != SRC_CN[code]:
        raise ValueError("bad source for this code")
    if code == COLOR_GRAY2BGR:
        return np.repeat(src[:, :, None], 3, axis=2)
    if code == COLOR_BGR2BGRA:
        return np.concatenate([src, np.full(src.shape[:2] + (1,), 255, np.uint8)], axis=2)
    s = src.astype(np.int32)
    c0, c2 = (B2Y, R2Y) if code in (COLOR_BGR2GRAY, COLOR_BGRA2GRAY) else (R2Y, B2Y)
    y = (s[:, :, 0] * c0 + s[:, :, 1] * G2Y + s[:, :, 2] * c2 + (1 << (YUV_SHIFT - 1))) >> YUV_SHIFT
    return y.astype(np.uint8)


def _sat_short(v):
    # saturate_cast<short>(float): cvRound (half to even), clamped
    return np.clip(np.rint(v), -32768, 32767).astype(np.int32)


def linear_coeffs(ssize, dsize):
    """(offset, a0, a1) per destination index, as resize.cpp:3609-3702 makes them
    for one axis; the x clamps are applied by the caller."""
    inv_scale = np.float64(dsize) / np.float64(ssize)
    scale = np.float64(1.0) / inv_scale
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = (f - s.astype(np.float32)).astype(np.float32)
    return s, f


def _coef_pair(f):
    c0 = (np.float32(1.0) - f).astype(np.float32)
    return _sat_short(c0 * np.float32(2048)), _sat_short(f * np.float32(2048))


def resize_linear(src, dsize):
    """cv::resize(src, dst, dsize, 0, 0, INTER_LINEAR) of a u8 image (H, W) or (H, W, cn)."""
    src = np.asarray(src)
    if src.dtype != np.uint8:
        raise ValueError("u8 only")
    dw, dh = int(dsize[0]), int(dsize[1])
    s3 = src[:, :, None] if src.ndim == 2 else src
    sh, sw, cn = s3.shape
    if (dw, dh) == (sw, sh):
        out = s3.copy()
    elif sw == 2 * dw and sh == 2 * dh:  # INTER_AREA, ResizeAreaFastVec
        s = s3.astype(np.int32)
        out = ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    else:
        sx, fx = linear_coeffs(sw, dw)
        lo = sx < 0
        fx = np.where(lo, np.float32(0), fx)
        sx = np.where(lo, 0, sx)
        hi = sx >= sw - 1
        fx = np.where(hi, np.float32(0), fx).astype(np.float32)
        sx = np.where(hi, sw - 1, sx)
        a0, a1 = _coef_pair(fx)
        sx1 = np.minimum(sx + 1, sw - 1)  # a1 == 0 wherever sx + 1 is outside
        sy, fy = linear_coeffs(sh, dh)
        b0, b1 = _coef_pair(fy)
        y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
        s = s3.astype(np.int32)
        rows = s[:, sx] * a0[None, :, None] + s[:, sx1] * a1[None, :, None]  # HResizeLinear, (sh, dw, cn)
        S0, S1 = rows[y0], rows[y1]
        out = ((((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2)
        out = out.astype(np.uint8)
    return out[:, :, 0] if src.ndim == 2 else out


def cvt_resize_gray(src, code, dsize):
    """The fused front end: every source tap converted to gray, then interpolated."""
    return resize_linear(cvt_color(src, code), dsize)
