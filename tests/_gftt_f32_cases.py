"""Inputs of the 32F / 16U GFTT tests and the cases of
tests/golden/reference_gftt_f32.npz: cornerMinEigenVal / cornerHarris maps and
goodFeaturesToTrack lists, with and without a mask, on CV_32F images, recorded
from the real reference by `tools/record_reference_cases.py <driver> gftt_f32`
(tools/record_reference_cases.md).  Every input is generated; none is stored.

Content kinds (all finite):
  unit  : an 8-bit frame (the basketball frame, or hashed noise for the small
          map shapes) plus a hashed sub-LSB fraction, over 255: values in [0, 1)
          with full mantissas
  u16   : integer values 0..65535 (the frame in the high byte, hashed noise in
          the low one); as uint16 for our extension, as float32 for the reference
  hdr   : hashed mantissas and signs, exponents over 26 binades: a hashed two
          bits, plus 22 binades on every fourth row, the phase moving on by a
          row every 8 columns.  A row's sums then leave the running ColumnSum
          next to sums 2^44 times smaller, which rounds them, in every band of 32
          columns at the latest two rows below a ROI's top wherever that lies: a
          row segment's fresh start never equals the running sum
          (O32.fresh_start_mismatch: every row >= 2 of every strip at least
          HDR_MIN_STRIP columns wide; hashed exponents alone leave the first rows
          of most strips exact)
  small : hashed integers 0..7 as float32: no fresh start differs on any committed
          shape (0..15 already leaves a rounded sum in 3 % of a frame's strip rows)

The fixture follows tests/_reference_cases.py's layout (`state`,
`other_ints_equal`, `other_share`, `other_maxabs`; `<i>_e` the map of case i,
whole or as row CRCs; `<i>_c` the corner list as uint16 pairs): the map cases
first, then the list cases."""
import functools

import numpy as np

import _frontend_oracle as F
import _gftt_mask_cases as MC
import _reference_cases as RC

KINDS = ("unit", "u16", "hdr")
HARRIS_K = 0.04


def _hash16(w, h, seed):
    b = np.ascontiguousarray(F.pattern(w, h, 2, seed)).reshape(h, w, 2).astype(np.uint32)
    return b[:, :, 0] * 256 + b[:, :, 1]


def _base(w, h, seed):
    """the 8-bit picture under `unit` and `u16`: the basketball frame where it
    fits (the top-left w x h), hashed noise otherwise"""
    bb = RC.basketball()[0]
    if w >= 64 and h >= 64 and w <= bb.shape[1] and h <= bb.shape[0]:
        return np.ascontiguousarray(bb[:h, :w])
    return RC.noise(w, h, 1, seed).reshape(h, w)


def unit(w, h, seed):
    frac = _hash16(w, h, seed + 1).astype(np.float32) / np.float32(65536)
    return ((_base(w, h, seed).astype(np.float32) + frac) / np.float32(255)).astype(np.float32)


def u16(w, h, seed):
    low = np.ascontiguousarray(F.pattern(w, h, 1, seed + 2)).reshape(h, w).astype(np.uint16)
    return ((_base(w, h, seed).astype(np.uint16) << 8) | low).astype(np.uint16)


HDR_MIN_STRIP = 16  # columns of a strip from which the `hdr` guarantee holds


def hdr(w, h, seed):
    m = np.float32(1) + _hash16(w, h, seed + 3).astype(np.float32) / np.float32(65536)
    b = np.ascontiguousarray(F.pattern(w, h, 2, seed + 4)).reshape(h, w, 2).astype(np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    e = np.where((yy + xx // 8) % 4 == 0, 22, 0) + (b[:, :, 0] % 4) - 14
    sign = np.where(b[:, :, 1] & 1, np.float32(-1), np.float32(1))
    return (sign * np.ldexp(m, e)).astype(np.float32)


def small(w, h, seed):
    return (np.ascontiguousarray(F.pattern(w, h, 1, seed + 5)).reshape(h, w) & 7).astype(np.float32)


def image(kind, w, h, seed):
    """the image the kernels are given: float32, or uint16 for `u16`"""
    return {"unit": unit, "u16": u16, "hdr": hdr, "small": small}[kind](w, h, seed)


# ---- response maps: (h, w) x kind x (block, harris) -------------------------------
MAP_SHAPES = [(1, 7), (9, 1), (2, 2), (3, 3), (37, 61), (130, 121), (57, 9), (113, 40)]
MAP_MODES = [(2, 0), (3, 0), (5, 0), (3, 1)]
MAP_SEED = 900


def map_cases():
    """[(h, w, kind, block, harris)]"""
    return [(h, w, kind, b, hs) for (h, w) in MAP_SHAPES for kind in KINDS for b, hs in MAP_MODES]


def map_image(h, w, kind):
    return image(kind, w, h, MAP_SEED + 7 * h + w)


# ---- corner lists: isolated ROI crops of a 640 x 480 frame of each kind ----------------
FRAME_SEED = 1200
LIST_ROIS = [(0, 0, 160, 120), (401, 203, 57, 40), (10, 400, 113, 80), (600, 440, 3, 3)]
# (maxCorners, quality, minDistance, block, harris)
LIST_ROWS = [(256, 0.01, 3.0, 3, 0), (1000, 0.01, 0.0, 3, 0), (64, 0.05, 8.0, 5, 1), (300, 0.001, 2.5, 2, 0)]
LIST_MASKS = ("none", "rect1", "checker", "zero")


@functools.lru_cache(maxsize=None)
def frame(kind):
    """the 640 x 480 frame of a kind (shared: read only)"""
    f = image(kind, 640, 480, FRAME_SEED)
    f.setflags(write=False)
    return f


def list_cases():
    """[(kind, roi index, mask kind, maxCorners, quality, minDistance, block, harris)]"""
    return [(kind, r, mk, *row) for kind in KINDS for r in range(len(LIST_ROIS)) for mk in LIST_MASKS
            for row in LIST_ROWS]


def list_image(kind, r):
    x, y, w, h = LIST_ROIS[r]
    return np.ascontiguousarray(frame(kind)[y:y + h, x:x + w])


def list_mask(mk, w, h):
    return None if mk == "none" else {"rect1": MC.rect1, "checker": MC.checker, "zero": MC.zero}[mk](w, h)


def fixture():
    return RC.fixture("gftt_f32")
