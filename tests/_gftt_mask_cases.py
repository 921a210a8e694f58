"""Mask kinds of the masked GFTT tests, and the cases of
tests/golden/reference_gftt_mask.npz: goodFeaturesToTrack with a mask on
isolated ROI crops, recorded from the real reference by
`tools/record_reference_cases.py <driver> gftt_mask` (tools/record_reference_cases.md).

The fixture follows tests/_reference_cases.py's layout (`state`,
`other_ints_equal`, ..., `<i>_c` the corner list of case i as uint16 pairs) and
also stores the masks the reference was given, bit-packed: `mask_<m>_bits`
(np.packbits of mask != 0, row-major over the ROI) and `mask_<m>_val` (the
non-zero byte value: one element when all non-zero bytes are equal, else the
non-zero bytes in row-major order).  `case_mask[i]` is the mask of case i."""
import numpy as np

import _frontend_oracle as F
import _gftt_mask_oracle as MO
import _oracle as O
import _reference_cases as RC

KINDS = ("ones", "zero", "rect1", "checker", "sparse", "hole", "ring")
RESPONSE_KINDS = ("hole", "ring")  # built from the ROI's response map, so they depend on (block, harris)
HARRIS_K = 0.04


def ones(w, h):
    return np.full((h, w), 255, np.uint8)


def zero(w, h):
    return np.zeros((h, w), np.uint8)


def rect1(w, h):
    """the middle half in each axis, value 1"""
    m = np.zeros((h, w), np.uint8)
    m[h // 4:h - h // 4, w // 4:w - w // 4] = 1
    return m


def checker(w, h, sq=8):
    """sq x sq squares alternating 0 and 255 (the square at the origin is 0)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // sq) + (xx // sq)) & 1) * 255).astype(np.uint8)


def sparse(w, h, seed=4711):
    """about 10 % non-zero from the hashed noise of seed, values from {1, 128, 255}"""
    b = np.ascontiguousarray(F.pattern(w, h, 1, seed)).reshape(h, w).astype(np.int32)
    vals = np.array([1, 128, 255], np.uint8)
    return np.where(b < 26, vals[b % 3], 0).astype(np.uint8)


def hole(img, block=3, harris=False, k=HARRIS_K, radius=6):
    """255 except a disc around the image's strongest unmasked corner"""
    h, w = img.shape
    m = ones(w, h)
    c = O.gftt_ex(img, 1, 0.01, 0.0, block, harris, k)
    if len(c):
        yy, xx = np.mgrid[0:h, 0:w]
        m[(xx - int(c[0, 0])) ** 2 + (yy - int(c[0, 1])) ** 2 <= radius * radius] = 0
    return m


def ring_only(w, h, value=3):
    m = np.zeros((h, w), np.uint8)
    m[0, :] = m[-1, :] = value
    m[:, 0] = m[:, -1] = value
    return m


def ring(img, block=3, harris=False, k=HARRIS_K, value=3):
    """the outer one-pixel ring, plus every interior pixel whose response is
    below 0.25 x the ring's maximum"""
    h, w = img.shape
    m = ring_only(w, h, value)
    resp = MO.response(img, block, harris, k)
    ring_max = resp[m != 0].max()
    low = resp < np.float32(0.25) * ring_max
    low[m != 0] = False
    m[low] = value
    return m


def make(kind, img, block=3, harris=False, k=HARRIS_K, sq=8):
    """the mask of `kind` for an isolated image"""
    h, w = img.shape
    if kind == "ones":
        return ones(w, h)
    if kind == "zero":
        return zero(w, h)
    if kind == "rect1":
        return rect1(w, h)
    if kind == "checker":
        return checker(w, h, sq)
    if kind == "sparse":
        return sparse(w, h)
    if kind == "hole":
        return hole(img, block, harris, k)
    if kind == "ring":
        return ring(img, block, harris, k)
    raise ValueError(kind)


def pack_mask(m):
    nz = m[m != 0]
    val = nz[:1] if nz.size == 0 or (nz == nz[0]).all() else nz
    return np.packbits(m != 0), np.ascontiguousarray(val, dtype=np.uint8)


def unpack_mask(bits, val, w, h):
    on = np.unpackbits(bits)[:w * h].astype(bool)
    m = np.zeros(w * h, np.uint8)
    if val.size == 1:
        m[on] = val[0]
    elif val.size:
        m[on] = val
    return m.reshape(h, w)


# ---- the recorded cases ----------------------------------------------------------

# (frame, x, y, w, h)
ROIS = [("basketball", 0, 0, 160, 120), ("basketball", 300, 200, 77, 33), ("basketball", 250, 200, 64, 48),
        ("synth", 100, 100, 113, 90), ("basketball", 0, 0, 3, 3)]
# (maxCorners, quality, minDistance, block, harris)
ROWS = [(256, 0.01, 3.0, 3, 0), (1000, 0.01, 0.0, 3, 0), (64, 0.05, 8.0, 5, 1), (300, 0.001, 2.5, 2, 0)]


def roi_image(r):
    name, x, y, w, h = ROIS[r]
    return np.ascontiguousarray(RC.gftt_frame(name)[y:y + h, x:x + w])


def masks():
    """[(roi index, kind, block, harris)]: one entry per distinct mask (block and
    harris are 0 for the kinds that do not depend on the response)"""
    out = []
    modes = sorted({(b, hs) for _, _, _, b, hs in ROWS})
    for r in range(len(ROIS)):
        for kind in KINDS:
            out += [(r, kind, b, hs) for b, hs in modes] if kind in RESPONSE_KINDS else [(r, kind, 0, 0)]
    return out


def mask_of(entry):
    r, kind, block, harris = entry
    return make(kind, roi_image(r), block or 3, bool(harris))


def cases():
    """[(roi index, mask index, maxCorners, quality, minDistance, block, harris)]"""
    ms = masks()
    out = []
    for r in range(len(ROIS)):
        for kind in KINDS:
            for maxc, q, md, b, hs in ROWS:
                key = (r, kind, b, hs) if kind in RESPONSE_KINDS else (r, kind, 0, 0)
                out.append((r, ms.index(key), maxc, q, md, b, hs))
    return out


def fixture():
    return RC.fixture("gftt_mask")


def fixture_mask(fx, m):
    r = masks()[m][0]
    _, _, _, w, h = ROIS[r]
    return unpack_mask(fx[f"mask_{m}_bits"], fx[f"mask_{m}_val"], w, h)
