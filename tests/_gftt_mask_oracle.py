"""goodFeaturesToTrack under an 8-bit mask, restated in numpy on top of the
oracle's response maps (O.min_eig / O.corner_response), for the masked GFTT
tests.  Steps of imgproc/src/featureselect.cpp:361-516 from the response on:

  maxVal   = max of the response over the pixels whose mask byte is non-zero
             (:393 minMaxLoc(eig, 0, &maxVal, 0, 0, mask); 0 when there is none,
             core/src/minmax.cpp:806-807), over the whole map without a mask
  thr      = (float)(maxVal * qualityLevel); threshold-to-zero and the 3x3
             dilation run over every pixel, masked in or not (:394-395)
  candidate: interior pixel, val != 0, val == dilated, mask != 0 (:411)
  order    : value descending, then address descending (:56-64)
  walk     : greedy, a candidate is dropped when an accepted corner lies
             closer than minDistance, (float)(dx*dx + dy*dy) < minDistance^2
             (:466-481); stops at maxCorners

With mask=None it equals O.gftt_ex (tests/test_gftt_mask_oracle.py)."""
import numpy as np

import _oracle as O


def response(img, block=3, harris=False, k=0.04):
    """the map goodFeaturesToTrack selects from, as O.gftt_ex computes it"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if block == 3 and not harris:
        return O.min_eig(img)
    return O.corner_response(img, block, harris, k)


def masked_max(resp, mask):
    """maxVal (a double, as minMaxLoc returns it)"""
    if mask is None:
        return float(resp.max())
    sel = np.asarray(mask) != 0
    return float(resp[sel].max()) if sel.any() else 0.0


def select(resp, mask, maxc, q, md):
    """steps 2-5 on a response map -> (n, 2) float32 corners (x, y)"""
    h, w = resp.shape
    none = np.zeros((0, 2), np.float32)
    if h < 3 or w < 3:
        return none
    thr = np.float32(masked_max(resp, mask) * q)
    t = np.where(resp > thr, resp, np.float32(0)).astype(np.float32)
    dil = t[1:-1, 1:-1].copy()
    for dy in range(3):
        for dx in range(3):
            dil = np.maximum(dil, t[dy:dy + h - 2, dx:dx + w - 2])
    v = t[1:-1, 1:-1]
    ok = (v != 0) & (v == dil)
    if mask is not None:
        ok &= np.asarray(mask)[1:-1, 1:-1] != 0
    ys, xs = np.nonzero(ok)
    if ys.size == 0:
        return none
    ys, xs = ys + 1, xs + 1
    vals = t[ys, xs].astype(np.float64)
    idx = ys.astype(np.int64) * w + xs
    order = np.lexsort((-idx, -vals))  # value descending, then address descending
    ys, xs = ys[order], xs[order]
    if not md >= 1:
        n = min(len(ys), maxc) if maxc > 0 else len(ys)
        return np.stack([xs[:n], ys[:n]], 1).astype(np.float32)
    # the offsets closer than minDistance, with the walk's float32 rounding of dx*dx + dy*dy
    R = int(np.ceil(md))
    d = np.arange(-R, R + 1, dtype=np.float32)
    close = (d[None, :] * d[None, :] + d[:, None] * d[:, None]).astype(np.float32).astype(np.float64) < md * md
    acc = np.zeros((h + 2 * R, w + 2 * R), bool)  # accepted corners, R pixels of margin
    out = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        if (acc[y:y + 2 * R + 1, x:x + 2 * R + 1] & close).any():
            continue
        acc[y + R, x + R] = True
        out.append((x, y))
        if maxc > 0 and len(out) == maxc:
            break
    return np.array(out, np.float32).reshape(-1, 2)


def gftt_masked(img, mask, maxc, q, md, block=3, harris=False, k=0.04):
    """goodFeaturesToTrack(img, maxc, q, md, mask, block, harris, k) on an
    isolated u8 image; mask: None or a u8 array of img's shape"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.shape == img.shape and mask.dtype == np.uint8
    return select(response(img, block, harris, k), mask, maxc, q, md)


def gftt_rois_masked(frame, mask, rois, maxc=256, q=0.01, md=3.0, block=3, harris=False, k=0.04):
    """per-ROI gftt_masked on isolated ROIs with the mask cropped to the same
    rectangle; corners in frame coordinates (O.gftt_rois with a mask)"""
    res = []
    for (x, y, w, h) in rois:
        m = None if mask is None else mask[y:y + h, x:x + w]
        c = gftt_masked(frame[y:y + h, x:x + w], m, maxc, q, md, block, harris, k)
        res.append(c + np.float32([x, y]))
    return res
