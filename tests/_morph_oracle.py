"""numpy restatement of cv::getStructuringElement, cv::erode, cv::dilate and cv::morphologyEx (OPEN, CLOSE) on
8UC1 images (imgproc/src/morph.dispatch.cpp): a plain min / max over shifted copies of the border-extended image,
plus morphOp's iteration rules (:952-972).  Independent of the library's code; tests/test_morph_oracle.py holds it
to the recordings."""
import numpy as np

ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
RECT, CROSS, ELLIPSE = 0, 1, 2
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = 0, 1, 2, 3, 4
DEFAULT_BORDER_VALUE = -1


def normalize_anchor(anchor, kw, kh):
    ax = kw // 2 if anchor[0] == -1 else anchor[0]
    ay = kh // 2 if anchor[1] == -1 else anchor[1]
    assert 0 <= ax < kw and 0 <= ay < kh
    return ax, ay


def structuring_element(shape, ksize, anchor=(-1, -1)):
    """getStructuringElement(shape, Size(kw, kh), anchor) -> (kh, kw) uint8 of 0 / 1"""
    kw, kh = ksize
    ax, ay = normalize_anchor(anchor, kw, kh)
    if (kw, kh) == (1, 1):
        shape = RECT
    e = np.zeros((kh, kw), np.uint8)
    if shape == RECT:
        e[:] = 1
    elif shape == CROSS:
        e[ay, :] = 1
        e[:, ax] = 1
    else:
        r, c = kh // 2, kw // 2
        inv_r2 = 1.0 / (float(r) * r) if r else 0.0
        for i in range(kh):
            dy = i - r
            if abs(dy) <= r:
                dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv_r2)))  # half to even, in double
                e[i, max(c - dx, 0):min(c + dx + 1, kw)] = 1
    return e


def border_index(p, n, border):
    """borderInterpolate for an array of positions; -1 under BORDER_CONSTANT"""
    p = np.asarray(p)
    if border == BORDER_REPLICATE:
        return np.clip(p, 0, n - 1)
    if border in (BORDER_REFLECT, BORDER_REFLECT_101):
        if n == 1:
            return np.zeros_like(p)
        d = int(border == BORDER_REFLECT_101)
        q = p.copy()
        for _ in range(4 * (int(np.abs(p).max()) // n + 2)):  # the reference's loop, one fold a turn
            lo, hi = q < 0, q >= n
            if not (lo | hi).any():
                break
            q = np.where(lo, -q - 1 + d, np.where(hi, n - 1 - (q - n) - d, q))
        assert ((q >= 0) & (q < n)).all()
        return q
    assert border == BORDER_CONSTANT
    return np.where((p >= 0) & (p < n), p, -1)


def one_pass(img, elem, anchor, dilate, border, bval):
    """min / max of the extended image over the element's non-zero positions"""
    h, w = img.shape
    kh, kw = elem.shape
    ax, ay = anchor
    xs = border_index(np.arange(-ax, w + kw - 1 - ax), w, border)
    ys = border_index(np.arange(-ay, h + kh - 1 - ay), h, border)
    ext = img[np.clip(ys, 0, None)][:, np.clip(xs, 0, None)].astype(np.int32)
    ext[ys < 0, :] = bval
    ext[:, xs < 0] = bval
    out = np.full((h, w), 0 if dilate else 255, np.int32)
    for i in range(kh):
        for j in range(kw):
            if elem[i, j]:
                v = ext[i:i + h, j:j + w]
                out = np.maximum(out, v) if dilate else np.minimum(out, v)
    return out.astype(np.uint8)


def morph_op(img, dilate, elem, anchor, iterations, border, border_value):
    """morphOp: one erode or dilate call with the reference's iteration rules"""
    assert border in (BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101) and iterations >= 0
    kh, kw = (3, 3) if elem is None else elem.shape
    anchor = normalize_anchor(anchor, kw, kh)
    if iterations == 0 or (elem is not None and kw * kh == 1):
        return img.copy()
    if elem is None:
        elem = np.ones((1 + 2 * iterations,) * 2, np.uint8)
        anchor = (iterations, iterations)
        iterations = 1
    elif iterations > 1 and elem.all():
        anchor = (anchor[0] * iterations, anchor[1] * iterations)
        elem = np.ones((kh + (iterations - 1) * (kh - 1), kw + (iterations - 1) * (kw - 1)), np.uint8)
        iterations = 1
    assert elem.any()
    bval = border_value if border_value >= 0 else (0 if dilate else 255)
    out = img
    for _ in range(iterations):
        out = one_pass(out, elem, anchor, dilate, border, bval)
    return out


def morphology_ex(img, op, elem, anchor=(-1, -1), iterations=1, border=BORDER_CONSTANT,
                  border_value=DEFAULT_BORDER_VALUE):
    img = np.ascontiguousarray(img, np.uint8)
    elem = None if elem is None else (np.asarray(elem) != 0).astype(np.uint8)
    if op == ERODE:
        return morph_op(img, False, elem, anchor, iterations, border, border_value)
    if op == DILATE:
        return morph_op(img, True, elem, anchor, iterations, border, border_value)
    assert op in (OPEN, CLOSE)
    first = op == CLOSE
    t = morph_op(img, first, elem, anchor, iterations, border, border_value)
    return morph_op(t, not first, elem, anchor, iterations, border, border_value)
