"""numpy restatement of cv::connectedComponentsWithStats (imgproc/src/connectedcomponents.cpp), CV_32S labels:
a flood fill, then the components ranked by the key the reference's scan gives them, then CCStatsOp's stats.
Deliberately not a union-find; tests/test_cc_oracle.py holds it to the recordings.

The key: LabelingWu (CCL_WU, and connectivity 4 whatever the type) creates labels over pixels in raster order,
LabelingGrana (CCL_GRANA / CCL_DEFAULT at connectivity 8) over 2x2 blocks in block raster order; unions keep the
smaller label and flattenL numbers the roots in increasing order.  So a component's label is the rank of its first
pixel, or of its first block."""
import numpy as np

CCL_WU, CCL_DEFAULT, CCL_GRANA = 0, -1, 1
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def flood(fg, connectivity):
    """component ids (0 = background, 1.. in raster order of first pixels) by iterated minimum propagation
    along rows, columns and, for 8, diagonals"""
    fg = np.ascontiguousarray(fg)
    h, w = fg.shape
    big = h * w + 1
    lab = np.where(fg, np.arange(1, h * w + 1, dtype=np.int64).reshape(h, w), big)

    def sweep(a, f):  # every horizontal run of foreground takes its minimum
        flat, ff = a.reshape(-1), f.reshape(-1)
        start = ff.copy()
        start[1:] &= ~ff[:-1]
        start.reshape(f.shape)[:, 0] = f[:, 0]
        run = np.cumsum(start) - 1
        lo = np.full(int(start.sum()), big, np.int64)
        np.minimum.at(lo, run[ff], flat[ff])
        flat[ff] = lo[run[ff]]
        return flat.reshape(a.shape)

    while True:
        before = lab.copy()
        lab = sweep(np.ascontiguousarray(lab), fg)
        lab = np.ascontiguousarray(sweep(np.ascontiguousarray(lab.T), np.ascontiguousarray(fg.T)).T)
        if connectivity == 8:
            for dy, dx in ((1, 1), (1, -1)):
                a = lab[dy:, max(dx, 0):w + min(dx, 0)]
                b = lab[:h - dy, max(-dx, 0):w - max(dx, 0)]
                m = (a < big) & (b < big)
                lo = np.minimum(a, b)
                a[m] = lo[m]
                b[m] = np.minimum(b[m], lo[m])  # a and b overlap: b may just have been lowered through a
        if np.array_equal(before, lab):
            break
    ids = np.zeros((h, w), np.int64)
    roots = np.unique(lab[fg])
    ids[fg] = np.searchsorted(roots, lab[fg]) + 1
    return ids, len(roots)


def connected_components_with_stats(img, connectivity=8, ccltype=CCL_DEFAULT):
    """(N, labels int32, stats int32 [N][5], centroids float64 [N][2])"""
    assert connectivity in (4, 8) and ccltype in (CCL_WU, CCL_DEFAULT, CCL_GRANA)
    img = np.asarray(img)
    h, w = img.shape
    fg = img != 0
    ids, n = flood(fg, connectivity)
    ys, xs = np.nonzero(fg)
    comp = ids[ys, xs] - 1
    if connectivity == 8 and ccltype != CCL_WU:
        key = (ys // 2).astype(np.int64) * ((w + 1) // 2) + xs // 2
    else:
        key = ys.astype(np.int64) * w + xs
    first = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(first, comp, key)
    assert len(np.unique(first)) == n  # no two components share a key
    rank = np.empty(n, np.int64)
    rank[np.argsort(first)] = np.arange(n)
    labels = np.zeros((h, w), np.int32)
    labels[ys, xs] = rank[comp] + 1
    N = n + 1
    # CCStatsOp: init, one call per pixel, finish (int32 wraps, area read as unsigned, one double division)
    yy, xx = np.mgrid[0:h, 0:w]
    l = labels.ravel()
    minx, miny = np.full(N, INT_MAX, np.int64), np.full(N, INT_MAX, np.int64)
    maxx, maxy = np.full(N, INT_MIN, np.int64), np.full(N, INT_MIN, np.int64)
    np.minimum.at(minx, l, xx.ravel())
    np.minimum.at(miny, l, yy.ravel())
    np.maximum.at(maxx, l, xx.ravel())
    np.maximum.at(maxy, l, yy.ravel())
    area = np.bincount(l, minlength=N).astype(np.int64)
    sx = np.zeros(N, np.uint64)
    sy = np.zeros(N, np.uint64)
    np.add.at(sx, l, xx.ravel().astype(np.uint64))
    np.add.at(sy, l, yy.ravel().astype(np.uint64))
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)  # noqa: E731
    stats = np.stack([wrap(minx), wrap(miny), wrap(maxx - minx + 1), wrap(maxy - miny + 1), wrap(area)], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        centroids = np.stack([sx.astype(np.float64) / area.astype(np.float64),
                              sy.astype(np.float64) / area.astype(np.float64)], 1)
    return N, labels, stats, centroids


def same_centroids(a, b):
    """bit for bit, except that a NaN equals any NaN (the sign of 0/0 differs between x86 and the GPU)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())
