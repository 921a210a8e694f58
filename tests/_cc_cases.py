"""The recorded connectedComponentsWithStats cases (tests/golden/reference_cc.npz): image generators and the case
table.  tools/record_reference_cases.py records them; the oracle and GPU tests regenerate the images from here."""
import functools

import numpy as np

from _frontend_oracle import pattern

CCL_WU, CCL_DEFAULT, CCL_GRANA = 0, -1, 1
TYPE_NAMES = {CCL_DEFAULT: "default", CCL_WU: "wu", CCL_GRANA: "grana"}
WHOLE_LIMIT = 2048  # bytes: larger label images are stored as row CRCs (stats, centroids and N always whole)

SMALL = ((1, 1), (9, 1), (1, 7), (2, 2), (3, 3), (17, 13))  # (width, height)


def noise(w, h, density, seed, values=(255,)):
    p = pattern(w, h, 1, seed)
    v = np.array(values, np.uint8)[pattern(w, h, 1, seed + 1).astype(np.int32) % len(values)]
    return np.where(p < int(round(density * 256)), v, 0).astype(np.uint8)


def comb(w, h):
    """teeth in every second column, joined only by the last row: the unions come late"""
    img = np.zeros((h, w), np.uint8)
    img[:, ::2] = 255
    img[h - 1, :] = 255
    return img


def spiral(w, h):
    """two interleaved arms over the whole image: the rectangular rings at depths 0, 4, 8, .. joined through
    bridges at the top, those at depths 2, 6, 10, .. through bridges at the bottom, every ring cut where the other
    arm's bridge crosses it.  Each arm is one long winding path: the longest parent chains"""
    y, x = np.mgrid[0:h, 0:w]
    k = np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y))
    img = np.where(k % 2 == 0, np.where(k % 4 == 0, 255, 200), 0).astype(np.uint8)
    cx = w // 2
    for d in range(0, min(w, h) // 2 - 4, 4):
        # arm A's bridge from ring d to ring d + 4, through ring d + 2 at the top
        img[d + 2, cx - 1:cx + 2] = 0
        img[d + 1:d + 4, cx] = 255
        # arm B's bridge from ring d + 2 to ring d + 6, through ring d + 4 at the bottom
        if d + 6 < min(w, h) // 2:
            img[h - 1 - (d + 4), cx - 1:cx + 2] = 0
            img[h - 1 - (d + 5):h - 1 - (d + 2), cx] = 200
    return img


def diagonals(w, h):
    """both diagonals of the largest centred square: one component each way at 8, single pixels at 4"""
    img = np.zeros((h, w), np.uint8)
    n = min(w, h)
    i = np.arange(n)
    img[i, i] = 255
    img[i, n - 1 - i] = 255
    return img


def order(w, h):
    """components starting at (row 1, col 0) and at (row 0, col 2), repeated every 4 columns and 3 rows: the pixel
    scan numbers the second first, the block scan the first"""
    img = np.zeros((h, w), np.uint8)
    img[1::3, 0::4] = 255
    img[0::3, 2::4] = 255
    return img


@functools.lru_cache(maxsize=None)
def mog2_mask():
    """the mask of frame 30 (0-based) of the base _mog2_cases sequence, gray, history 12, through the restatement:
    0 / 127 / 255, the shadow value counting as foreground"""
    import _mog2_oracle as MO

    return np.ascontiguousarray(MO.expected(0)[0][30])


def image(content, w, h):
    if content == "zero":
        return np.zeros((h, w), np.uint8)
    if content == "full":
        return np.full((h, w), 255, np.uint8)
    if content == "checker":
        y, x = np.mgrid[0:h, 0:w]
        return (((x + y) % 2 == 0) * 255).astype(np.uint8)
    if content.startswith("noise"):
        return noise(w, h, float(content[5:]), 5100 + w + 3 * h)
    if content == "values":
        return noise(w, h, 0.5, 5200 + w + 3 * h, (1, 127, 255))
    if content == "mog2":
        assert (w, h) == (64, 48)
        return mog2_mask()
    return {"comb": comb, "spiral": spiral, "diagonals": diagonals, "order": order}[content](w, h)


def contents():
    """(content, shapes)"""
    return (
        ("zero", SMALL + ((130, 121),)),
        ("full", SMALL + ((130, 121),)),
        ("checker", SMALL + ((64, 48),)),
        ("noise0.3", ((3, 3), (17, 13), (67, 23), (300, 5))),
        ("noise0.5", ((3, 3), (17, 13), (67, 23), (64, 48))),
        ("noise0.6", ((3, 3), (17, 13), (67, 23), (130, 121))),
        ("comb", ((9, 1), (1, 7), (17, 13), (130, 121), (300, 5))),
        ("spiral", ((17, 13), (67, 23), (130, 121))),
        ("diagonals", ((3, 3), (17, 13), (64, 48))),
        ("order", ((3, 3), (17, 13), (67, 23))),
        ("values", ((17, 13), (67, 23))),
        ("mog2", ((64, 48),)),
    )


def cases():
    """(content, w, h, connectivity, ccltype)"""
    return [(c, w, h, conn, t) for c, shapes in contents() for (w, h) in shapes for conn in (4, 8)
            for t in (CCL_DEFAULT, CCL_WU, CCL_GRANA)]


def label(i):
    c, w, h, conn, t = cases()[i]
    return f"{c} {w}x{h} connectivity {conn} {TYPE_NAMES[t]}"


def stored_labels(labels):
    """a label image as the fixture holds it: whole (2-D) up to WHOLE_LIMIT bytes, else one CRC-32 per row, as
    int32 words (1-D)"""
    import _reference_cases as RC

    labels = np.ascontiguousarray(labels, np.int32)
    return labels if labels.nbytes <= WHOLE_LIMIT else RC.row_crcs(labels).view(np.int32)


def stored_stats(stats, centroids):
    """(N, 9) int32: the stats row, then the two centroids' 64-bit words (little-endian halves)"""
    stats = np.ascontiguousarray(stats, np.int32)
    cent = np.ascontiguousarray(centroids, np.float64).view(np.int32).reshape(len(stats), 4)
    return np.ascontiguousarray(np.concatenate([stats, cent], 1))


def unpack_stats(s):
    """stored_stats' inverse: (N, stats, centroids)"""
    s = np.ascontiguousarray(s, np.int32)
    return len(s), s[:, :5].copy(), np.ascontiguousarray(s[:, 5:]).view(np.float64).reshape(len(s), 2)
