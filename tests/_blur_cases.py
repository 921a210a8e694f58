"""The recorded GaussianBlur and threshold cases (tests/golden/reference_blur.npz, reference_threshold.npz): images,
kernels, the case tables and the coefficient sweep.  tools/record_reference_cases.py records them; the oracle, host
and GPU tests regenerate the inputs from here."""
import numpy as np

import _blur_oracle as BO
from _frontend_oracle import pattern

CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
BORDERS = (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101)
WHOLE_LIMIT = 512  # bytes: larger outputs are stored as row CRCs

SMALL = ((1, 1), (9, 1), (1, 7), (5, 4))  # (width, height)
LARGE = ((130, 121), (300, 5))


def image(w, h, content, cn=1):
    """"noise": full-range hashed bytes; "runs": 0 / 127 / 255 in blocks 40 wide and 9 high, so that 255-filled runs
    are longer than the largest kernel; "mog2": frame 30's mask of the base MOG2 sequence (64 x 48)"""
    if content == "noise":
        return np.ascontiguousarray(pattern(w, h, cn, 5100 + w * 7 + h + cn * 31))
    assert cn == 1
    if content == "runs":
        p = pattern(w // 40 + 1, h // 9 + 1, 1, 5200 + w + h * 5).astype(np.int32) % 3
        p[0, 0], p[-1, -1] = 2, 2
        p = np.repeat(np.repeat(p, 9, 0), 40, 1)[:h, :w]
        return np.ascontiguousarray(np.array([0, 127, 255], np.uint8)[p])
    assert content == "mog2" and (w, h) == (64, 48)
    import _cc_cases as LC

    return LC.mog2_mask()


# ---- the coefficient sweep ------------------------------------------------------------------------------------

SWEEP_STEP = 0.0837  # aligned with nothing


def sweep_pairs():
    """(n, sigma): n odd 3..31, sigma 0 and 0.3 to 12"""
    sig = [0.0] + [0.3 + j * SWEEP_STEP for j in range(140)]
    assert sig[-1] < 12.0 < sig[-1] + SWEEP_STEP
    return [(n, s) for n in range(3, 32, 2) for s in sig]


SWEEP_W, SWEEP_P0, SWEEP_P1, SWEEP_V0, SWEEP_V1 = 128, 32, 96, 255, 128


def sweep_image():
    """one row, two impulses further apart than the widest kernel.  With the column kernel collapsed to one tap of
    256 the response to an impulse v at tap k is (k v + 128) >> 8: for v = 255 that is k up to 128 and k - 1 above,
    so 128 and 129 both give 128; v = 128 gives (k + 1) >> 1, 64 and 65 there.  Together they determine k."""
    img = np.zeros((1, SWEEP_W), np.uint8)
    img[0, SWEEP_P0], img[0, SWEEP_P1] = SWEEP_V0, SWEEP_V1
    return img


def sweep_response(k):
    """what the two windows of the response row hold for coefficients k: 2 n bytes"""
    k = np.asarray(k, np.int64)
    return np.concatenate([np.minimum((k * v + 128) >> 8, 255) for v in (SWEEP_V0, SWEEP_V1)]).astype(np.uint8)


def sweep_decode(resp, n):
    """the coefficients a recorded response of 2 n bytes determines; asserts that it determines them"""
    r0, r1 = resp[:n].astype(np.int64), resp[n:].astype(np.int64)
    out = []
    for a, b in zip(r0, r1):
        cand = [k for k in range(0, 512) if min((k * SWEEP_V0 + 128) >> 8, 255) == a and min((k * SWEEP_V1 + 128) >> 8, 255) == b]
        assert len(cand) == 1, (a, b, cand)
        out.append(cand[0])
    return np.array(out, np.uint16)


def largest_sum_sigma(n):
    """the sweep's sigma at which the n coefficients of the restatement sum to the most"""
    best = max((int(BO.gaussian_kernel_u8(m, s).sum()), -s) for m, s in sweep_pairs() if m == n)
    return -best[1]


# ---- GaussianBlur -----------------------------------------------------------------------------------------------

def kernels():
    """name -> (kw, kh, sigma_x, sigma_y)"""
    out = {}
    for n in (3, 5, 7):
        for s in (0.0, 0.8, 1.5):
            out[f"{n}@{s:g}"] = (n, n, s, 0.0)
    out["11@3.5"] = (11, 11, 3.5, 3.5)
    out["9@3.9"] = (9, 9, 3.9, 0.0)
    out["25@max"] = (25, 25, largest_sum_sigma(25), 0.0)
    out["31@0"] = (31, 31, 0.0, 0.0)
    out["31@5"] = (31, 31, 5.0, 0.0)
    out["7x1"] = (7, 1, 2.0, 0.7)
    out["1x7"] = (1, 7, 0.7, 2.0)
    out["5x11"] = (5, 11, 1.1, 2.7)
    out["auto1"] = (0, 0, 1.0, 0.0)
    out["auto2.2"] = (0, 0, 2.2, 0.0)
    return out


_CASES = None


def cases():
    """dicts: w, h, cn, content, kernel (a name of kernels()), border, inplace"""
    global _CASES
    if _CASES is not None:
        return _CASES
    rows, seen = [], set()

    def add(size, content, kernel, border, cn=1, inplace=False):
        key = (size, content, kernel, border, cn, inplace)
        if key in seen:
            return
        seen.add(key)
        rows.append(dict(w=size[0], h=size[1], cn=cn, content=content, kernel=kernel, border=border, inplace=inplace))

    names = list(kernels())
    for size in SMALL:
        for border in BORDERS:
            for k in ("3@0", "5@0.8", "7@1.5", "11@3.5", "31@0", "7x1", "5x11", "auto1"):
                add(size, "noise", k, border)
    for border in BORDERS:
        for k in ("3@0", "5@0", "7@0", "9@3.9", "25@max"):
            add((37, 23), "noise", k, border)
    for size in ((37, 23),) + LARGE:
        for j, k in enumerate(names):
            add(size, "noise", k, REFLECT_101)
            add(size, "noise", k, (CONSTANT, REPLICATE, REFLECT, WRAP)[j % 4])
    for size, content in (((130, 121), "runs"), ((64, 48), "mog2")):
        for j, k in enumerate(("11@3.5", "9@3.9", "25@max", "31@5", "3@0", "5@1.5")):
            add(size, content, k, REFLECT_101)
            add(size, content, k, (REPLICATE, CONSTANT)[j % 2])
    for cn in (3, 4):
        for size in ((37, 23), (130, 121)):
            for j, k in enumerate(("3@0", "5@0.8", "7@0", "11@3.5", "25@max", "5x11")):
                add(size, "noise", k, REFLECT_101, cn=cn)
                add(size, "noise", k, (CONSTANT, WRAP, REFLECT)[j % 3], cn=cn)
    add((130, 121), "noise", "11@3.5", REFLECT_101, inplace=True)
    add((37, 23), "noise", "5@0", REPLICATE, cn=3, inplace=True)
    _CASES = rows
    return rows


def label(i):
    c = cases()[i]
    return "{}x{} cn {} {} {} {}{}".format(c["w"], c["h"], c["cn"], c["content"], c["kernel"],
                                           BO.BORDER_NAMES[c["border"]], " in place" if c["inplace"] else "")


def case_image(c):
    return image(c["w"], c["h"], c["content"], c["cn"])


SMOOTH_MASK = ("11@3.5", 10.0, 255.0, BO.BINARY)  # samples/cpp/bgfg_segm.cpp's smoothMask step


# ---- threshold --------------------------------------------------------------------------------------------------

THRESHOLDS = (-1.0, 0.0, 10.0, 127.5, 254.0, 255.0, 300.0)
MAXVALS = (255.0, 100.6, 300.0)
TYPES = (BO.BINARY, BO.BINARY_INV, BO.TRUNC, BO.TOZERO, BO.TOZERO_INV)
F32_SIZE = (32, 20)  # w * h a multiple of 16: every pixel goes through thresh_32f's vector body in both states


def f32_image():
    w, h = F32_SIZE
    a = (pattern(w, h, 1, 5300).astype(np.float32) - np.float32(100.0)) * np.float32(0.37)
    b = pattern(w, h, 1, 5301)
    a[b < 12] = np.nan
    a[(b >= 12) & (b < 20)] = np.inf
    a[(b >= 20) & (b < 28)] = -np.inf
    a[0, 0], a[0, 1], a[0, 2] = np.float32(0.5), np.float32(-0.0), np.float32(0.0)
    return a


def otsu_image(name):
    if name == "noise":
        return image(37, 23, "noise")
    if name == "bimodal":
        a = pattern(64, 48, 1, 5400).astype(np.int32)
        b = pattern(64, 48, 1, 5401)
        return np.where(b < 100, 40 + a % 31, 170 + a % 47).astype(np.uint8)
    if name == "constant":
        return np.full((10, 20), 93, np.uint8)
    if name == "two":
        return np.where(pattern(33, 9, 1, 5402) < 60, 12, 201).astype(np.uint8)
    assert name == "mog2"
    return image(64, 48, "mog2")


OTSU_IMAGES = ("noise", "bimodal", "constant", "two", "mog2")


def thresh_cases():
    """dicts: kind ("u8", "f32", "otsu"), image (a size or a name), thresh, maxval, type"""
    rows = []
    for size in ((37, 23), (300, 5)):
        for t in TYPES:
            for th in THRESHOLDS:
                for mv in MAXVALS:
                    rows.append(dict(kind="u8", image=size, thresh=th, maxval=mv, type=t))
    for t in TYPES:
        for th in (0.5, -7.25, float("inf")):
            for mv in (1.0, 255.5):
                rows.append(dict(kind="f32", image=F32_SIZE, thresh=th, maxval=mv, type=t))
    for name in OTSU_IMAGES:
        for t in (BO.BINARY, BO.TOZERO_INV):
            rows.append(dict(kind="otsu", image=name, thresh=55.0, maxval=255.0, type=t | BO.OTSU))
    return rows


def thresh_image(c):
    if c["kind"] == "u8":
        return image(c["image"][0], c["image"][1], "noise")
    return f32_image() if c["kind"] == "f32" else otsu_image(c["image"])


def thresh_label(i):
    c = thresh_cases()[i]
    return "{} {} thresh {} maxval {} type {}".format(c["kind"], c["image"], c["thresh"], c["maxval"], c["type"])
