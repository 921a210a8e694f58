"""The recorded morphology cases (tests/golden/reference_morph.npz): images, structuring elements, the case table
and the getStructuringElement table.  tools/record_reference_cases.py records them; the oracle, host and GPU tests
regenerate the inputs from here."""
import numpy as np

from _frontend_oracle import pattern

ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
RECT, CROSS, ELLIPSE = 0, 1, 2
CONSTANT, REPLICATE, REFLECT, REFLECT_101 = 0, 1, 2, 4
OP_NAMES = {ERODE: "erode", DILATE: "dilate", OPEN: "open", CLOSE: "close"}
BORDER_NAMES = {CONSTANT: "constant", REPLICATE: "replicate", REFLECT: "reflect", REFLECT_101: "reflect101"}
WHOLE_LIMIT = 512  # bytes: larger outputs are stored as row CRCs

SIZES = ((1, 1), (9, 1), (1, 7), (5, 4), (37, 23), (130, 121), (300, 5))  # (width, height)


def image(w, h, content):
    """"noise": full-range hashed bytes; "mask": 0 / 127 / 255, about a third each, in 3-pixel blobs"""
    if content == "noise":
        return np.ascontiguousarray(pattern(w, h, 1, 4100 + w * 7 + h))
    assert content == "mask"
    p = pattern(w // 3 + 1, h // 2 + 1, 1, 4200 + w + h * 5).astype(np.int32) % 3
    p = np.repeat(np.repeat(p, 2, 0), 3, 1)[:h, :w]
    return np.ascontiguousarray(np.array([0, 127, 255], np.uint8)[p])


def _shape_element(shape, kw, kh, anchor):
    import _morph_oracle as MO  # the shapes' recorded bits are pinned by the strel table below

    return MO.structuring_element(shape, (kw, kh), anchor)


def _arbitrary(kw, kh, seed, zero_at=None):
    e = (pattern(kw, kh, 1, seed) > 110).astype(np.uint8)
    e[0, kw - 1] = 1  # never empty, never full
    e[kh - 1, 0] = 0
    if zero_at is not None:
        e[zero_at[1], zero_at[0]] = 0
    return e


def shaped():
    """name -> (shape, kw, kh, anchor) of the elements getStructuringElement makes; the recorder checks that the
    reference's own element equals the one used here"""
    out = {}
    for kw, kh in ((3, 3), (5, 5), (7, 3)):
        out[f"cross{kw}x{kh}"] = (CROSS, kw, kh, (-1, -1))
        out[f"cross{kw}x{kh}@0"] = (CROSS, kw, kh, (0, 0))
    for kw, kh in ((5, 5), (7, 7), (9, 5), (15, 15), (31, 31)):
        out[f"ellipse{kw}x{kh}"] = (ELLIPSE, kw, kh, (-1, -1))
    return out


def elements():
    """name -> (kh, kw) uint8 element, None for the reference's empty Mat"""
    out = {"null": None}
    for kw, kh in ((3, 3), (5, 5), (7, 1), (1, 7), (2, 2), (4, 6)):
        out[f"rect{kw}x{kh}"] = np.ones((kh, kw), np.uint8)
    for name, (shape, kw, kh, anchor) in shaped().items():
        out[name] = _shape_element(shape, kw, kh, anchor)
    out["arb5x4"] = _arbitrary(5, 4, 4301)
    out["arb6x5z"] = _arbitrary(6, 5, 4302, zero_at=(3, 2))  # a zero at its (centre) anchor
    return out


def cases():
    """dicts: w, h, content, elem (a name of elements()), anchor, it, border, bval, op, inplace"""
    rows, seen = [], set()

    def add(size, content, elem, op, anchor=(-1, -1), it=1, border=CONSTANT, bval=-1, inplace=False):
        key = (size, content, elem, op, anchor, it, border, bval, inplace)
        if key in seen:
            return
        seen.add(key)
        rows.append(dict(w=size[0], h=size[1], content=content, elem=elem, op=op, anchor=anchor, it=it,
                         border=border, bval=bval, inplace=inplace))

    names = [n for n in elements() if n != "null"]
    ops = (ERODE, DILATE, OPEN, CLOSE)
    # every element x every op
    for n in names:
        anchor = (0, 0) if n.endswith("@0") else (-1, -1)
        for op in ops:
            add((37, 23), "noise", n, op, anchor=anchor)
    # every image x both contents
    for k, size in enumerate(SIZES):
        for c, content in enumerate(("noise", "mask")):
            for e, n in enumerate(("rect3x3", "ellipse5x5", "arb5x4")):
                add(size, content, n, (ERODE, DILATE)[(k + c + e) % 2], border=REFLECT_101)
                add(size, content, n, (OPEN, CLOSE)[(k + c + e) % 2])
    # borders and explicit border values, on an image smaller than the element too
    for size in ((5, 4), (37, 23)):
        for border in (CONSTANT, REPLICATE, REFLECT, REFLECT_101):
            for bval in (-1, 0, 100, 255):
                for n in ("ellipse7x7", "rect5x5"):
                    for op in (ERODE, DILATE):
                        add(size, "noise", n, op, border=border, bval=bval)
            add(size, "mask", "arb6x5z", OPEN, border=border, bval=100)
            add(size, "mask", "arb6x5z", CLOSE, border=border)
    # iterations
    for it in (0, 1, 2, 3):
        for n in ("rect3x3", "cross3x3", "arb5x4", "null", "rect2x2"):
            for op in (ERODE, DILATE):
                add((37, 23), "noise", n, op, it=it)
        add((37, 23), "mask", "cross3x3", OPEN, it=it)
        add((37, 23), "mask", "null", CLOSE, it=it)
    for size in ((5, 4), (130, 121)):
        for op in ops:
            add(size, "noise", "rect3x3", op, it=15)  # merges to 31 x 31, the limit
    # where one pass of the merged rectangle and iterating differ
    for border in (CONSTANT, REPLICATE):
        add((37, 23), "noise", "rect3x3", ERODE, it=2, border=border, bval=0)
        add((37, 23), "noise", "rect3x3", DILATE, it=2, border=border, bval=255)
        add((37, 23), "noise", "cross3x3", ERODE, it=2, border=border, bval=0)
    add((37, 23), "noise", "rect4x6", ERODE, anchor=(0, 0), it=2, bval=0)
    add((37, 23), "noise", "rect4x6", DILATE, anchor=(3, 5), it=3, bval=255)
    # anchors at the corners
    for n in ("rect4x6", "ellipse9x5", "arb5x4", "cross7x3", "rect2x2"):
        e = elements()[n]
        for anchor in ((0, 0), (e.shape[1] - 1, e.shape[0] - 1)):
            for size in ((5, 4), (37, 23)):
                for op in (ERODE, DILATE):
                    add(size, "noise", n, op, anchor=anchor, border=REFLECT)
            add((37, 23), "mask", n, OPEN, anchor=anchor)
    # more than one tile each way, wide elements
    for n in ("ellipse31x31", "ellipse15x15", "rect5x5", "arb6x5z", "rect7x1", "rect1x7"):
        for op in ops:
            add((130, 121), "noise", n, op, border=REFLECT_101 if op in (ERODE, CLOSE) else CONSTANT)
        add((300, 5), "mask", n, ERODE, border=REPLICATE)
        add((300, 5), "noise", n, CLOSE)
    # where one pass of the merged rectangle and iterating do differ: an off-centre anchor under a reflecting border
    for border in (REFLECT, REFLECT_101):
        add((37, 23), "noise", "rect4x6", ERODE, anchor=(0, 0), it=2, border=border)
        add((37, 23), "noise", "rect4x6", DILATE, anchor=(3, 5), it=2, border=border)
        add((37, 23), "noise", "rect2x2", ERODE, it=2, border=border)
        add((5, 4), "noise", "rect2x2", DILATE, it=3, border=border)
    # in place
    add((130, 121), "noise", "ellipse7x7", ERODE, inplace=True)
    add((37, 23), "mask", "rect3x3", OPEN, inplace=True)
    return rows


def label(i):
    c = cases()[i]
    return "{}x{} {} {} {} anchor {} it {} {} bval {}{}".format(
        c["w"], c["h"], c["content"], OP_NAMES[c["op"]], c["elem"], c["anchor"], c["it"], BORDER_NAMES[c["border"]],
        c["bval"], " in place" if c["inplace"] else "")


# ---- getStructuringElement ------------------------------------------------------------------------------------

def strel_cases():
    """(shape, kw, kh, anchor): every ELLIPSE 1..31 square plus three oblong ones, CROSS with three anchors"""
    rows = [(ELLIPSE, k, k, (-1, -1)) for k in range(1, 32)]
    rows += [(ELLIPSE, 9, 5, (-1, -1)), (ELLIPSE, 5, 9, (-1, -1)), (ELLIPSE, 31, 3, (-1, -1))]
    rows += [(CROSS, 7, 5, (-1, -1)), (CROSS, 7, 5, (0, 0)), (CROSS, 7, 5, (6, 4)), (RECT, 4, 6, (-1, -1))]
    return rows
