"""Small images whose rows span 2 GiB and 4 GiB: the arena and the protocol of
tests/test_gpu_far_views.py (numpy only until a device function is called, so
tests/test_far_cases.py checks the arithmetic without a GPU).

include/tbdk.h ("image layout") takes any pitch >= a row, and a pitch is an int:
a 97 x 40 view with a pitch of 100 MB is legal (a column crop of a mosaic, a
plane of a huge interleaved surface).  Every other test keeps the byte offset of
a pixel from its image's first byte far below 2^31, so a row offset computed in
32 bits passes them all.  Here only the pitch grows.

Layouts, for an image of h rows (h >= 32) of `row` bytes whose pitch must be a
multiple of `unit` bytes:
  under_2g  P = the largest pitch with (h - 1) * P + row <= 2^31 - 1; then
            h * P > 2^31: the extent fits 31 bits, pitch * height does not
  over_2g   P = ceil(2^31 / (h - 8)) rounded up to unit: the last 8 rows start
            at or beyond 2^31, the rest below it
  over_4g   the same for 2^32
P stays below 2^31 and the extent below 1.3 * 2^32.

The arena keeps a wrong address inside the allocation.  One device allocation:
a low guard of 4 GiB, the image span of 5.5 GiB, a high guard of 1 MiB, all
filled with the byte 0x5A (finite in fp16 and fp32).  Every image of a call is
a rectangle of the span at its own column offset.  A true byte offset here is
below 2^33, so whatever is computed in 32 bits, signed or unsigned, differs from
it by exactly 2^32 downward, and a 32-bit product that is then sign-extended
lands at most 2 GiB below the image base; element indices cannot wrap at this
span for elements of 2 bytes or more; a wrapped offset is never above the true
one.  So every address a wrong kernel can form lies inside the arena, and a
defect shows as a wrong result or a changed poison byte, never as a fault.
separated() holds that no rectangle comes within 4096 bytes of another, or of
another's rows shifted by 2^31 or 2^32, so a wrapped access cannot land on data
that happens to be right.

Protocol (test_gpu_far_views.py run_far): place the far images, copy the inputs
in, call, clone the outputs, overwrite every rectangle with poison, scan the
whole arena in chunks of 512 MiB for a byte that is not poison (a failure that
names its offset from each image base, and that offset modulo 2^32), then run the
entry point's oracle comparison on the clones.  The scan leaves the arena all
poison for the next test."""
from dataclasses import dataclass

import numpy as np

import _views as V

GIB = 1 << 30
LOW_GUARD = 4 * GIB
SPAN = 11 * GIB // 2
HIGH_GUARD = 1 << 20
ARENA_BYTES = LOW_GUARD + SPAN + HIGH_GUARD
NEED_FREE = 14 * GIB
POISON = 0x5A
CHUNK = 512 << 20
SEPARATION = 4096
MIN_ROWS = 32
EDGE_ROWS = 8
SLOT = 1 << 16  # column offsets are slot * SLOT + the residue of a tests/_views.py layout
LAYOUTS = ("under_2g", "over_2g", "over_4g")
BOUNDARY = {"under_2g": 1 << 31, "over_2g": 1 << 31, "over_4g": 1 << 32}
SHIFTS = (0, 1 << 31, 1 << 32)
RESIDUE = "odd_both"  # the default of _views.LAYOUTS' five


def pitch_of(layout, h, row, unit):
    """the layout's pitch in bytes for h rows of `row` bytes, a multiple of `unit`"""
    assert h >= MIN_ROWS and row > 0 and unit in (1, 2, 4, 8) and row % unit == 0, (h, row, unit)
    if layout == "under_2g":
        p = ((1 << 31) - 1 - row) // (h - 1)
        return p - p % unit
    p = -(-BOUNDARY[layout] // (h - EDGE_ROWS))
    return p + (-p) % unit


def extent(h, pitch, row):
    """bytes from the image's first byte to the end of its last row's pixels"""
    return (h - 1) * pitch + row


@dataclass(frozen=True)
class Rect:
    """one image in the span: rows of `row` bytes, `pitch` apart, the first at span offset `col`"""
    name: str
    col: int
    h: int
    row: int
    pitch: int
    unit: int

    @property
    def extent(self):
        return self.col + extent(self.h, self.pitch, self.row)

    def starts(self):
        return self.col + np.arange(self.h, dtype=np.int64) * self.pitch


def gap(a, b, shift=0):
    """the fewest bytes between a row of a and a row of b moved `shift` bytes down (<= 0: they overlap)"""
    sa, sb = a.starts()[:, None], b.starts()[None, :] - shift
    return int(np.maximum(sb - (sa + a.row), sa - (sb + b.row)).min())


def separated(rects):
    """no two rectangles within SEPARATION bytes of each other, or of the other's rows shifted by 2^31 or 2^32"""
    for i, a in enumerate(rects):
        for b in rects[i + 1:]:
            for s in SHIFTS:
                if gap(a, b, s) < SEPARATION or (s and gap(b, a, s) < SEPARATION):
                    return False
    return True


def column(slot, unit, residue=RESIDUE):
    return slot * SLOT + V.layout_of(residue, unit, 1)[0]


def place(images, layout, residue=RESIDUE, pitches=None, taken=()):
    """Rects for `images` = [(name, h, row bytes, unit)], each at the first column slot that keeps it separated
    from the ones before it (and from `taken`).  Images that must share a pitch (pitches: {name: group}) get
    their group's first pitch; they must have the same rows."""
    out, slot, group = list(taken), 0, {}
    for name, h, row, unit in images:
        p = pitch_of(layout, h, row, unit)
        g = (pitches or {}).get(name)
        if g is not None:
            p = group.setdefault(g, p)
        while True:
            r = Rect(name, column(slot, unit, residue), h, row, p, unit)
            slot += 1
            if separated(out + [r]):
                break
            assert slot < 64, f"no column for {name}"
        assert r.extent <= SPAN, (name, r.extent)
        out.append(r)
    return out[len(taken):]


def with_pitch(rect, pitch):
    return Rect(rect.name, rect.col, rect.h, rect.row, pitch, rect.unit)


# ---- the device side ------------------------------------------------------------------------------------------------

_state = {}


def arena():
    """the session's arena (one allocation, all poison), or a pytest skip naming the free memory"""
    import pytest
    import torch

    if "arena" not in _state:
        free = torch.cuda.mem_get_info()[0]
        if free < NEED_FREE:
            pytest.skip(f"the far-view arena needs {NEED_FREE / GIB:.0f} GiB free, the device has {free / GIB:.1f} GiB")
        a = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
        assert a.data_ptr() % 256 == 0
        a.fill_(POISON)
        _state["arena"] = a
    return _state["arena"]


def release():
    import torch

    _state.pop("arena", None)
    torch.cuda.empty_cache()


def view(rect, shape, dtype):
    """the torch view of `rect`: `shape` = (h, w) or (h, w, c) of `dtype`, rows rect.pitch bytes apart"""
    import torch

    a = arena()
    es = torch.empty((), dtype=dtype).element_size()
    inner = int(np.prod(shape[1:]))
    assert shape[0] == rect.h and inner * es == rect.row and rect.pitch % es == 0 and (LOW_GUARD + rect.col) % es == 0
    typed = a if es == 1 else a.view(dtype)
    strides = (rect.pitch // es,) + tuple(int(np.prod(shape[k + 1:])) for k in range(1, len(shape)))
    return torch.as_strided(typed, tuple(shape), strides, (LOW_GUARD + rect.col) // es)


def _rows(rect):
    a = arena()
    for y in range(rect.h):
        o = LOW_GUARD + rect.col + y * rect.pitch
        yield a[o:o + rect.row]


def put(rect, src):
    """a contiguous device tensor of the rectangle's size into it, row by row (each copy is a small contiguous one)"""
    import torch

    flat = (src.view(torch.int16) if src.dtype == torch.uint16 else src).contiguous().view(torch.uint8).reshape(rect.h, rect.row)
    for y, r in enumerate(_rows(rect)):
        r.copy_(flat[y])


def get(rect):
    """the rectangle's bytes as a contiguous (h, row) uint8 clone"""
    import torch

    return torch.stack(list(_rows(rect)))


def poison(rect):
    for r in _rows(rect):
        r.fill_(POISON)


def scan(rects, what):
    """every byte of the arena is poison, or an AssertionError naming the first stray byte's offset from each image
    base and that offset modulo 2^32; the stray bytes are overwritten first, so the arena is all poison after"""
    import torch

    a = arena()
    words = a.view(torch.int64)
    pat = int.from_bytes(bytes([POISON]) * 8, "little")
    step = CHUNK // 8
    flags = torch.stack([(words[o:o + step] != pat).any() for o in range(0, words.numel(), step)]).cpu().numpy()
    if not flags.any():
        return
    k = int(np.flatnonzero(flags)[0])
    chunk = a[k * CHUNK:(k + 1) * CHUNK]
    first = k * CHUNK + int(torch.nonzero(chunk != POISON)[0])
    count = sum(int((a[j * CHUNK:(j + 1) * CHUNK] != POISON).sum()) for j in np.flatnonzero(flags))
    for j in np.flatnonzero(flags):
        a[j * CHUNK:(j + 1) * CHUNK].fill_(POISON)
    where = "; ".join(f"{r.name} base {first - LOW_GUARD - r.col:+d} (mod 2^32: {(first - LOW_GUARD - r.col) % (1 << 32)})"
                      for r in rects)
    raise AssertionError(f"{what}: {count} byte(s) outside every image changed; the first at arena offset {first}, "
                         f"span offset {first - LOW_GUARD:+d}: {where}")
