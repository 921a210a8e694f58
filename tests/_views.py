"""Pitched, unaligned image views for the layout tests (torch / numpy only, so
CPU tensors work too).

window(arr, layout, seed) puts `arr` into the interior of a larger allocation:
guard rows above and below, guard columns left and right, all filled with
seeded noise, so that a kernel that reads a guard byte as a pixel disagrees
with its oracle and a kernel that writes one is caught by guards_intact.  No
window touches the first or the last byte of its allocation: whatever a wrong
kernel reads or writes near the window stays inside the parent.

LAYOUTS names each layout by the code path it selects: the byte offset of the
window's first byte mod 16 and the byte pitch mod 16.  Offsets and pitches are
whole pixels (elements x channels), so for wider elements or several channels
the byte figures are the nearest a whole pixel allows; layout_of() gives the
figures a given element size and channel count really get.
"""
from collections import namedtuple

import numpy as np
import torch

Layout = namedtuple("Layout", "base pitch selects")

# name -> (first byte mod 16, byte pitch mod 16) for one-channel u8, and the path that selects
LAYOUTS = {
    "a16_pitched": Layout(0, 0, "16-byte path with pitch != row"),
    "vec4": Layout(4, 0, "dword path, not the 16-byte one"),
    "odd_base": Layout(1, 0, "scalar path through the base alone"),
    "odd_pitch": Layout(0, 5, "scalar path through the pitch alone"),
    "odd_both": Layout(3, 6, "neither aligned"),
}

GUARD_ROWS = 2
GUARD_RIGHT = 16  # bytes, at least
ALIGN = 64  # spare bytes at both ends of the allocation, outside the parent

_NP = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float16): torch.float16,
       np.dtype(np.float32): torch.float32}

# byte pitch mod 16 per element size where whole elements cannot give the u8 figure
_PITCH = {"odd_pitch": {1: 5, 2: 10, 4: 4}, "odd_both": {1: 6, 2: 6, 4: 12}}


def _left_pixels(name, esize, cn):
    """guard columns on the left, in whole pixels (at least one): a16_pitched and
    odd_pitch the fewest that give base 0, vec4 the fewest that give base 4 (if any),
    odd_base one pixel, odd_both three"""
    px = esize * cn
    if name == "odd_base":
        return 1
    if name == "odd_both":
        return 3
    want = LAYOUTS[name].base
    for n in range(1, 17):
        if (n * px) % 16 == want:
            return n
    return 1  # pixels of 8 or 16 bytes cannot give base 4: one pixel, the least misaligned offset there is


def layout_of(name, esize=1, cn=1):
    """(first byte mod 16, byte pitch mod 16) that `name` gives for elements of
    `esize` bytes and `cn` channels; LAYOUTS' own figures for one-channel u8"""
    return (_left_pixels(name, esize, cn) * esize * cn) % 16, _PITCH.get(name, {}).get(esize, LAYOUTS[name].pitch)


def _pitch_bytes(name, esize, cn, row, left_bytes):
    """smallest pitch >= left + row + GUARD_RIGHT with the layout's residue mod 16"""
    want = layout_of(name, esize, cn)[1]
    p = left_bytes + row + GUARD_RIGHT
    return p + (want - p) % 16


def window(arr, layout, seed=0, device="cpu", guard_rows=GUARD_ROWS):
    """(parent, view): `view` has arr's shape and content and is an interior
    window of the 1-D byte tensor `parent` (whose other bytes are seeded noise),
    with the layout's base offset and pitch; arr is (H, W) or (H, W, C), u8, u16,
    f16 or f32 (numpy)"""
    arr = np.ascontiguousarray(arr)
    assert arr.ndim in (2, 3) and arr.dtype in _NP, (arr.shape, arr.dtype)
    h, w = arr.shape[:2]
    cn = arr.shape[2] if arr.ndim == 3 else 1
    esize = arr.dtype.itemsize
    row = w * cn * esize
    left = _left_pixels(layout, esize, cn) * cn * esize
    pitch = _pitch_bytes(layout, esize, cn, row, left)
    rows = h + 2 * guard_rows
    rng = np.random.default_rng([seed, h, w, cn, esize])
    # noise that is a finite number in every element type: bytes 1..119 (fp16 / fp32 exponents stay below the top)
    host = rng.integers(1, 120, ALIGN + rows * pitch + ALIGN, dtype=np.uint8)
    raw = torch.from_numpy(host).to(device)
    start = guard_rows * pitch + left
    # the parent begins ALIGN..ALIGN+15 bytes into the allocation (never at its first byte), where the
    # window's first byte gets the layout's residue mod 16 whatever the guard rows above it add
    off = ALIGN + (layout_of(layout, esize, cn)[0] - (raw.data_ptr() + ALIGN + start)) % 16
    parent = raw[off:off + rows * pitch]
    typed = parent.view(_NP[arr.dtype]) if esize > 1 else parent
    strides = (pitch // esize, cn, 1) if arr.ndim == 3 else (pitch // esize, 1)
    view = torch.as_strided(typed, arr.shape, strides, typed.storage_offset() + start // esize)
    src = torch.from_numpy(arr.view(np.int16) if arr.dtype == np.uint16 else arr)
    if arr.dtype == np.uint16:
        view.view(torch.int16).copy_(src.to(device))
    else:
        view.copy_(src.to(device))
    return parent, view


def snapshot(parent):
    """the parent's bytes, to hand to guards_intact after the call"""
    return parent.clone()


def window_mask(parent, view):
    """bool tensor over the parent's bytes: True inside the window"""
    esize = view.element_size()
    pitch = view.stride(0) * esize
    row = view[0].numel() * esize
    start = view.data_ptr() - parent.data_ptr()
    m = torch.zeros(parent.numel(), dtype=torch.bool, device=parent.device)
    idx = (start + torch.arange(view.shape[0], device=parent.device)[:, None] * pitch +
           torch.arange(row, device=parent.device)[None, :])
    m[idx.reshape(-1)] = True
    return m


def guards_intact(parent, before, view):
    """True iff every byte of `parent` outside the window equals `before`"""
    out = ~window_mask(parent, view)
    return bool(torch.equal(parent[out], before[out]))


def margins(parent, view):
    """(rows above, rows below, bytes left, bytes right) of the window in its parent"""
    esize = view.element_size()
    pitch = view.stride(0) * esize
    row = view[0].numel() * esize
    start = view.data_ptr() - parent.data_ptr()
    top, left = divmod(start, pitch)
    return top, parent.numel() // pitch - top - view.shape[0], left, pitch - left - row


def host(view):
    """numpy copy of a view (uint16 through its int16 bits)"""
    if view.dtype == torch.uint16:
        return view.view(torch.int16).cpu().numpy().view(np.uint16)
    return view.cpu().numpy()
