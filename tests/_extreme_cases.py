"""Saturated, flat and periodic 8-bit pictures for the pixel kernels (pure
numpy, deterministic).  tests/test_extreme_cases.py proves on the CPU oracles
that each picture does what tests/test_gpu_extreme.py relies on it for.

Default sizes: 160x120 for sparse LK and GFTT, 96x64 for dense LK, 97x61 for
Farneback and the warps, 96x160 for HOG."""
from __future__ import annotations

import numpy as np

LK_SIZE = (160, 120)
DENSE_SIZE = (96, 64)
SMALL_SIZE = (97, 61)
HOG_SIZE = (96, 160)

NAMES = ("zero", "full", "vstripe2", "hstripe2", "check1", "check2", "blocks", "binary", "binblk", "quadrant",
         "impulse", "hole", "ramp")
PAIRS = ("same", "shift", "inverted")
# min-eigenvalue exactly 0 in every window: flat, one-directional or derivative-free content
SINGULAR = ("zero", "full", "vstripe2", "hstripe2", "check1")
# no trackable point and no corner at any size: those, and ramp (a function of x alone, cliff included)
FEATURELESS = SINGULAR + ("ramp",)


def patterns(w: int, h: int) -> dict[str, np.ndarray]:
    """name -> (h, w) uint8 picture"""
    y, x = np.mgrid[0:h, 0:w]
    u8 = lambda m: (np.asarray(m) != 0).astype(np.uint8) * 255  # noqa: E731
    rng = np.random.default_rng(20261020)
    binary = rng.integers(0, 2, (h, w))
    cells = rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4))
    impulse = np.zeros((h, w), np.uint8)
    impulse[h // 2, w // 2] = 255
    return {
        "zero": np.zeros((h, w), np.uint8),
        "full": np.full((h, w), 255, np.uint8),
        "vstripe2": u8((x >> 1) & 1),
        "hstripe2": u8((y >> 1) & 1),
        "check1": u8((x + y) & 1),
        "check2": u8(((x >> 1) + (y >> 1)) & 1),
        "blocks": u8(((x // 5) + (y // 7)) & 1),
        "binary": u8(binary),
        "binblk": u8(cells.repeat(4, 0).repeat(4, 1)[:h, :w]),
        "quadrant": u8((x >= w // 2) ^ (y >= h // 2)),
        "impulse": impulse,
        "hole": 255 - impulse,
        "ramp": (x & 255).astype(np.uint8),
    }


def pair(a: np.ndarray, kind: str) -> np.ndarray:
    """the second frame of a pair whose first frame is `a`"""
    if kind == "same":
        return a
    s = np.roll(a, (1, 2), (0, 1))
    if kind == "shift":
        return s
    assert kind == "inverted", kind
    return 255 - s  # |J - I| is 255 wherever `a` and its shift agree: the largest mismatch sums


def to_u16(a: np.ndarray, top: int) -> np.ndarray:
    """0 / 255 -> 0 / top (uint16); other values scale linearly, rounded down"""
    return (a.astype(np.uint32) * top // 255).astype(np.uint16)


def to_cn(a: np.ndarray, cn: int) -> np.ndarray:
    """(h, w) -> (h, w, cn): a, roll(a, 1 along x), 255 - a, 255 - roll: channels in anti-phase"""
    r = np.roll(a, 1, 1)
    return np.ascontiguousarray(np.stack([a, r, 255 - a, 255 - r][:cn], 2))


def grid(w: int, h: int) -> np.ndarray:
    """the 9-pixel grid at integer positions (margin 4)"""
    ys, xs = np.mgrid[4:h - 4:9, 4:w - 4:9]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


def edge_points(w: int, h: int) -> np.ndarray:
    """test_lk_edge_points_and_flags' points, placed relative to a w x h frame"""
    return np.array([[-100, -100], [1e4, 5], [0, 0], [w - 0.1, h - 0.1], [-21.0, 50.0], [-20.5, 3.0],
                     [w + 10.0, h + 10.0], [w / 2 + 0.5, h / 2 + 0.5], [3.2, h - 2.1], [-10.0, -10.0],
                     [w + 19.0, h + 19.0], [-31.0, 80.0]], np.float32)


def points(w: int, h: int) -> np.ndarray:
    """the grid at +0.37, the same grid at integer positions (interpolation
    weights exactly 16384/0/0/0: the interpolated derivative is the raw Scharr
    value), and the edge points"""
    g = grid(w, h)
    return np.concatenate([g + np.float32(0.37), g, edge_points(w, h)])
