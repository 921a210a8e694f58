"""Inputs of the whole-frame GFTT tests and the cases of
tests/golden/reference_gftt_frame.npz: goodFeaturesToTrack on whole frames,
most of them with more candidates than the LDS selection holds (16384), recorded
from the real reference by `tools/record_reference_cases.py <driver> gftt_frame`
(tools/record_reference_cases.md).  Every input is generated or read from
basketball_pair.npz; none is stored.

The fixture follows tests/_reference_cases.py's layout (`state`,
`other_ints_equal`, ...); `<i>_c` is the corner list of case i, whole, as int16
pairs (positions are integers below 2048)."""
import functools

import numpy as np

import _gftt_f32_cases as FC
import _gftt_mask_cases as MC
import _oracle as O
import _reference_cases as RC

HARRIS_K = 0.04
LDS_CAP = 16384  # kGfttCap: the candidates gftt_select_kernel holds at most


@functools.lru_cache(maxsize=None)
def frame(name):
    """the frame of a name (shared: read only)"""
    if name == "noise":  # 640 x 480 uniform noise
        f = np.random.default_rng(123).integers(0, 256, (480, 640), dtype=np.uint8)
    elif name == "kitti":  # a KITTI-shaped synth frame
        f = np.ascontiguousarray(O.synth(20261015, 1242, 375, 64, 0, 1)[0][0])
    elif name == "bench":  # the benchmark's own 1080p frame
        f = np.ascontiguousarray(O.synth(20261015, 1920, 1080, 128, 0, 1)[0][0])
    elif name == "basketball":
        f = np.ascontiguousarray(RC.basketball()[0])
    elif name == "unit":  # float32 in [0, 1): tests/_gftt_f32_cases.py's 640 x 480 frame
        f = np.array(FC.frame("unit"))
    else:
        raise ValueError(name)
    f.setflags(write=False)
    return f


def tiled_noise():
    """a 64 x 48 noise block tiled 10 x 10 to 640 x 480, with a flat band: every
    response value about a hundred times, so ties meet every chunk boundary"""
    block = np.random.default_rng(5).integers(0, 256, (48, 64), dtype=np.uint8)
    img = np.tile(block, (10, 10))
    img[100:140, 50:300] = 77  # flat band: ties and empty regions
    return img


def tiled_block():
    """a 4 x 4 block tiled over 640 x 480: away from the border every tile's
    strongest pixel has the same response, so nearly all candidates tie exactly"""
    return np.tile(np.random.default_rng(11).integers(0, 256, (4, 4), dtype=np.uint8), (120, 160))


# the mixed batch of tests/test_gpu_gftt_frame.py on the noise frame: (x, y, w, h, overflows the LDS selection)
MIXED_ROIS = [(0, 0, 640, 480, True), (100, 200, 200, 150, False), (0, 0, 3, 3, False), (5, 5, 2, 50, False),
              (100, 100, 1, 1, False), (40, 10, 600, 470, True)]
MIXED_ROW = (1500, 0.01, 2.5)


def mask(kind, name):
    """the mask of a kind of tests/_gftt_mask_cases.py for a frame (none: no mask)"""
    if kind == "none":
        return None
    f = frame(name)
    return MC.make(kind, f)


# (frame, mask kind, maxCorners, quality, minDistance, block, harris, overflows the LDS selection)
CASES = [
    ("noise", "none", 1000, 0.01, 0.0, 3, 0, True),
    ("noise", "none", 700, 0.01, 4.0, 3, 0, True),
    ("noise", "none", 500, 0.01, 10.0, 3, 0, True),
    ("noise", "none", 25000, 0.001, 0.0, 3, 0, True),
    ("kitti", "none", 4000, 0.01, 1.5, 3, 0, True),
    ("kitti", "checker", 4000, 0.01, 1.5, 3, 0, False),  # half the frame: below the capacity
    ("bench", "none", 8000, 0.01, 0.0, 3, 0, True),
    ("bench", "none", 4000, 0.01, 10.0, 3, 0, True),
    ("basketball", "none", 1000, 0.01, 0.0, 3, 0, False),
    ("unit", "none", 256, 0.01, 3.0, 3, 0, False),
    ("noise", "none", 500, 0.01, 2.0, 3, 1, True),
    ("noise", "none", 500, 0.01, 2.0, 5, 0, True),
]


def label(i):
    name, mk, maxc, q, md, block, harris, _ = CASES[i]
    return f"{name}" + (f" mask {mk}" if mk != "none" else "") + f" ({maxc}, {q}, {md}) block {block}" + \
        (" harris" if harris else "")


def index(name, mk, maxc, q, md, block=3, harris=0):
    """the case of these parameters"""
    for i, c in enumerate(CASES):
        if c[:7] == (name, mk, maxc, q, md, block, harris):
            return i
    raise KeyError((name, mk, maxc, q, md, block, harris))


def fixture():
    return RC.fixture("gftt_frame")


def corners(fx, i):
    """case i's recorded list as the float32 (K, 2) array the entry points return"""
    return fx[f"{i}_c"].astype(np.float32).reshape(-1, 2)
