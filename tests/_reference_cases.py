"""Inputs, case tables and fixture access of tests/golden/reference_<op>.npz:
what the real reference returned, recorded by tools/record_reference_cases.py
(how: tools/record_reference_cases.md).  The recorder and the two pin suites
(tests/test_reference_pins.py on the CPU oracle, tests/test_gpu_reference_pins.py
on the kernels) all generate the inputs through this module, so a fixture
stores outputs only.

Every fixture carries `state`: the reference's runtime CPU dispatch state its
full recording was made under ("both" where the default dispatch and
OPENCV_CPU_DISABLE=AVX2,AVX512_SKX gave byte-identical recordings, else
"default" or "noavx2": the state the oracle file models).  Where the states
differ, `other_ints_equal[i]` says whether case i's integer-valued results
(corner lists, status, window positions, rects) were the same in the other
state (where not, `other_<i>_<name>` holds the other state's), and
`other_share[i]` / `other_maxabs[i]` give the share of equal 32-bit words and
the largest absolute difference of its float results.

An output is stored whole in its own dtype, or, where it is large, as one
CRC-32 per row (a uint32 vector)."""
import os
import zlib

import numpy as np

import _frontend_oracle as F
import _oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WHOLE_LIMIT = 6144  # bytes: larger outputs are stored as row CRCs


def fixture(op):
    return np.load(os.path.join(GOLDEN, f"reference_{op}.npz"))


def rows(a):
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)


def row_crcs(a):
    return np.array([zlib.crc32(r.tobytes()) for r in rows(a)], np.uint32)


def pack(a, whole_limit=WHOLE_LIMIT):
    a = np.ascontiguousarray(a)
    assert a.dtype != np.uint32
    return a if a.nbytes <= whole_limit else row_crcs(a)


def assert_pinned(got, stored, what=""):
    """got equals the recording bit for bit (floats compared as their words)."""
    got = np.ascontiguousarray(got)
    if stored.dtype == np.uint32:  # row CRCs
        crc = row_crcs(got)
        assert crc.shape == stored.shape, (what, "rows", crc.shape, stored.shape)
        bad = np.flatnonzero(crc != stored)
        assert bad.size == 0, (what, f"{bad.size} of {crc.size} rows differ, first", bad[:8].tolist())
        return
    assert got.dtype == stored.dtype and got.size == stored.size, (what, got.dtype, got.shape, stored.shape)
    g, s = got.reshape(-1).view(np.uint8), np.ascontiguousarray(stored).reshape(-1).view(np.uint8)
    if not np.array_equal(g, s):
        bad = np.flatnonzero(got.reshape(-1) != stored.reshape(-1))
        raise AssertionError((what, f"{bad.size} of {got.size} values differ, first at", bad[:8].tolist()))


# ---- inputs -------------------------------------------------------------------

def noise(w, h, cn, seed):
    return np.ascontiguousarray(F.pattern(w, h, cn, seed))


def with_channels(gray, cn, seed):
    """(H, W) -> (H, W, cn): channel 0 the image; channel c a darker copy of it
    with a little hashed noise, moved c pixels along x (so every channel carries
    its own texture and the same motion)."""
    if cn == 1:
        return np.ascontiguousarray(gray)
    h, w = gray.shape
    n = F.pattern(w, h, cn, seed).astype(np.int32)
    ch = [gray]
    for c in range(1, cn):
        v = np.clip(gray.astype(np.int32) * (c + 1) // (c + 2) + (n[:, :, c] & 15) - 8, 0, 255)
        ch.append(np.roll(v.astype(np.uint8), c, 1))
    return np.ascontiguousarray(np.stack(ch, 2))


def basketball():
    d = np.load(os.path.join(GOLDEN, "basketball_pair.npz"))
    return d["a"], d["b"]


LK_PAIRS = ("basketball", "synth")


def lk_pair(name, cn):
    """the two 160 x 120 frame pairs of the PyrLK cases"""
    if name == "basketball":
        a, b = (f[180:300, 240:400] for f in basketball())
    else:
        fr, _ = O.synth(4242, 160, 120, 6, 0, 2)
        a, b = fr[0], fr[1]
    seed = 900 + LK_PAIRS.index(name)
    return with_channels(a, cn, seed), with_channels(b, cn, seed)


LK_EDGE_POINTS = np.float32([[-5, 10], [170, 20], [0.5, 0.5], [159.5, 119.5], [-0.5, -0.5], [159.5, 0.5]])
OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS = 4, 8
LK_WINDOWS = [((21, 21), 3), ((15, 9), 2), ((7, 7), 2), ((31, 31), 1), ((63, 63), 0)]


def lk_pad(win):
    """the oracle pyramid's border must cover the window's reach outside the frame"""
    return max(32, max(win) + 1)


def lk_cases():
    """(pair, cn, win, max_level, flags, want_err)"""
    out = []
    for pair in LK_PAIRS:
        for cn in (1, 2, 3, 4):
            for win, lev in LK_WINDOWS:
                out.append((pair, cn, win, lev, 0, 1))
            sets = LK_WINDOWS[:2] if cn in (1, 3) else LK_WINDOWS[:1]
            for win, lev in sets:
                out.append((pair, cn, win, lev, OPTFLOW_USE_INITIAL_FLOW, 1))
                out.append((pair, cn, win, lev, OPTFLOW_LK_GET_MIN_EIGENVALS, 1))
                out.append((pair, cn, win, lev, 0, 0))
    return out


# (w, h, cn, win, max_level, seed)
PYR_CASES = [(29, 37, 1, (15, 15), 3, 11), (93, 61, 1, (7, 7), 4, 12)] + \
            [(160, 120, cn, (21, 21), 3, 20 + cn) for cn in (1, 2, 3, 4)] + \
            [(301, 77, cn, (15, 9), 2, 30 + cn) for cn in (1, 2, 3, 4)]

# corner maps: (w, h, seed) x (block, harris)
CMAP_SHAPES = [(3, 3, 41), (7, 1, 42), (1, 9, 43), (2, 2, 44), (61, 37, 45), (121, 130, 46)]
CMAP_MODES = [(2, 0), (3, 0), (5, 0), (3, 1)]
HARRIS_K = 0.04

# GFTT: the (maxCorners, quality, minDistance) rows of test_gftt_rois_match_oracle
GFTT_ROWS = [(256, 0.01, 3.0), (1000, 0.01, 0.0), (64, 0.05, 8.0), (32, 0.3, 1.0), (33, 0.02, 5.0), (300, 0.001, 2.5),
             (2000, 0.001, 6.5)]
GFTT_MODES = [(2, 0), (5, 0), (3, 1)]  # besides (3, 0): (block, harris), on the first two rows
# (frame, x, y, w, h)
GFTT_ROIS = [("synth", 40, 60, 24, 24), ("synth", 200, 150, 96, 64), ("synth", 317, 233, 57, 41),
             ("basketball", 250, 200, 64, 48), ("noise", 10, 60, 80, 60), ("noise", 60, 105, 40, 30)]


def gftt_frame(name):
    if name == "synth":
        fr, _ = O.synth(20261015, 640, 480, 32, 0, 1)
        return fr[0]
    if name == "basketball":
        return basketball()[0]
    img = noise(200, 160, 1, 77)
    img[100:140, 50:150] = 77  # a flat band; the last ROI lies wholly inside it
    return img


def gftt_cases():
    """(roi index, maxCorners, quality, minDistance, block, harris)"""
    out = []
    for r in range(len(GFTT_ROIS)):
        out += [(r, *row, 3, 0) for row in GFTT_ROWS]
        out += [(r, *row, b, hs) for b, hs in GFTT_MODES for row in GFTT_ROWS[:2]]
    return out


def gftt_roi(r):
    name, x, y, w, h = GFTT_ROIS[r]
    return np.ascontiguousarray(gftt_frame(name)[y:y + h, x:x + w])


# warpAffine: every interpolation x border x inverse flag; sizes cycle through these
WARP_SRC = [(97, 61), (8, 8), (64, 48), (31, 57)]
WARP_DST = [(120, 90), (33, 17), (64, 48), (1, 1), (97, 61), (7, 90), (50, 50)]
WARP_DEGENERATE = [np.zeros((2, 3)), np.array([[1e6, 0, 0], [0, 1e-7, 5e9]]), np.array([[0.0, 1, 0], [1, 0, 0]])]


def warp_inputs(i, sw, sh, dw, dh):
    return noise(sw, sh, 1, 500 + i), noise(dw, dh, 1, 700 + i)


# Farneback: (w, h, pyr_scale, poly_n, winsize, flags, use_initial_flow); levels 3, iterations 3.
# The box variant (flags 0) has a fixture of its own: its flows are stored whole, because
# the kernels are compared with them within a tolerance (tests/test_gpu_reference_pins.py).
FB_GAUSSIAN = 256
FB_LEVELS, FB_ITERS = 3, 3
FB_CASES = [(w, h, ps, pn, ws, FB_GAUSSIAN, 0) for w, h in ((64, 40), (130, 70))
            for ps, pn, ws in ((0.5, 5, 13), (0.3, 7, 13), (0.8, 5, 9))] + \
           [(64, 40, 0.5, 5, 13, FB_GAUSSIAN, 1)]
FB_BOX_CASES = [(w, h, ps, pn, ws, 0, 0) for w, h in ((64, 40), (130, 70))
                for ps, pn, ws in ((0.5, 5, 13), (0.3, 7, 13), (0.8, 5, 15))]


def fb_pair(w, h):
    fr, _ = O.synth(w * 7 + h, w, h, 3, 0, 2)
    return fr[0], fr[1]


def fb_sigma(poly_n):
    return 1.1 if poly_n <= 5 else 1.5


def fb_init(w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    n = (F.pattern(w, h, 2, 61).astype(np.float32) - np.float32(128)) / np.float32(256)
    return np.ascontiguousarray(np.stack([2.5 + 0.01 * xx, -1.25 - 0.005 * yy], 2).astype(np.float32) + n)


# HOG
# (w, h, cn, gamma correction, signed gradient, image seed).  cartToPolar runs its scalar forms on
# rows, and on the remainder of a row's 1024-element chunks, shorter than 16 pixels: widths 15 and 6,
# the 7 pixels after 1024 of 1031, the 2 after 2048 of 2050 (the shapes of
# test_gpu_hog.test_gradient_bit_exact).  The seeds of the narrow cases are the ones of 200..259 at
# which most of those pixels separate the fused scalar atan_f32 from the unfused one (at 2050 both).
HOG_GRAD_CASES = [(96, 160, 1, 1, 0, 197), (96, 160, 3, 1, 0, 199), (15, 17, 1, 1, 0, 116), (15, 17, 3, 1, 0, 118),
                  (15, 33, 1, 1, 0, 234), (15, 33, 3, 0, 1, 227), (6, 5, 1, 0, 1, 225), (6, 5, 3, 1, 0, 256),
                  (1031, 9, 1, 0, 1, 250), (1031, 9, 3, 1, 0, 245), (2050, 7, 3, 1, 0, 253), (2050, 7, 1, 0, 1, 257)]
HOG_DET_CASES = [((64, 128), 3, 0), ((64, 128), 3, 2), ((48, 96), 1, 0), ((48, 96), 1, 2)]  # (win, cn, group)


def hog_grad_image(i):
    w, h, cn, _, _, seed = HOG_GRAD_CASES[i]
    return hog_image(w, h, cn, seed)


def hog_image(w, h, cn, seed):
    fr, _ = O.synth(seed, w, h, 8, 0, 1)
    if cn == 1:
        return np.ascontiguousarray(fr[0])
    n = F.pattern(w, h, cn, seed).astype(np.int32)
    return np.ascontiguousarray(np.clip(fr[0].astype(np.int32)[:, :, None] + (n & 63) - 32, 0, 255).astype(np.uint8))
