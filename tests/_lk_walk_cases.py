"""Inputs and oracle references of tests/test_gpu_lk_walk_exits.py: one 160x120
frame pair and one point list built so that every pixel type's tracker leaves
the level walk (opencv_amd/csrc/lk_walk.hpp) by each of its ways out.
tests/test_lk_walk_exits_cases.py checks that on the CPU, from the oracle alone.

The frames are frames 0 and 3 of a synthetic sequence with a flat rectangle
and a still textured one painted into both.  Window 9x9 (8x8 for the
forward-backward call, which then runs the generic kernels), 3 levels, 2 Newton
steps per level: a point that never meets the eps test takes all 6 steps.  The points: far outside the frame
(lost at every level's bounds gate, no step taken), in the flat rectangle
(steps at the coarse levels, whose windows reach texture, then lost at level
0's minEig gate), within half a window of each edge, in a textured rectangle
that is the same in both frames (the eps test ends each level early), and a
grid of interior textured points."""
import numpy as np

import _fb_oracle as F
import _oracle as O

W, H = 160, 120
WIN, FB_WIN, MAX_LEVEL, MAX_COUNT, EPS, MIN_EIG, FB_THR = 9, 8, 2, 2, 0.01, 1e-4, 1.0
FULL = (MAX_LEVEL + 1) * MAX_COUNT
FLAGS = (0, O.OPTFLOW_LK_GET_MIN_EIGENVALS, O.OPTFLOW_USE_INITIAL_FLOW)
FLAT = (slice(36, 84), slice(56, 112))  # rows, columns
STILL = (slice(84, 120), slice(0, 60))  # a textured rectangle that does not move
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def gray_pair():
    def make():
        fr, _ = O.synth(20261022, W, H, 6, 0, 4)
        a, b = fr[0].copy(), fr[3].copy()
        a[FLAT] = 128
        b[FLAT] = 128
        still = np.kron(np.random.default_rng(3).integers(40, 220, (12, 20)), np.ones((3, 3), int)).astype(np.uint8)
        a[STILL] = still
        b[STILL] = still
        return np.ascontiguousarray(a), np.ascontiguousarray(b)

    return _once("gray", make)


def cn3_pair():
    """3 interleaved u8 channels: the gray frame and two rescaled, shifted copies"""
    def make():
        out = []
        for g in gray_pair():
            ch = [g] + [np.roll((g.astype(np.int32) * (c + 1) // (c + 2)).astype(np.uint8), c, 1) for c in (1, 2)]
            out.append(np.ascontiguousarray(np.stack(ch, 2)))
        return tuple(out)

    return _once("cn3", make)


def u16_cn3_pair():
    """the same as 16U: each value a fixed function of the u8 one (flat stays flat)"""
    def make():
        return tuple(np.ascontiguousarray(f.astype(np.uint16) * 257 + (f.astype(np.uint16) * 37) % 256)
                     for f in cn3_pair())

    return _once("u16cn3", make)


def points():
    def make():
        far = [(-50, -50), (400, 60), (80, 300), (-1000, 2000), (W + 4.5, H / 2), (W / 2, -5.25)]
        flat = [(84, 60), (70.5, 50.25), (100, 70), (60, 40), (108, 80), (90.75, 44.5)]
        edge = [(2, 60), (W - 2.5, 60), (80, 1.5), (80, H - 2), (1, 1), (W - 1.25, H - 1.75), (3.5, H - 3), (W - 4, 2.25)]
        still = [(20, 100), (30.5, 104.25), (40, 98), (14.75, 107.5)]
        ys, xs = np.mgrid[12:H - 8:19, 10:W - 8:23]
        grid = [(x + 0.25 * (i % 4), y + 0.5 * (i % 2)) for i, (x, y) in enumerate(zip(xs.ravel(), ys.ravel()))
                if not (FLAT[0].start - 6 <= y < FLAT[0].stop + 6 and FLAT[1].start - 6 <= x < FLAT[1].stop + 6)]
        return np.ascontiguousarray(np.array(far + flat + edge + still + grid, np.float32))

    return _once("pts", make)


def initial_flow():
    """the start of USE_INITIAL_FLOW: the points moved by up to 2 px"""
    return _once("init", lambda: points() + np.random.default_rng(9).uniform(-2, 2, points().shape).astype(np.float32))


def _init(flags):
    return initial_flow() if flags & O.OPTFLOW_USE_INITIAL_FLOW else None


def ref_gray(flags):
    """(next_pts, status, err, iters) of the one-channel u8 kernels"""
    def make():
        a, b = gray_pair()
        w = (WIN, WIN)
        return O.lk(O.Pyramid(a, w, MAX_LEVEL), O.Pyramid(b, w, MAX_LEVEL), points(), w, MAX_LEVEL, MAX_COUNT, EPS,
                    flags, MIN_EIG, O.ACCUM_EXACT, init=_init(flags))

    return _once(("gray", flags), make)


def ref_fb(flags):
    """_fb_oracle.Checked of the forward-backward call at window 8"""
    def make():
        a, b = gray_pair()
        w = (FB_WIN, FB_WIN)
        return F.checked_trace(O.Pyramid(a, w, MAX_LEVEL), O.Pyramid(b, w, MAX_LEVEL), points(), FB_WIN, MAX_LEVEL,
                               MAX_COUNT, EPS, MIN_EIG, FB_THR, O.ACCUM_EXACT, flags=flags, init=_init(flags))

    return _once(("fb", flags), make)


def ref_cn3(flags):
    def make():
        a, b = cn3_pair()
        w = (WIN, WIN)
        return O.lk(O.Pyramid(a, w, MAX_LEVEL), O.Pyramid(b, w, MAX_LEVEL), points(), w, MAX_LEVEL, MAX_COUNT, EPS,
                    flags, MIN_EIG, O.ACCUM_EXACT, init=_init(flags))

    return _once(("cn3", flags), make)


def ref_u16_cn3(flags):
    def make():
        a, b = u16_cn3_pair()
        w = (WIN, WIN)
        return O.lk16(O.Pyramid16(a, w, MAX_LEVEL, f32=True), O.Pyramid16(b, w, MAX_LEVEL, f32=True), points(), w,
                      MAX_LEVEL, MAX_COUNT, EPS, flags, MIN_EIG, init=_init(flags))

    return _once(("u16cn3", flags), make)


def exits(status, iters):
    """how many points left the walk by each way out"""
    status, iters = np.asarray(status), np.asarray(iters)
    return dict(lost_no_step=int(((status == 0) & (iters == 0)).sum()),
                lost_after_steps=int(((status == 0) & (iters > 0)).sum()),
                kept_every_step=int(((status == 1) & (iters == FULL)).sum()),
                kept_fewer_steps=int(((status == 1) & (iters < FULL)).sum()))
