"""The Scharr-on-the-fly PyrLK setup's integer-origin arm (lk_int_origin.hpp:
waves whose stepping points all have a zero-fraction window origin at the level,
as every goodFeaturesToTrack corner has at level 0) against the exact-order
oracle, bit for bit on nextPts, status, err and iters.  The arm is chosen per
wave and per level, so the cases order their point lists by waves of
64 // win points.  Built like tests/test_gpu_lk_trims.py: impl 3, pyramids
without derivative planes.  With the trace build of the library present
(opencv_amd/lib/libtbdk_trace.so, -DTBDK_LK_TRACE) the last test also reads
which waves took the arm."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fb_oracle as F
import _loop_pair as LP
import _oracle as O
from test_gpu_lk_trims import assert_exact, crosses, textured_pair, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk_trace.so")
BIG, SMALL = (384, 320), (160, 128)  # level 2: 96 x 80 (window 21 has interior windows there) / 40 x 32
FRAC = np.float32([0.37, 0.61])


def klt():
    from opencv_amd import klt as K

    return K


_PAIRS = {}


def pair(size, kind="texture"):
    """the frame pairs, made once: a textured pair, a 0/255 checkerboard (2 px
    cells) and its shifted copy with 5 % of the pixels flipped, 0/255 vertical
    stripes (3 px) shifted by one column, a flat pair"""
    key = (size, kind)
    if key not in _PAIRS:
        w, h = size
        yy, xx = np.mgrid[0:h, 0:w]
        if kind == "texture":
            _PAIRS[key] = textured_pair(w, h, 7)
        elif kind == "checker":
            a = (((yy // 2 + xx // 2) & 1) * 255).astype(np.uint8)
            b = np.roll(a, (1, 0), (0, 1))
            b[np.random.default_rng(11).random(b.shape) < 0.05] ^= 255
            _PAIRS[key] = (a, b)
        elif kind == "stripes":
            a = (((xx // 3) & 1) * 255).astype(np.uint8)
            _PAIRS[key] = (a, np.roll(a, 1, 1))
        else:
            _PAIRS[key] = (np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8))
    return _PAIRS[key]


def interior_grid(size, win, maxlev, step=(9, 13)):
    """integer points whose window is inside the level at every level (where the
    coarsest level has room for one; else inside level 0), odd and even
    coordinates alike: with an odd step the coordinates cover every residue
    modulo 2^maxlev, so the coarse levels see every fraction class"""
    w, h = size
    half = (win - 1) // 2
    m = (half + 1) << maxlev
    if w - 2 * m < 16 or h - 2 * m < 16:
        m = half + 2
    ys, xs = np.mgrid[m:h - m - 1:step[1], m:w - m - 1:step[0]]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    assert not crosses(pts, win, 0, w, h).any() and (pts == np.floor(pts)).all()
    return pts


def takes_arm(pts, win, w, h, level=0):
    """the kernel's rule per wave of 64 // win points at `level`: no stepping
    point's window leaves the level and every stepping point's window origin
    has a zero fraction (a point wholly outside the level does not step)"""
    P = 64 // win
    half = np.float32((win - 1) * 0.5)
    sc = np.float32(1.0 / (1 << level))
    lw, lh = w, h
    for _ in range(level):
        lw, lh = (lw + 1) // 2, (lh + 1) // 2
    o = pts * sc - half
    io = np.floor(o)
    steps = ~((io[:, 0] < -win) | (io[:, 0] >= lw) | (io[:, 1] < -win) | (io[:, 1] >= lh))
    bad = steps & (crosses(pts, win, level, w, h) | (o != io).any(1))
    n = len(pts)
    pad = (-n) % P
    bad = np.concatenate([bad, np.zeros(pad, bool)]).reshape(-1, P)
    steps = np.concatenate([steps, np.zeros(pad, bool)]).reshape(-1, P)
    return ~bad.any(1) & steps.any(1)


def run(gpu, a, b, pts, win, maxlev, borrow=False, init=None, iters=30):
    K = klt()
    h, w = a.shape
    lk = K.SparsePyrLKOpticalFlow((win, win), maxlev, iters, useInitialFlow=init is not None, impl=3)
    Pa = K.Pyramid(gpu, w, h, maxlev, (win, win), derivs=False)
    Pb = K.Pyramid(gpu, w, h, maxlev, (win, win), derivs=False)
    fa, fb = to_dev(a), to_dev(b)
    if borrow:
        Pa.build_borrowed(fa)
        Pb.build_borrowed(fb)
    else:
        Pa.build(fa)
        Pb.build(fb)
    r = lk.calc(Pa, Pb, to_dev(pts), to_dev(init) if init is not None else None, want_iters=True)
    torch.cuda.synchronize()
    return r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()


_ORACLE = {}


def oracle(key, a, b, pts, win, maxlev, init=None):
    """the exact-order oracle's result, computed once per case"""
    if key not in _ORACLE:
        Ra, Rb = O.Pyramid(a, (win, win), maxlev), O.Pyramid(b, (win, win), maxlev)
        _ORACLE[key] = O.lk(Ra, Rb, pts, (win, win), maxlev, 30, 0.01, O.OPTFLOW_USE_INITIAL_FLOW if init is not None
                            else 0, accum=O.ACCUM_EXACT, init=init)
    return _ORACLE[key]


# ---- the point lists (also built by the trace worker) -------------------------

def case_interior():
    """case 1: 594 interior integer points, window 21, 3 levels"""
    return pair(BIG) + (interior_grid(BIG, 21, 2), 21, 2)


def case_patterns():
    """case 2: waves of three points in all eight integer / fractional patterns
    (bit s of the pattern: point s of the wave is moved by a fraction; the
    fraction is in x only, in y only or in both, in turn), 13 times over"""
    g = interior_grid(BIG, 21, 2)
    pts = []
    for rep in range(13):
        for pat in range(8):
            for s in range(3):
                p = g[(rep * 24 + pat * 3 + s) * 7 % len(g)].copy()
                if pat >> s & 1:
                    p += FRAC * np.float32([(rep + s) % 3 != 1, (rep + s) % 3 != 0])
                pts.append(p)
    return pair(BIG) + (np.array(pts, np.float32), 21, 2)


def case_edges():
    """case 3: integer points whose level-0 window crosses each edge and each
    corner, and points wholly outside the frame (status 0), each in the middle
    or at an end of a wave of interior integer points"""
    w, h = BIG
    g = interior_grid(BIG, 21, 2)
    edge = [(3, 160), (380, 161), (190, 4), (191, 316), (2, 3), (381, 3), (2, 317), (381, 316), (9, 100), (100, 309)]
    outside = [(-40, 100), (420, 100), (100, -40), (101, 360), (-30, -30), (5000, 5000)]
    pts = []
    for j, sp in enumerate(edge + outside):
        wave = [g[(3 * j + t) * 11 % len(g)] for t in range(3)]
        wave[j % 3] = np.float32(sp)
        pts += wave
    pts = np.array(pts, np.float32)
    kind = np.array([1] * len(edge) + [2] * len(outside))  # per wave: an edge point / an outside point
    assert crosses(pts, 21, 0, w, h).reshape(-1, 3).sum(1).tolist() == [1] * len(kind)
    return pair(BIG) + (pts, 21, 2), kind


# ---- the cases -----------------------------------------------------------------

@pytest.mark.parametrize("borrow", [False, True], ids=["padded", "borrowed"])
def test_interior_integer_points(gpu, borrow):
    a, b, pts, win, ml = case_interior()
    assert 550 <= len(pts) <= 650 and {0, 1} == set((pts[:, 0] % 2).tolist()) == set((pts[:, 1] % 2).tolist())
    assert len({(x % 4, y % 4) for x, y in pts.tolist()}) == 16
    assert takes_arm(pts, win, *BIG).all()
    g = run(gpu, a, b, pts, win, ml, borrow=borrow)
    assert_exact(g, oracle("interior", a, b, pts, win, ml))
    assert (g[1] == 1).mean() > 0.9


def test_integer_and_fractional_points_mixed_in_a_wave(gpu):
    a, b, pts, win, ml = case_patterns()
    arm = takes_arm(pts, win, *BIG)
    arm = arm.reshape(13, 8)
    assert arm[:, 0].all() and not arm[:, 1:].any()
    assert_exact(run(gpu, a, b, pts, win, ml), oracle("patterns", a, b, pts, win, ml))


@pytest.mark.parametrize("borrow", [False, True], ids=["padded", "borrowed"])
def test_edge_and_outside_points_among_interior_ones(gpu, borrow):
    (a, b, pts, win, ml), kind = case_edges()
    ex = oracle("edges", a, b, pts, win, ml)
    g = run(gpu, a, b, pts, win, ml, borrow=borrow)
    assert_exact(g, ex)
    special = np.arange(len(kind)) * 3 + np.arange(len(kind)) % 3
    assert not g[1][special[kind == 2]].any() and (g[1] == 1).mean() > 0.7  # the outside points are lost


@pytest.mark.parametrize("n", [100, 64, 1])
def test_point_count_not_a_multiple_of_the_wave(gpu, n):
    """case 4: 100 = 33 x 3 + 1 and 64 = 21 x 3 + 1 points leave one point in the
    last wave, whose other lanes are idle and must not enter the test"""
    a, b, pts, win, ml = case_interior()
    pts = np.ascontiguousarray(pts[::5][:n])
    assert len(pts) == n and n % 3 == 1
    assert_exact(run(gpu, a, b, pts, win, ml), oracle(("count", n), a, b, pts, win, ml))


def test_segmented_launch_with_one_point_in_a_last_wave(gpu):
    """case 4, segmented: the TBD loop's launches over point sets of stride 64
    (21 waves of three candidates and one of a single candidate per set), a
    refreshed set tracked straight from its integer GFTT corners; every frame
    against the oracle pipeline"""
    c = LP._case("int_origin_seg", {"win": 21, "max_level": 2, "max_corners": 64}, N=6, F=6, drop=0.0)
    stats = LP.run_pair(gpu, c.W, c.H, c.N, c.F, c.seed, c.drop, c.cfg, c.options)
    assert stats["refreshed"] > 0 and stats["lk_points"] > 100 and stats["preds"] > 0


@pytest.mark.parametrize("win", [7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31])
def test_every_on_the_fly_instance(gpu, win):
    """case 5: about 60 integer points per window, 160 x 128 for windows up to 13"""
    size = SMALL if win <= 13 else BIG
    a, b = pair(size)
    g = interior_grid(size, win, 2, (7, 5))
    pts = np.ascontiguousarray(g[:: max(1, len(g) // 60)][:61])
    assert 50 <= len(pts) <= 61 and takes_arm(pts, win, *size).all()
    r = run(gpu, a, b, pts, win, 2)
    assert_exact(r, oracle(("win", win), a, b, pts, win, 2))
    assert (r[1] == 1).mean() > 0.5


def test_initial_flow_with_fractional_start(gpu):
    """case 6: prev is integer (the arm is taken at level 0), next starts at a
    fractional position"""
    a, b, pts, win, ml = case_interior()
    pts = np.ascontiguousarray(pts[::3])
    rng = np.random.default_rng(5)
    init = (pts + np.float32([1.3, -0.8]) + rng.uniform(-0.5, 0.5, pts.shape)).astype(np.float32)
    assert (init != np.floor(init)).all()
    assert_exact(run(gpu, a, b, pts, win, ml, init=init), oracle("init", a, b, pts, win, ml, init=init))


@pytest.mark.parametrize("ml", [0, 3])
def test_one_level_and_four_levels(gpu, ml):
    """case 7: maxLevel 0 (level 0 is the first level) and 3"""
    a, b, pts, win, _ = case_interior()
    pts = np.ascontiguousarray(pts[::3])
    assert_exact(run(gpu, a, b, pts, win, ml), oracle(("levels", ml), a, b, pts, win, ml))


@pytest.mark.parametrize("kind", ["checker", "stripes", "flat"])
@pytest.mark.parametrize("win", [21, 7])
def test_extreme_frames(gpu, kind, win):
    """case 8: a 0/255 checkerboard (the +-4080 derivatives, G partials on the
    lo/hi-split sums), 0/255 vertical stripes and a flat pair (the minimum
    eigenvalue rejection)"""
    a, b = pair(SMALL, kind)
    pts = interior_grid(SMALL, win, 0, (5, 7))
    r = run(gpu, a, b, pts, win, 2)
    ex = oracle((kind, win), a, b, pts, win, 2)
    assert_exact(r, ex)
    if kind != "checker":
        assert not r[1].any()


@pytest.mark.parametrize("solo", [0, 4])
def test_one_point_steps_after_the_arm(gpu, solo):
    """case 9: lk_solo 0 and 4"""
    a, b, pts, win, ml = case_interior()
    pts = np.ascontiguousarray(pts[1::3])
    gpu.set_option("lk_solo", solo)
    try:
        assert_exact(run(gpu, a, b, pts, win, ml), oracle("solo", a, b, pts, win, ml))
    finally:
        gpu.set_option("lk_solo", 4)


def test_forward_backward_check_on_integer_points(gpu):
    """case 10: tbdk_lk_sparse_fb; the forward pass takes the arm, the backward
    pass starts from its results and does not"""
    K = klt()
    a, b, pts, win, ml = case_interior()
    pts = np.ascontiguousarray(pts[::2])
    h, w = a.shape
    Ra, Rb = O.Pyramid(a, (win, win), ml), O.Pyramid(b, (win, win), ml)
    ref = F.checked_trace(Ra, Rb, pts, win, ml, 30, 0.01, 1e-4, 0.25, O.ACCUM_EXACT)
    lk = K.SparsePyrLKOpticalFlow((win, win), ml, 30, impl=3)
    Pa = K.Pyramid(gpu, w, h, ml, (win, win), derivs=False).build(to_dev(a))
    Pb = K.Pyramid(gpu, w, h, ml, (win, win), derivs=False).build(to_dev(b))
    r = lk.calc_checked(Pa, Pb, to_dev(pts), back_threshold=0.25, want_iters=True)
    torch.cuda.synchronize()
    bits = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32)
    st, nx = r.status.cpu().numpy(), r.next_pts.cpu().numpy()
    assert np.array_equal(st, ref.status) and 0 < st.sum()
    ok = ref.fwd_status == 1
    assert np.array_equal(bits(nx[ok]), bits(ref.next_pts[ok]))
    assert np.array_equal(bits(r.err.cpu().numpy()[ok]), bits(ref.err[ok]))
    assert np.array_equal(r.iters.cpu().numpy(), ref.iters)
    sel = ok & (ref.back_status == 1)
    assert np.array_equal(bits(r.back_pts.cpu().numpy()[sel]), bits(ref.back_pts[sel]))
    assert np.array_equal(bits(r.fb_err.cpu().numpy()), bits(ref.fb_err))


def test_trace_build_reports_the_arm(gpu):
    """case 11: the trace build's per-wave record (bits 56.. of word 5: the
    levels whose setup took the arm) for cases 1 to 3, read by a child process
    that loads the trace library.  Level 0: every wave of case 1; only the
    all-integer pattern of case 2; in case 3 no wave that holds an edge point,
    and every wave whose third point is wholly outside the frame (it does not
    step, so it is not asked)."""
    if not os.path.exists(TRACE_LIB):
        pytest.skip("the trace build (make EXTRA=-DTBDK_LK_TRACE OUT=../lib/libtbdk_trace.so "
                    "BUILD=../../build/tbdk_trace) is not present: the arm's bits are not read")
    env = dict(os.environ, TBDK_LIB=TRACE_LIB)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lk_int_trace_worker.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    w, h = BIG
    for name, case in (("interior", case_interior()), ("patterns", case_patterns()), ("edges", case_edges()[0])):
        pts, win, ml = case[2:]
        bits = np.array(got[name])
        assert len(bits) == (len(pts) + 2) // 3
        for lv in range(ml + 1):
            assert np.array_equal((bits >> lv & 1).astype(bool), takes_arm(pts, win, w, h, lv)), (name, lv)
    assert all(v & 1 for v in got["interior"])
    pat = np.array(got["patterns"]).reshape(13, 8) & 1
    assert pat[:, 0].all() and not pat[:, 1:].any()
    kind = case_edges()[1]
    assert not (np.array(got["edges"])[kind == 1] & 1).any() and (np.array(got["edges"])[kind == 2] & 1).all()
