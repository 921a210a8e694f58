"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle.

Bars:
  * synthetic frames, pyramid levels (interior + reflect-101 frame): bit-exact
  * LK vs oracle in ORC_ACCUM_EXACT mode (same integer sums, one rounding):
    bit-exact next_pts / status / err / iteration counts
  * LK vs oracle in the reference's SSE2 accumulation order: |dp| <= 1e-2 px for
    >= 99.5 % of tracked points and status agreement >= 99.5 %,
    plus the reference's own GPU-vs-CPU rule (test_optflow.cpp:241-264: int-truncated
    positions within 1 px, mismatch <= 1 %).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import _oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def klt():
    from opencv_amd import klt as K

    return K


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grid_points(h, w, step, margin):
    ys, xs = np.mgrid[margin:h - margin:step, margin:w - margin:step]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


def basketball_pair():
    d = np.load(os.path.join(GOLDEN, "basketball_pair.npz"))
    return d["a"], d["b"]


def test_synth_render_matches_oracle(gpu):
    K = klt()
    fr, gt = K.synth_render(20261015, 640, 480, 32, 0, 3, ctx=gpu)
    ofr, ogt = O.synth(20261015, 640, 480, 32, 0, 3)
    assert np.array_equal(fr.cpu().numpy(), ofr)
    assert np.array_equal(gt.numpy(), ogt)
    golden = json.load(open(os.path.join(GOLDEN, "synth_hashes.json")))
    fr2, gt2 = K.synth_render(20261015, 1920, 1080, 128, 0, 2, ctx=gpu)
    f2 = fr2.cpu().numpy()
    assert [hashlib.sha256(f2[i].tobytes()).hexdigest() for i in range(2)] == golden["1920x1080x128"]
    assert hashlib.sha256(gt2.numpy().tobytes()).hexdigest() == golden["1920x1080x128_gt"]


@pytest.mark.parametrize("shape,maxlev,win", [((480, 640), 3, 21), ((1080, 1920), 2, 21), ((375, 1242), 3, 21),
                                             ((61, 93), 4, 7), ((2160, 3840), 3, 21), ((37, 29), 3, 15)])
def test_pyramid_bit_exact(gpu, shape, maxlev, win):
    K = klt()
    img = np.random.default_rng(shape[0]).integers(0, 256, shape, dtype=np.uint8)
    P = K.build_pyramid(to_dev(img), (win, win), maxlev, ctx=gpu)
    torch.cuda.synchronize()
    R = O.Pyramid(img, (win, win), maxlev, pad=P.pyr.lv[0].pad)
    assert P.nlevels == R.nlevels
    for lvl in range(P.nlevels):
        assert np.array_equal(P.level(lvl, True), R.level(lvl, True)), f"level {lvl}"
        assert np.array_equal(P.deriv(lvl), O.scharr(R.level(lvl))), f"deriv level {lvl}"


@pytest.mark.parametrize("shape,maxlev,win", [((1080, 1920), 2, 21), ((1081, 1923), 2, 21), ((480, 640), 3, 21),
                                             ((375, 1242), 3, 21), ((2160, 3840), 4, 21), ((137, 261), 2, 21),
                                             ((61, 93), 4, 7), ((133, 70), 2, 21), ((66, 5000), 1, 21),
                                             ((37, 29), 3, 15), ((300, 301), 5, 7)])
def test_pyramid_levels_only_bit_exact(gpu, shape, maxlev, win):
    """tbdk_pyr_create_levels: the fused build (the padded level-0 copy and
    level 1, both straight from the frame with reflect-101 taps, in one launch;
    then one pyrDown launch per level), tiny levels whose padding reflects more
    than once included; every padded level bit-exact with the oracle's, padding
    included."""
    K = klt()
    img = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
    for _ in range(2):  # a rebuild rewrites every byte the first build wrote
        P = K.build_pyramid(to_dev(img), (win, win), maxlev, ctx=gpu, derivs=False)
        img = img[::-1].copy()
    torch.cuda.synchronize()
    assert not P.pyr.dv[0].data and P.pyr.flags == 1
    R = O.Pyramid(img[::-1].copy(), (win, win), maxlev, pad=P.pyr.lv[0].pad)
    assert P.nlevels == R.nlevels
    for lvl in range(P.nlevels):
        assert np.array_equal(P.level(lvl, True), R.level(lvl, True)), f"level {lvl}"


@pytest.mark.parametrize("shape", [(1081, 1920), (361, 640), (77, 124)])
def test_pyramid_frame_at_allocation_end(gpu, shape):
    """a frame whose last byte is the last byte of its allocation (odd height,
    width a multiple of 4, so the fused build's dword fast path reaches the last
    row): both builds bit-exact with the oracle (the fast path's aligned dwords
    end with the one holding the last in-image byte, klt_pyr.hip role B)"""
    K = klt()
    h, w = shape
    img = np.random.default_rng(w).integers(0, 256, shape, dtype=np.uint8)
    n = (h * w + 4095) // 4096 * 4096
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    frame = buf[n - h * w:].view(h, w)
    frame.copy_(to_dev(img))
    for derivs in (False, True):
        P = K.build_pyramid(frame, (21, 21), 2, ctx=gpu, derivs=derivs)
        torch.cuda.synchronize()
        R = O.Pyramid(img, (21, 21), 2, pad=P.pyr.lv[0].pad)
        for lvl in range(P.nlevels):
            assert np.array_equal(P.level(lvl, True), R.level(lvl, True)), f"level {lvl} derivs {derivs}"


@pytest.mark.parametrize("shape,maxlev,win", [((2160, 3840), 2, 21), ((2161, 3841), 3, 21), ((1079, 1919), 2, 21),
                                             ((517, 1023), 2, 31), ((255, 257), 2, 21), ((140, 140), 2, 21),
                                             ((1200, 300), 4, 7), ((375, 1242), 2, 45)])
def test_pyramid_fuse_modes_bit_exact(gpu, shape, maxlev, win):
    """ctx option pyr_fuse: 1 (two-role launch, 4 / 2 / 1 rows per thread: ctx
    option pyr_rows; pads of 32 / 48 / 64) and 0 (one launch per level): every
    padded level bit-exact with the oracle's, levels-only and with derivative
    planes"""
    K = klt()
    img = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    R = None
    try:
        for mode, rows, xcd in ((1, 4, 1), (1, 2, 0), (1, 1, 1), (1, 4, 0), (0, 4, 1)):
            gpu.set_option("pyr_fuse", mode)
            gpu.set_option("pyr_rows", rows)  # rows per thread of the two-role launch
            gpu.set_option("pyr_xcd", xcd)  # row bands per XCD
            for derivs in (False, True):
                P = K.build_pyramid(to_dev(img), (win, win), maxlev, ctx=gpu, derivs=derivs)
                torch.cuda.synchronize()
                if R is None:
                    R = O.Pyramid(img, (win, win), maxlev, pad=P.pyr.lv[0].pad)
                assert P.nlevels == R.nlevels
                for lvl in range(P.nlevels):
                    assert np.array_equal(P.level(lvl, True), R.level(lvl, True)), f"mode {mode}/{rows} level {lvl}"
                if derivs:
                    assert np.array_equal(P.deriv(0), O.scharr(R.level(0))), f"mode {mode}/{rows} deriv"
    finally:
        gpu.set_option("pyr_fuse", 1)
        gpu.set_option("pyr_rows", 1)
        gpu.set_option("pyr_xcd", 1)


@pytest.mark.parametrize("shape,maxlev,win", [((1080, 1920), 2, 21), ((2160, 3840), 2, 21), ((1081, 1923), 3, 21),
                                             ((137, 261), 2, 21), ((61, 93), 4, 7), ((375, 1242), 3, 15)])
def test_pyramid_borrowed_level0_bit_exact(gpu, shape, maxlev, win):
    """tbdk_pyr_build_borrowed: level 0 is the frame itself (pad 0, the frame's
    pitch), levels 1.. bit-exact with the oracle's padded levels; a following
    tbdk_pyr_build gives the pyramid its own padded level 0 again, and a
    borrowed build after that borrows again"""
    K = klt()
    rng = np.random.default_rng(sum(shape) + win)
    imgs = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(2)]
    frames = [to_dev(i) for i in imgs]
    P = K.Pyramid(gpu, shape[1], shape[0], maxlev, (win, win), derivs=False)
    own = P.pyr.lv[0].data
    for k, op in enumerate(("borrow", "build", "borrow")):
        img = imgs[k & 1]
        if op == "borrow":
            P.build_borrowed(frames[k & 1])
        else:
            P.build(frames[k & 1])
        torch.cuda.synchronize()
        L0 = P.pyr.lv[0]
        if op == "borrow":
            assert L0.data == frames[k & 1].data_ptr() and L0.pad == 0 and L0.pitch == shape[1]
        else:
            assert L0.data == own and L0.pad > 0
        R = O.Pyramid(img, (win, win), maxlev, pad=P.pyr.lv[1].pad)
        assert P.nlevels == R.nlevels
        assert np.array_equal(P.level(0), img)
        for lvl in range(1, P.nlevels):
            assert np.array_equal(P.level(lvl, True), R.level(lvl, True)), f"{op} level {lvl}"
        if op == "build":
            assert np.array_equal(P.level(0, True), R.level(0, True))


@pytest.mark.parametrize("win,maxlev", [(21, 2), (21, 3), (7, 3), (31, 2), (15, 4)])
def test_lk_borrowed_level0_equals_padded(gpu, win, maxlev):
    """PyrLK (the several-points-per-wave kernel) on pyramids whose level 0 is
    the frame itself (tbdk_pyr_build_borrowed: reflect-101 taps by coordinates
    where a window crosses the frame edge) equals PyrLK on the padded pyramids
    bit for bit, windows over the edges and points outside the frame included,
    with and without the minimum-eigenvalue error; other kernels refuse the
    borrowed level"""
    K = klt()
    fr, _ = K.synth_render(57 + win, 640, 480, 24, 0, 2, ctx=gpu)
    rng = np.random.default_rng(win + maxlev)
    pts = np.concatenate([rng.uniform([-12, -12], [652, 492], (3000, 2)),
                          np.array([[0, 0], [639, 479], [0.5, 240], [639.75, 10.25], [320, 0], [320, 479.5]])])
    pts = to_dev(pts.astype(np.float32))
    for flags8 in (False, True):
        lk = K.SparsePyrLKOpticalFlow((win, win), maxlev, 30, getMinEigenVals=flags8, impl=3)
        out = []
        for borrow in (False, True):
            Pa = K.Pyramid(gpu, 640, 480, maxlev, (win, win), derivs=False)
            Pb = K.Pyramid(gpu, 640, 480, maxlev, (win, win), derivs=False)
            if borrow:
                Pa.build_borrowed(fr[0])
                Pb.build_borrowed(fr[1])
            else:
                Pa.build(fr[0])
                Pb.build(fr[1])
            r = lk.calc(Pa, Pb, pts, want_iters=True)
            torch.cuda.synchronize()
            out.append([r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()])
        for a, b in zip(*out):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"flags8 {flags8}"
        assert out[0][1].mean() > 0.5
    lk1 = K.SparsePyrLKOpticalFlow((win, win), maxlev, 30, impl=1)
    with pytest.raises(Exception):
        lk1.calc(Pa, Pb, pts)


@pytest.mark.parametrize("win,maxlev", [(21, 2), (21, 3), (7, 3), (31, 2), (15, 4)])
def test_lk_levels_only_equals_derivative_planes(gpu, win, maxlev):
    """PyrLK on levels-only pyramids (the window's Scharr values derived in the
    kernel, BORDER_CONSTANT zeros outside the level) and with ctx option
    lk_scharr_fly on pyramids with planes: identical to the planes' results,
    including windows over the frame edges and points outside it."""
    K = klt()
    fr, gt = K.synth_render(31 + win, 640, 480, 24, 0, 2, ctx=gpu)
    rng = np.random.default_rng(win)
    pts = np.concatenate([rng.uniform([-12, -12], [652, 492], (3000, 2)),
                          np.array([[0, 0], [639, 479], [0.5, 240], [639.75, 10.25], [320, 0], [320, 479.5]])])
    pts = pts.astype(np.float32)
    lk = K.SparsePyrLKOpticalFlow((win, win), maxlev, 30)
    out = {}
    for mode in ("planes", "levels", "fly"):
        d = mode != "levels"
        Pa = K.build_pyramid(fr[0], (win, win), maxlev, ctx=gpu, derivs=d)
        Pb = K.build_pyramid(fr[1], (win, win), maxlev, ctx=gpu, derivs=d)
        gpu.set_option("lk_scharr_fly", 1 if mode == "fly" else 0)
        try:
            r = lk.calc(Pa, Pb, to_dev(pts), want_iters=True)
            torch.cuda.synchronize()
        finally:
            gpu.set_option("lk_scharr_fly", 0)
        out[mode] = [r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()]
    for mode in ("levels", "fly"):
        for a, b in zip(out["planes"], out[mode]):
            assert np.array_equal(a, b), mode
    assert out["planes"][1].mean() > 0.5


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (480, 640), (1079, 1919), (375, 1242)])
def test_pyr_down_plain_bit_exact(gpu, shape):
    K = klt()
    img = np.random.default_rng(3).integers(0, 256, shape, dtype=np.uint8)
    got = K.pyr_down(to_dev(img), ctx=gpu).cpu().numpy()
    assert np.array_equal(got, O.pyr_down(img))


def run_pair(gpu, a, b, pts, win=(21, 21), maxlev=3, iters=30, eps=0.01, flags=0, init=None, impl=0):
    K = klt()
    lk = K.SparsePyrLKOpticalFlow(win, maxlev, iters, bool(flags & 4), epsilon=eps,
                                  getMinEigenVals=bool(flags & 8), impl=impl)
    Pa = K.build_pyramid(to_dev(a), win, maxlev, ctx=gpu)
    Pb = K.build_pyramid(to_dev(b), win, maxlev, ctx=gpu)
    r = lk.calc(Pa, Pb, to_dev(pts), None if init is None else to_dev(init), want_iters=True)
    torch.cuda.synchronize()
    g = (r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy())
    pad = Pa.pyr.lv[0].pad
    Ra, Rb = O.Pyramid(a, win, maxlev, pad), O.Pyramid(b, win, maxlev, pad)
    n = len(pts)
    gx, gs = np.empty(n, np.float32), np.empty(n, np.float32)
    ex = O.lk(Ra, Rb, pts, win, maxlev, iters, eps, flags, accum=O.ACCUM_EXACT, init=init, gate=gx) + (gx,)
    sse = O.lk(Ra, Rb, pts, win, maxlev, iters, eps, flags, accum=O.ACCUM_SSE2, init=init, gate=gs) + (gs,)
    return g, ex, sse


def assert_exact(g, ex):
    nx, st, er, it = g
    assert np.array_equal(st, ex[1]), f"status mismatch {np.flatnonzero(st != ex[1])[:10]}"
    ok = st == 1
    assert np.array_equal(nx[ok].view(np.uint32), ex[0][ok].view(np.uint32)), \
        f"next_pts mismatch: max {np.abs(nx - ex[0])[ok].max()}"
    assert np.array_equal(er[ok].view(np.uint32), ex[2][ok].view(np.uint32))
    assert np.array_equal(it, ex[3])


def assert_tolerance(g, sse, frac=0.995, tol=1e-2, ex=None):
    """SURVEY.md §8(c) against the reference's SSE2 accumulation order; with
    `ex` (the exact-order oracle run carrying its gate margins, which the GPU
    equals bit for bit) also the clause that every status disagreement lies
    within 1e-3 (relative) of a minEig / determinant / bounds threshold in one
    of the two orders"""
    nx, st = g[0], g[1]
    assert (st == sse[1]).mean() >= frac
    if ex is not None:
        dis = np.flatnonzero(st != sse[1])
        m = np.minimum(ex[4][dis], sse[4][dis])
        assert (m <= 1e-3).all(), f"status disagreements away from every threshold: {list(zip(dis, m))[:5]}"
    ok = (st == 1) & (sse[1] == 1)
    d = np.abs(nx - sse[0]).max(1)[ok]
    assert (d <= tol).mean() >= frac, f"only {(d <= tol).mean():.4f} within {tol}"
    # reference GPU-vs-CPU rule (cudaoptflow/test/test_optflow.cpp:241-264)
    bad = (np.abs(np.trunc(nx) - np.trunc(sse[0])).max(1) > 1) | (st != sse[1])
    assert bad.mean() <= 0.01


IMPLS = [pytest.param(3, id="multi"), pytest.param(1, id="strip"), pytest.param(2, id="generic")]


@pytest.mark.parametrize("impl", IMPLS)
def test_lk_synthetic_640(gpu, impl):
    fr, _ = O.synth(20261015, 640, 480, 32, 0, 2)
    pts = grid_points(480, 640, 6, 2)
    g, ex, sse = run_pair(gpu, fr[0], fr[1], pts, impl=impl)
    assert_exact(g, ex)
    assert_tolerance(g, sse, ex=ex)


@pytest.mark.parametrize("impl", IMPLS)
def test_lk_basketball_pair(gpu, impl):
    a, b = basketball_pair()
    pts = grid_points(a.shape[0], a.shape[1], 5, 0)
    g, ex, sse = run_pair(gpu, a, b, pts, impl=impl)
    assert_exact(g, ex)
    assert_tolerance(g, sse, ex=ex)


@pytest.mark.parametrize("win,maxlev,iters", [((7, 7), 2, 7), ((9, 9), 3, 30), ((11, 11), 2, 30), ((15, 9), 4, 30),
                                              ((15, 15), 3, 30), ((19, 19), 3, 30), ((23, 23), 3, 30),
                                              ((29, 29), 3, 30), ((31, 31), 3, 30), ((41, 41), 4, 30),
                                              ((21, 21), 0, 1)])
def test_lk_window_and_level_variants(gpu, win, maxlev, iters):
    fr, _ = O.synth(77, 320, 240, 12, 3, 2)
    pts = grid_points(240, 320, 7, 0) + np.float32([0.37, 0.61])
    g, ex, sse = run_pair(gpu, fr[0], fr[1], pts, win, maxlev, iters)
    assert_exact(g, ex)
    if win[0] == win[1] and win[0] <= 31:  # every kernel must agree bit for bit
        for impl in (1, 2):
            g2, _, _ = run_pair(gpu, fr[0], fr[1], pts, win, maxlev, iters, impl=impl)
            assert_exact(g2, ex)


@pytest.mark.parametrize("impl", IMPLS)
def test_lk_edge_points_and_flags(gpu, impl):
    fr, _ = O.synth(9, 200, 150, 6, 0, 2)
    pts = np.array([[-100, -100], [1e4, 5], [0, 0], [199.9, 149.9], [-21.0, 50.0], [-20.5, 3.0], [210.0, 160.0],
                    [100.5, 75.5], [3.2, 147.9], [-10.0, -10.0], [219.0, 169.0], [-31.0, 80.0]], np.float32)
    g, ex, _ = run_pair(gpu, fr[0], fr[1], pts, impl=impl)
    assert_exact(g, ex)
    g, ex, _ = run_pair(gpu, fr[0], fr[1], pts, flags=8, impl=impl)  # OPTFLOW_LK_GET_MIN_EIGENVALS
    assert_exact(g, ex)
    init = pts + np.float32([1.5, -0.5])
    g, ex, _ = run_pair(gpu, fr[0], fr[1], pts, flags=4, init=init, impl=impl)  # OPTFLOW_USE_INITIAL_FLOW
    assert_exact(g, ex)


@pytest.mark.parametrize("impl", IMPLS)
def test_lk_high_contrast_exact_sums(gpu, impl):
    """binary 0/255 noise in 2x2 cells: per-column partial sums of diff * Ix reach
    ~1e8 > 2^26, so the multi-point kernel leaves its plain-scan fast path for the
    lo/hi-split exact sums; every kernel still equals the oracle bit for bit"""
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 2, (120, 160)) * 255).astype(np.uint8).repeat(2, 0).repeat(2, 1)
    b = np.roll(a, (1, -2), (0, 1))
    b[rng.random(b.shape) < 0.1] ^= 255
    pts = grid_points(240, 320, 9, 0) + np.float32([0.43, 0.27])
    for win, maxlev in (((21, 21), 2), ((31, 31), 1), ((9, 9), 0)):
        g, ex, _ = run_pair(gpu, a, b, pts, win, maxlev, 30, impl=impl)
        assert_exact(g, ex)
        assert (g[1] == 1).mean() > 0.2


def test_lk_empty_input(gpu):
    K = klt()
    lk = K.SparsePyrLKOpticalFlow()
    img = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    r = lk.calc(img, img, torch.zeros((0, 2), dtype=torch.float32, device="cuda"))
    assert r.next_pts.shape == (0, 2) and r.status.shape == (0,)


@pytest.mark.parametrize("impl", IMPLS)
def test_lk_1080p_full_size(gpu, impl):
    # config 2: 1080p pair, 64 boxes x 256 corners-like point count, 3-level PyrLK
    fr, gt = O.synth(20261015, 1920, 1080, 128, 0, 2)
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(0, 1920, 16384), rng.uniform(0, 1080, 16384)], 1).astype(np.float32)
    g, ex, sse = run_pair(gpu, fr[0], fr[1], pts, maxlev=2, impl=impl)
    assert_exact(g, ex)
    assert_tolerance(g, sse, ex=ex)


@pytest.mark.parametrize("solo", [1, 3])
def test_lk_one_point_steps_bit_exact(gpu, solo):
    """ctx option lk_solo: a wave whose other points have stopped runs its last
    point's remaining Newton steps from step `solo` on with the window's rows
    split over all its lanes; next_pts / status / err / iteration counts equal
    the exact-order oracle for windows 7..31 (1..9 points per wave), the
    lo/hi-split sums, the edge points and flags, levels-only (Scharr on the fly)
    and derivative-plane pyramids"""
    K = klt()
    gpu.set_option("lk_solo", solo)
    try:
        fr, _ = O.synth(20261015, 640, 480, 32, 0, 2)
        pts = grid_points(480, 640, 6, 2)
        g, ex, _ = run_pair(gpu, fr[0], fr[1], pts, impl=3)
        assert_exact(g, ex)
        fr, _ = O.synth(77, 320, 240, 12, 3, 2)
        pts = grid_points(240, 320, 7, 0) + np.float32([0.37, 0.61])
        for win, maxlev in (((7, 7), 2), ((13, 13), 3), ((21, 21), 3), ((31, 31), 2)):
            g, ex, _ = run_pair(gpu, fr[0], fr[1], pts, win, maxlev, 30, impl=3)
            assert_exact(g, ex)
        fr, _ = O.synth(9, 200, 150, 6, 0, 2)
        pts = np.array([[-100, -100], [1e4, 5], [0, 0], [199.9, 149.9], [-21.0, 50.0], [-20.5, 3.0], [210.0, 160.0],
                        [100.5, 75.5], [3.2, 147.9], [-10.0, -10.0], [219.0, 169.0], [-31.0, 80.0]], np.float32)
        for flags, init in ((0, None), (8, None), (4, pts + np.float32([1.5, -0.5]))):
            g, ex, _ = run_pair(gpu, fr[0], fr[1], pts, flags=flags, init=init, impl=3)
            assert_exact(g, ex)
        rng = np.random.default_rng(5)
        a = (rng.integers(0, 2, (120, 160)) * 255).astype(np.uint8).repeat(2, 0).repeat(2, 1)
        b = np.roll(a, (1, -2), (0, 1))
        b[rng.random(b.shape) < 0.1] ^= 255
        pts = grid_points(240, 320, 9, 0) + np.float32([0.43, 0.27])
        for win, maxlev in (((21, 21), 2), ((31, 31), 1)):
            g, ex, _ = run_pair(gpu, a, b, pts, win, maxlev, 30, impl=3)
            assert_exact(g, ex)
        # levels-only pyramids (the TBD loop's instance) against the planes instance
        fr, _ = K.synth_render(52, 640, 480, 24, 0, 2, ctx=gpu)
        pts = np.random.default_rng(21).uniform([-12, -12], [652, 492], (3000, 2)).astype(np.float32)
        lk = K.SparsePyrLKOpticalFlow((21, 21), 2, 30)
        out = []
        for d in (True, False):
            Pa = K.build_pyramid(fr[0], (21, 21), 2, ctx=gpu, derivs=d)
            Pb = K.build_pyramid(fr[1], (21, 21), 2, ctx=gpu, derivs=d)
            r = lk.calc(Pa, Pb, to_dev(pts), want_iters=True)
            torch.cuda.synchronize()
            out.append([r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()])
        gpu.set_option("lk_solo", 0)
        Pa = K.build_pyramid(fr[0], (21, 21), 2, ctx=gpu, derivs=False)
        Pb = K.build_pyramid(fr[1], (21, 21), 2, ctx=gpu, derivs=False)
        r = lk.calc(Pa, Pb, to_dev(pts), want_iters=True)
        torch.cuda.synchronize()
        base = [r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()]
        for o in out:
            for u, v in zip(o, base):
                assert np.array_equal(u, v)
    finally:
        gpu.set_option("lk_solo", 4)


def _sample_hash(i):
    """splitmix64(i): the library times launch i iff this % timing_every == 0"""
    M = (1 << 64) - 1
    x = (i + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def test_timing_sampling(gpu):
    """ctx option timing_every: events on a pseudo-random 1/N of the selected
    launches (splitmix64 of the launch index); tbdk_timing_calls
    counts all of them (bench.py's roofline uses both)"""
    K = klt()
    fr, _ = O.synth(3, 320, 240, 8, 0, 2)
    pts = to_dev(grid_points(240, 320, 16, 8))
    P0 = K.build_pyramid(to_dev(fr[0]), (21, 21), 2, ctx=gpu)
    P1 = K.build_pyramid(to_dev(fr[1]), (21, 21), 2, ctx=gpu)
    lk = K.SparsePyrLKOpticalFlow((21, 21), 2)
    try:
        gpu.timing_select(["lk_sparse"])
        gpu.set_option("timing_every", 3)
        gpu.timing_enable(True)
        for _ in range(7):
            lk.calc(P0, P1, pts)
        torch.cuda.synchronize()
        c, ms = gpu.timing_query("lk_sparse")
        assert gpu.timing_calls("lk_sparse") == 7
        assert c == sum(_sample_hash(i) % 3 == 0 for i in range(7)) and ms > 0
    finally:
        gpu.timing_enable(False)
        gpu.timing_select(None)
        gpu.set_option("timing_every", 1)
    with pytest.raises(Exception):
        gpu.set_option("timing_every", 0)
