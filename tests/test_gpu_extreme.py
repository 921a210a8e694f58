"""Every pixel kernel on saturated, flat and periodic frames (tests/_extreme_cases.py)
against its CPU oracle in exact-order mode, bit for bit: frames that are all 0 or
all 255, 0/255 edges that drive Scharr to +-4080 on every pixel of a window,
periodic pictures whose corner responses tie by the thousand, cubic interpolation
across 0/255 steps, windows whose G matrix is exactly singular, and the float
pixel paths at and beyond the end of their finite range.
tests/test_extreme_cases.py proves on the CPU that the pictures do all that.

Every float output is compared as bit patterns, no point or pixel is left out,
and a failure names the pattern, the pair, the kernel and the first differing
index.  Sparse results follow the suite's rule (assert_exact): status and
iteration counts at every point, positions and errors where status is 1 (a lost
point's position is a leftover of the level that lost it).

What a wrong kernel would trip over here and not on synthetic scenes or noise
(by reasoning, one example per family):
  pyramids / Scharr   a plane clamped to +-4079, or narrowed below 13 bits: vstripe2, every pixel +-4080
  sparse PyrLK u8     a 32-bit whole-window sum, or err added in another order than the reference's
                      float chain once it passes 2^24: binary / binblk inverted, window 63 (found, fixed)
  forward-backward    a wave none of whose points survives the forward pass: zero (all 454 lost)
  multi-channel       a 32-bit whole-window sum in klt_cn: binary, window 63 (its err chain: found, fixed)
  dense PyrLK         case images that clamp an interpolated derivative: check2, +-4080 at integer positions
  GFTT                a tie order that depends on the chunking of the wide path: check2, 18,096 equal keys,
                      also under ROIs cut at odd offsets; an int32 product on 16U maps: any 0 | 65535 edge
  cornerSubPix        the singular-matrix guard: zero, full, check1 (every gradient 0)
  warpAffine, remap   cubic without saturation at either end: binblk, blocks (0, 255 and between in one output)
  front end           a rounding term or a coefficient sum that is not exactly 1: full must stay 255
  Farneback           a fast reciprocal or flushed denormals in the 2x2 solve: vstripe2, flows of 1e-9 by bits
  HOG                 block normalisation without its epsilon: zero, full (0 / 0)
  float pixel paths   a NaN window position converted to 0 and tracked on: 0 | 4095 (found, fixed)"""
import numpy as np
import pytest
import torch

import _extreme_cases as X
import _fb_oracle as FBO
import _frontend_oracle as FE
import _gftt_f32_oracle as O32
import _oracle as O
import _remap_cases as PC
import _remap_oracle as R
import _subpix_oracle as SO
from test_gpu_f32 import _cn_pyr
from test_gpu_farneback import _gpu_flow
from test_gpu_gftt import check as gftt_check, detect as gftt_detect
from test_gpu_hog import _prm as hog_prm
from test_gpu_klt import IMPLS, assert_exact, run_pair
from test_gpu_klt_cn import run_pair_cn
from test_gpu_lk_fb import back_equal, host as fb_host

pytestmark = pytest.mark.gpu

W, H = X.LK_SIZE
PAT = X.patterns(W, H)
PTS = X.points(W, H)
ALL = list(X.NAMES)


def K():
    from opencv_amd import klt

    return klt


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:  # torch has no uint16 arithmetic; the kernels only take the pointer
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(got, want, what, nan_any=False):
    """bit patterns equal everywhere; the message carries the first differing
    index.  nan_any: a NaN equals a NaN whatever its sign and payload (what an
    invalid operation returns there is the processor's choice: x86 gives the
    negative quiet NaN, gfx950 the positive one)"""
    got, want = host(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    ne = np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)
    if nan_any:
        ne &= ~(np.isnan(got) & np.isnan(want))
    if ne.any():
        i = tuple(int(v) for v in np.argwhere(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} values differ, first at index {i}: "
                             f"got {got[i]!r}, want {want[i]!r}")


def lk_same(what, g, ex):
    """g, ex: (next_pts, status, err, iters)"""
    same_bits(g[1], ex[1], f"{what}: status")
    same_bits(g[3], ex[3], f"{what}: iters")
    ok = ex[1] == 1
    same_bits(g[0][ok], ex[0][ok], f"{what}: next_pts of the tracked points")
    same_bits(g[2][ok], ex[2][ok], f"{what}: err of the tracked points")
    assert np.isfinite(g[0][ok]).all() and np.isfinite(g[2][ok]).all(), f"{what}: non-finite result at status 1"
    assert_exact(g, ex)


# ---- pyramids and Scharr planes -------------------------------------------------------------------

def _reflect_frame(level, pad):
    hh, ww = level.shape[:2]
    ry = [O.load().orc_reflect101(y - pad, hh) for y in range(hh + 2 * pad)]
    rx = [O.load().orc_reflect101(x - pad, ww) for x in range(ww + 2 * pad)]
    return level[np.ix_(ry, rx)]


def _fp_pyramid_same(what, P, Rf):
    assert P.nlevels == Rf.nlevels, what
    for i in range(P.nlevels):
        same_bits(P.level(i), Rf.levels[i], f"{what} level {i}")
        same_bits(P.level(i, True), _reflect_frame(Rf.levels[i], P.pyr.lv[i].pad), f"{what} level {i} with border")
        same_bits(P.deriv(i), Rf.derivs[i], f"{what} derivative plane {i}")


@pytest.mark.parametrize("size", [X.SMALL_SIZE, X.LK_SIZE], ids=["97x61", "160x120"])
@pytest.mark.parametrize("name", ALL)
def test_pyramids_and_scharr_planes(gpu, name, size):
    k = K()
    w, h = size
    img = X.patterns(w, h)[name]
    win, ml = (9, 9), 3
    R = None
    try:
        for fuse in (1, 0):
            gpu.set_option("pyr_fuse", fuse)
            P = k.build_pyramid(dev(img), win, ml, ctx=gpu)
            torch.cuda.synchronize()
            R = R or O.Pyramid(img, win, ml, pad=P.pyr.lv[0].pad)
            assert P.nlevels == R.nlevels, (name, size)
            for i in range(P.nlevels):
                same_bits(P.level(i, True), R.level(i, True), f"{name} {w}x{h} pyr_fuse {fuse} level {i} with border")
                same_bits(P.deriv(i), O.scharr(R.level(i)), f"{name} {w}x{h} pyr_fuse {fuse} Scharr plane {i}")
    finally:
        gpu.set_option("pyr_fuse", 1)
    frame = dev(img)
    B = k.Pyramid(gpu, w, h, ml, win, derivs=False).build_borrowed(frame)
    torch.cuda.synchronize()
    Rb = O.Pyramid(img, win, ml, pad=B.pyr.lv[1].pad)
    same_bits(B.level(0), img, f"{name} {w}x{h} borrowed level 0")
    for i in range(1, B.nlevels):
        same_bits(B.level(i, True), Rb.level(i, True), f"{name} {w}x{h} borrowed build level {i} with border")
    img3 = X.to_cn(img, 3)
    P3 = k.build_pyramid(dev(img3), win, ml, ctx=gpu)
    torch.cuda.synchronize()
    R3 = O.Pyramid(img3, win, ml, pad=P3.pyr.lv[0].pad)
    assert P3.nlevels == R3.nlevels and P3.channels == 3
    for i in range(P3.nlevels):
        same_bits(P3.level(i, True), R3.level(i, True), f"{name} {w}x{h} cn 3 level {i} with border")
        same_bits(P3.deriv(i), O.scharr(R3.level(i)), f"{name} {w}x{h} cn 3 Scharr plane {i}")
    for dt, f32 in ((torch.float16, False), (torch.float32, True)):
        Pf = k.Pyramid(gpu, w, h, ml, win, dt).build(dev(img))
        torch.cuda.synchronize()
        _fp_pyramid_same(f"{name} {w}x{h} {'fp32' if f32 else 'fp16'} from u8", Pf, O.Pyramid16(img, win, ml, f32=f32))


# ---- sparse PyrLK, 8-bit -----------------------------------------------------------------------------

# (window, max_level): the levels exist at 160x120; 5, 41 and 63 are the generic kernel's alone
LK_WINDOWS = {3: [(9, 3), (21, 2)], 1: [(9, 3), (21, 2)], 2: [(5, 2), (9, 3), (21, 2), (41, 1), (63, 0)]}
IMPL_NAME = {0: "auto", 1: "strip", 2: "generic", 3: "multi"}


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", ALL)
def test_lk_sparse_u8(gpu, name, impl):
    a = PAT[name]
    tracked = 0
    for kind in X.PAIRS:
        b = X.pair(a, kind)
        for win, ml in LK_WINDOWS[impl]:
            g, ex, _ = run_pair(gpu, a, b, PTS, (win, win), ml, impl=impl)
            lk_same(f"{name}/{kind} {IMPL_NAME[impl]} win {win} levels {ml}", g, ex)
            tracked += int(g[1].sum())
    assert (tracked == 0) == (name in X.FEATURELESS), f"{name}: {tracked} points tracked over all pairs and windows"


@pytest.mark.parametrize("impl", [0, 2], ids=["auto", "generic"])
def test_lk_sparse_u8_non_square_window(gpu, impl):
    a = PAT["binblk"]
    for kind in X.PAIRS:
        g, ex, _ = run_pair(gpu, a, X.pair(a, kind), PTS, (15, 9), 2, impl=impl)
        lk_same(f"binblk/{kind} {IMPL_NAME[impl]} win 15x9", g, ex)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", ["binblk", "check2"])
def test_lk_sparse_u8_flags(gpu, name, impl):
    """OPTFLOW_LK_GET_MIN_EIGENVALS puts the G sums' smaller eigenvalue into err; OPTFLOW_USE_INITIAL_FLOW"""
    a = PAT[name]
    init = PTS + np.float32([1.5, -0.5])
    for kind in ("shift", "inverted"):
        b = X.pair(a, kind)
        for win, ml in LK_WINDOWS[impl][-2:] if impl == 2 else [(21, 2)]:
            g, ex, _ = run_pair(gpu, a, b, PTS, (win, win), ml, flags=O.OPTFLOW_LK_GET_MIN_EIGENVALS, impl=impl)
            lk_same(f"{name}/{kind} {IMPL_NAME[impl]} win {win} min-eigenvalue err", g, ex)
            same_bits(g[2], ex[2], f"{name}/{kind} {IMPL_NAME[impl]} win {win}: min-eigenvalue err at every point")
            g, ex, _ = run_pair(gpu, a, b, PTS, (win, win), ml, flags=O.OPTFLOW_USE_INITIAL_FLOW, init=init, impl=impl)
            lk_same(f"{name}/{kind} {IMPL_NAME[impl]} win {win} initial flow", g, ex)


# ---- the forward-backward call ----------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [("binblk", "shift"), ("check2", "shift"), ("zero", "same")])
@pytest.mark.parametrize("win,ml", [(21, 2), (5, 1)])
def test_lk_forward_backward(gpu, name, kind, win, ml):
    k = K()
    a, b = PAT[name], X.pair(PAT[name], kind)
    lk = k.SparsePyrLKOpticalFlow((win, win), ml, 30)
    Pa, Pb = k.build_pyramid(dev(a), (win, win), ml, ctx=gpu), k.build_pyramid(dev(b), (win, win), ml, ctx=gpu)
    g = fb_host(lk.calc_checked(Pa, Pb, dev(PTS), back_threshold=1.0, want_iters=True))
    pad = Pa.pyr.lv[0].pad
    ref = FBO.checked_trace(O.Pyramid(a, (win, win), ml, pad), O.Pyramid(b, (win, win), ml, pad), PTS, win, ml, 30,
                            0.01, 1e-4, 1.0, O.ACCUM_EXACT)
    what = f"{name}/{kind} calc_checked win {win}"
    same_bits(g["status"], ref.status, f"{what}: checked status")
    same_bits(g["iters"], ref.iters, f"{what}: iters")
    ok = ref.fwd_status == 1
    same_bits(g["next_pts"][ok], ref.next_pts[ok], f"{what}: next_pts of the points tracked forward")
    same_bits(g["err"][ok], ref.err[ok], f"{what}: err of the points tracked forward")
    same_bits(g["fb_err"], ref.fb_err, f"{what}: fb_err")
    back_equal(g, ref)
    same_bits(g["back_pts"][~ok], PTS[~ok], f"{what}: back_pts of the points lost forward")
    assert (ref.status.sum() == 0) == (name == "zero"), what


# ---- multi-channel PyrLK -----------------------------------------------------------------------------

CN_PATTERNS = ["zero", "check1", "check2", "binblk", "binary"]
CN_WINDOWS = [(21, 2), (63, 0)]


@pytest.mark.parametrize("cn", [3, 4])
@pytest.mark.parametrize("name", CN_PATTERNS)
def test_lk_cn_u8(gpu, name, cn):
    a = PAT[name]
    for kind in ("shift", "inverted"):
        A, B = X.to_cn(a, cn), X.to_cn(X.pair(a, kind), cn)
        for win, ml in CN_WINDOWS:
            g, ex, _ = run_pair_cn(gpu, A, B, PTS, (win, win), ml)
            lk_same(f"{name}/{kind} klt_cn cn {cn} win {win}", g, ex)


@pytest.mark.parametrize("name", CN_PATTERNS)
def test_lk_cn_f32_at_16_bit_white(gpu, name):
    k = K()
    a = PAT[name]
    for kind in ("shift", "inverted"):
        A, B = X.to_u16(X.to_cn(a, 3), 65535), X.to_u16(X.to_cn(X.pair(a, kind), 3), 65535)
        for win, ml in CN_WINDOWS:
            Pa, Pb = _cn_pyr(gpu, A, (win, win), ml), _cn_pyr(gpu, B, (win, win), ml)
            r = k.SparsePyrLKOpticalFlow((win, win), ml, 30).calc(Pa, Pb, dev(PTS), want_iters=True)
            g = (host(r.next_pts), host(r.status), host(r.err), host(r.iters))
            ex = O.lk16(O.Pyramid16(A, (win, win), ml, f32=True), O.Pyramid16(B, (win, win), ml, f32=True), PTS,
                        (win, win), ml)
            what = f"{name}/{kind} klt_cn_f32 cn 3 win {win}"
            for i, part in enumerate(("next_pts", "status", "err", "iters")):
                same_bits(g[i], ex[i], f"{what}: {part}")


# ---- dense PyrLK -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["zero", "full", "vstripe2", "check1", "check2", "binblk"])
def test_lk_dense(gpu, name):
    k = K()
    w, h = X.DENSE_SIZE
    a = X.patterns(w, h)[name]
    ys, xs = np.mgrid[0:h, 0:w]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    try:
        for kind in ("shift", "inverted"):
            b = X.pair(a, kind)
            nx, st, _, _ = O.lk(O.Pyramid(a, (13, 13), 2), O.Pyramid(b, (13, 13), 2), pts, win=(13, 13), max_level=2,
                                accum=O.ACCUM_EXACT, want_err=False)
            ref = (nx - pts).astype(np.float32)
            for case in (1, 0):
                gpu.set_option("lk_dense_case", case)
                flow, status = k.DensePyrLKOpticalFlow.create((13, 13), 2, 30).calc(dev(a), dev(b), want_status=True)
                flow, status = host(flow).reshape(-1, 2), host(status).ravel()
                what = f"{name}/{kind} dense lk_dense_case {case}"
                same_bits(status, st, f"{what}: status")
                same_bits(flow[st == 1], ref[st == 1], f"{what}: flow of the tracked pixels")
            assert (st.sum() == 0) == (name in X.FEATURELESS), f"{name}/{kind}: {int(st.sum())} pixels tracked"
    finally:
        gpu.set_option("lk_dense_case", 1)


# ---- GFTT and response maps --------------------------------------------------------------------------

RESPONSE_MODES = [(3, False), (3, True), (7, False), (7, True)]
ROIS = [(0, 0, W, H), (3, 5, 77, 51), (81, 7, 64, 101), (1, 61, 131, 57)]  # three cut the cells at odd offsets


@pytest.mark.parametrize("name", ALL)
def test_corner_response_maps(gpu, name):
    k = K()
    img = PAT[name]
    same_bits(k.corner_min_eigen_val(dev(img), ctx=gpu), O.min_eig(img), f"{name} cornerMinEigenVal")
    u16 = X.to_u16(img, 65535)
    for block, harris in RESPONSE_MODES:
        what = f"{name} block {block} {'Harris' if harris else 'min-eigenvalue'}"
        same_bits(k.corner_response(dev(img), block, harris, 0.04, ctx=gpu), O.corner_response(img, block, harris, 0.04),
                  f"{what} u8")
        with np.errstate(over="ignore", invalid="ignore"):
            ref = O32.response(u16, block, harris, 0.04)
        same_bits(k.corner_response(dev(u16), block, harris, 0.04, ctx=gpu), ref, f"{what} 16U at 65535")


@pytest.mark.parametrize("name", ALL)
def test_gftt_corner_lists(gpu, name):
    img = PAT[name]
    total = 0
    for md in (0.0, 3.0):
        for maxc in (50, 100000):
            c, n = gftt_detect(gpu, img, ROIS, maxc, 0.01, md)
            try:
                gftt_check(img, ROIS, c, n, maxc, 0.01, md)
            except AssertionError as e:
                raise AssertionError(f"{name} GFTT minDistance {md} maxCorners {maxc}: {e}") from None
            total += int(n.sum())
    assert (total == 0) == (name in X.FEATURELESS), f"{name}: {total} corners"


def test_gftt_check2_takes_the_wide_path_on_its_own(gpu):
    """18,096 exactly tied candidates (more than one workgroup's LDS holds) with
    gftt_wide at its default: only the address orders them"""
    img = PAT["check2"]
    for md, maxc in ((0.0, 100000), (0.0, 50), (3.0, 100000)):
        c, n = gftt_detect(gpu, img, ROIS[:1], maxc, 0.01, md)
        (want,) = O.gftt_rois(img, ROIS[:1], maxc, 0.01, md)
        assert n[0] == len(want), f"check2 minDistance {md} maxCorners {maxc}: count {n[0]} vs {len(want)}"
        same_bits(c[0, :n[0]], want, f"check2 wide GFTT minDistance {md} maxCorners {maxc}")
        if md == 0.0 and maxc == 100000:
            assert n[0] > 16384


@pytest.mark.parametrize("name", ["blocks", "binblk"])
def test_gftt_wide_path_equals_lds_path(gpu, name):
    img = PAT[name]
    for md, maxc in ((0.0, 100000), (3.0, 100000), (0.0, 50)):
        c0, n0 = gftt_detect(gpu, img, ROIS, maxc, 0.01, md)
        gpu.set_option("gftt_wide", 1)
        try:
            c1, n1 = gftt_detect(gpu, img, ROIS, maxc, 0.01, md)
        finally:
            gpu.set_option("gftt_wide", 0)
        same_bits(n1, n0, f"{name} gftt_wide 1 against 0, minDistance {md} maxCorners {maxc}: counts")
        for i in range(len(ROIS)):
            same_bits(c1[i, :n1[i]], c0[i, :n0[i]], f"{name} gftt_wide 1 against 0, minDistance {md}: ROI {i}")
        gftt_check(img, ROIS, c1, n1, maxc, 0.01, md)


# ---- cornerSubPix -------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", ["8u", "32f"])
@pytest.mark.parametrize("name", ["zero", "full", "check1", "check2", "binblk", "quadrant", "impulse"])
def test_corner_sub_pix(gpu, name, depth):
    k = K()
    img = PAT[name] if depth == "8u" else PAT[name].astype(np.float32)
    g = X.grid(W, H)
    pts = np.concatenate([g + np.float32(0.37), g])
    for half in (2, 5, 10):
        got = k.corner_sub_pix(dev(img), dev(pts), (half, half), (-1, -1), (3, 20, 0.03), ctx=gpu)
        same_bits(got, SO.corner_sub_pix(img, pts, (half, half), (-1, -1), (3, 20, 0.03)),
                  f"{name} cornerSubPix {depth} half-window {half}")


# ---- warpAffine ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["vstripe2", "check1", "blocks", "binblk", "impulse", "hole"])
def test_warp_affine(gpu, name):
    k = K()
    src = X.patterns(*X.SMALL_SIZE)[name]
    c, s = 1.3 * np.cos(0.3), 1.3 * np.sin(0.3)
    M = np.array([[c, -s, 3.25], [s, c, -20.5]])
    init = np.random.default_rng(7).integers(0, 256, (50, 80), dtype=np.uint8)  # BORDER_TRANSPARENT keeps it
    for inter in (O.INTER_NEAREST, O.INTER_LINEAR, O.INTER_CUBIC, O.INTER_AREA):
        for border in range(6):
            for inverse in (0, O.WARP_INVERSE_MAP):
                got = k.warp_affine(dev(src), M, (80, 50), inter | inverse, border, 77, dst=dev(init), ctx=gpu)
                same_bits(got, O.warp_affine(src, M, (80, 50), inter | inverse, border, 77, dst=init),
                          f"{name} warpAffine interpolation {inter} border {border} inverse {bool(inverse)}")


# ---- remap, warpPerspective, remap_flow ---------------------------------------------------------------

def _smooth_map(sw, sh, dw, dh):
    """the destination grid scaled onto the source plus seeded jitter of +-3 px; float32 (dh, dw, 2)"""
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    j = np.random.default_rng(11).uniform(-3, 3, (dh, dw, 2))
    return np.ascontiguousarray(np.stack([x * sw / dw + j[..., 0], y * sh / dh + j[..., 1]], -1).astype(np.float32))


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("name", ["binblk", "check1", "blocks"])
def test_remap_family(gpu, name, cn):
    k = K()
    sw, sh = X.SMALL_SIZE
    dw, dh = 80, 50
    a = X.patterns(sw, sh)[name]
    src = a if cn == 1 else X.to_cn(a, cn)
    dst = np.zeros((dh, dw) + src.shape[2:], np.uint8)
    m = _smooth_map(sw, sh, dw, dh)
    grid = np.stack(np.broadcast_arrays(np.arange(dw, dtype=np.float32)[None, :],
                                        np.arange(dh, dtype=np.float32)[:, None]), -1)
    flow = np.ascontiguousarray((m - grid).astype(np.float32))
    M = PC.matrix("mild", sw, sh, dw, dh)
    bv = PC.BORDER_VALUE
    for inter in (R.INTER_NEAREST, R.INTER_LINEAR, R.INTER_CUBIC):
        for border in (R.BORDER_CONSTANT, R.BORDER_REPLICATE, R.BORDER_REFLECT_101):
            what = f"{name} cn {cn} interpolation {inter} border {border}"
            same_bits(k.remap(dev(src), dev(m), None, inter, border, bv, dst=dev(dst), ctx=gpu),
                      R.remap(src, dst, m, None, R.MAP_32FC2, inter, border, bv), f"{what} remap")
            same_bits(k.remap_flow(dev(src), dev(flow), 1, inter, border, bv, dst=dev(dst), ctx=gpu),
                      R.remap_flow(src, dst, flow, 1, inter, border, bv), f"{what} remap_flow")
            for inverse in (0, R.WARP_INVERSE_MAP):
                same_bits(k.warp_perspective(dev(src), M, (dw, dh), inter | inverse, border, bv, dst=dev(dst), ctx=gpu),
                          R.warp_perspective(src, dst, M, inter | inverse, border, bv),
                          f"{what} warpPerspective inverse {bool(inverse)}")


# ---- front end -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["binary", "check1", "full", "zero"])
def test_front_end(gpu, name):
    k = K()
    bgr = X.to_cn(X.patterns(*X.SMALL_SIZE)[name], 3)
    t = dev(bgr)
    for code in sorted(c for c, n in FE.SRC_CN.items() if n == 3):
        same_bits(k.cvt_color(t, code, ctx=gpu), FE.cvt_color(bgr, code), f"{name} cvt_color code {code}")
    gray = FE.cvt_color(bgr, FE.COLOR_BGR2GRAY)
    for dsize in ((53, 31), (160, 120)):
        same_bits(k.resize_linear(t, dsize, ctx=gpu), FE.resize_linear(bgr, dsize), f"{name} resize_linear cn 3 to {dsize}")
        same_bits(k.resize_linear(dev(gray), dsize, ctx=gpu), FE.resize_linear(gray, dsize),
                  f"{name} resize_linear gray to {dsize}")
        for code in (FE.COLOR_BGR2GRAY, FE.COLOR_RGB2GRAY):
            same_bits(k.cvt_resize_gray(t, code, dsize, ctx=gpu), FE.cvt_resize_gray(bgr, code, dsize),
                      f"{name} cvt_resize_gray code {code} to {dsize}")


# ---- Farneback ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_farneback_stages(gpu, name):
    from opencv_amd import farneback as F

    even = X.patterns(*X.DENSE_SIZE)[name]  # 96x64 -> 48x32: the exact 2x path
    odd = X.patterns(*X.SMALL_SIZE)[name]   # 97x61 -> 31x20: a ragged ratio on both axes
    for img, dst, ks, sigma in ((even, (48, 32), 3, 0.5), (odd, (31, 20), 9, 1.5), (odd, X.SMALL_SIZE, 3, 0.0)):
        same_bits(F.level_image(dev(img), dst, ks, sigma, ctx=gpu), O.fb_level_image(img, dst, ks, sigma),
                  f"{name} level_image {img.shape[::-1]} -> {dst}")
    lvl = odd.astype(np.float32)
    for n, sigma in ((5, 1.1), (7, 1.5)):
        same_bits(F.poly_exp(dev(lvl), n, sigma, ctx=gpu), O.fb_poly_exp(lvl, n, sigma), f"{name} poly_exp n {n}")


@pytest.mark.parametrize("flags", [0, O.FARNEBACK_GAUSSIAN], ids=["box", "gauss"])
@pytest.mark.parametrize("name", ALL)
def test_farneback_flow(gpu, name, flags):
    a = X.patterns(*X.SMALL_SIZE)[name]
    for kind in X.PAIRS:
        b = X.pair(a, kind)
        ref = O.farneback(a, b, levels=3, iterations=3, flags=flags, box_direct=flags == 0)
        same_bits(_gpu_flow(gpu, a, b, numLevels=3, numIters=3, flags=flags), ref, f"{name}/{kind} Farneback flags {flags}")


def test_farneback_initial_flow(gpu):
    a = X.patterns(*X.SMALL_SIZE)["binblk"]
    b = X.pair(a, "shift")
    init = np.empty(a.shape + (2,), np.float32)
    init[...] = np.float32([2.5, -1.25])
    for flags in (O.OPTFLOW_USE_INITIAL_FLOW, O.OPTFLOW_USE_INITIAL_FLOW | O.FARNEBACK_GAUSSIAN):
        ref = O.farneback(a, b, levels=3, iterations=3, flags=flags, box_direct=not flags & O.FARNEBACK_GAUSSIAN,
                          init_flow=init)
        same_bits(_gpu_flow(gpu, a, b, init=init, numLevels=3, numIters=3, flags=flags), ref,
                  f"binblk/shift Farneback initial flow flags {flags}")


# ---- HOG ---------------------------------------------------------------------------------------------------

HOG_PATTERNS = ["zero", "full", "check1", "vstripe2", "binary", "quadrant"]


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("name", HOG_PATTERNS)
def test_hog_gradient_and_blocks(gpu, name, cn):
    from opencv_amd import hog

    a = X.patterns(*X.HOG_SIZE)[name]
    img = a if cn == 1 else X.to_cn(a, 3)
    hg = hog.HOG.create(ctx=gpu)
    for gamma in (True, False):
        for signed in (False, True):
            hg.setGammaCorrection(gamma)
            hg.setSignedGradient(signed)
            g, q = hog.gradient(dev(img), hg, ctx=gpu)
            og, oq = O.hog_gradient(img, nbins=9, gamma=gamma, signed=signed)
            what = f"{name} cn {cn} gamma {gamma} signed {signed}"
            same_bits(q, oq, f"{what} HOG bins")
            same_bits(g, og, f"{what} HOG gradient magnitudes")
            B = hog.blocks(dev(og), dev(oq), hg, ctx=gpu)
            same_bits(B, O.hog_blocks(og, oq, hog_prm(hg)), f"{what} HOG block histograms")


@pytest.mark.parametrize("win", [(48, 96), (64, 128)], ids=["daimler48x96", "random64x128"])
@pytest.mark.parametrize("name", HOG_PATTERNS)
def test_hog_window_scores(gpu, name, win):
    """every window's score, not only the hits; zero and full are the zero-energy block normalisation"""
    from opencv_amd import hog

    a = X.patterns(*X.HOG_SIZE)[name]
    hg = hog.HOG.create(win, ctx=gpu)
    if win == (48, 96):
        hg.setSVMDetector(hg.getDefaultPeopleDetector())
    else:
        hg.setSVMDetector((np.random.default_rng(64128).standard_normal(hg.getDescriptorSize() + 1) * 0.05)
                          .astype(np.float32))
    hg.setHitThreshold(-1e9)
    for cn in (1, 3):
        img = a if cn == 1 else X.to_cn(a, 3)
        xy, sc = hg.detect(dev(img), confidences=True)
        oxy, osc = O.hog_detect(img, hog_prm(hg), hg.svm, hit_threshold=-1e9)
        what = f"{name} cn {cn} HOG {win[0]}x{win[1]}"
        assert len(oxy) == ((X.HOG_SIZE[0] - win[0]) // 8 + 1) * ((X.HOG_SIZE[1] - win[1]) // 8 + 1), what
        same_bits(np.array(xy, np.int32).reshape(-1, 2), oxy, f"{what} window positions")
        same_bits(np.array(sc, np.float64), osc, f"{what} window scores")


# ---- the float pixel paths at the ends of their range -------------------------------------------------------

def _fp_lk(gpu, a, b, dtype, win=21, ml=2):
    k = K()
    Pa = k.Pyramid(gpu, W, H, ml, (win, win), dtype).build(dev(a))
    Pb = k.Pyramid(gpu, W, H, ml, (win, win), dtype).build(dev(b))
    r = k.SparsePyrLKOpticalFlow((win, win), ml, 30).calc(Pa, Pb, dev(PTS), want_iters=True)
    g = (host(r.next_pts), host(r.status), host(r.err), host(r.iters))
    f32 = dtype == torch.float32
    Ra, Rb = O.Pyramid16(a, (win, win), ml, f32=f32), O.Pyramid16(b, (win, win), ml, f32=f32)
    return g, O.lk16(Ra, Rb, PTS, (win, win), ml), (Pa, Pb), (Ra, Rb)


def _fp_same(what, g, ex, nan_any=False):
    for i, part in enumerate(("next_pts", "status", "err", "iters")):
        same_bits(g[i], ex[i], f"{what}: {part}", nan_any=nan_any and i in (0, 2))
    bad = (g[1] == 1) & ~(np.isfinite(g[0]).all(1) & np.isfinite(g[2]))
    assert not bad.any(), f"{what}: status 1 with a non-finite result at points {np.flatnonzero(bad)[:8].tolist()}"


@pytest.mark.parametrize("name", ["binblk", "check2", "vstripe2", "quadrant"])
def test_f16_in_range(gpu, name):
    """0 / 4094: the largest 12-bit step whose Scharr value (16 * 4094 = 65504) is a finite fp16"""
    a = X.to_u16(PAT[name], 4094).astype(np.float16)
    b = X.to_u16(X.pair(PAT[name], "shift"), 4094).astype(np.float16)
    g, ex, (Pa, _), (Ra, _) = _fp_lk(gpu, a, b, torch.float16)
    _fp_pyramid_same(f"{name} fp16 at 4094", Pa, Ra)
    assert all(np.isfinite(d.astype(np.float32)).all() for d in Ra.derivs)
    _fp_same(f"{name}/shift lk_f16 at 4094", g, ex)
    assert (g[1].sum() == 0) == (name == "vstripe2"), name


@pytest.mark.parametrize("top", [4095, 65504])
@pytest.mark.parametrize("name", ["binblk", "check2", "vstripe2", "quadrant"])
def test_f16_out_of_range_pyramids(gpu, name, top):
    """beyond 4094 a hard edge's derivative rounds to an fp16 infinity: rounding only, so
    levels and planes stay bit-exact, infinities included"""
    a = X.to_u16(PAT[name], top).astype(np.float16)
    P = K().Pyramid(gpu, W, H, 2, (21, 21), torch.float16).build(dev(a))
    torch.cuda.synchronize()
    Rf = O.Pyramid16(a, (21, 21), 2)
    assert np.isinf(Rf.derivs[0].astype(np.float32)).any() and not np.isnan(Rf.derivs[0].astype(np.float32)).any()
    _fp_pyramid_same(f"{name} fp16 at {top}", P, Rf)


@pytest.mark.parametrize("top", [4095, 65504])
def test_f16_out_of_range_lk(gpu, top):
    """The derivative planes hold infinities, so G, the step and the window position
    become NaN.  The rule (oracle/klt16_oracle.c out_of_level, lk_device.hpp
    out_of_level): a non-finite window position fails the bounds gate, status 0
    at level 0, the iteration ends; no point has status 1 and a non-finite result.

    Why no window position can index memory, whatever its value.  lk_f16_kernel
    (klt_f16.hip) converts a position with (int)floorf: +-Inf saturate to
    INT_MAX / INT_MIN, a NaN gives 0.  Its loads are the window of I and the
    derivative planes (offsets from ipx, ipy), the first window of J (pinx,
    piny), the window of J in the iteration (inx, iny) and in the error pass
    (inx, iny).  Each offset is computed under `act ? ... : 0` / `jin ? ... : 0`
    / `want ? ... : 0`, and act, jin and want are only true after the bounds
    gate -win <= ix < w, -win <= iy < h passed on those very integers, so an
    offset is either 0 or inside the padded level (pad >= win + 2); a saturated
    value fails the gate, and 0 (from NaN) lies inside the level.  Every load
    also goes through a buffer resource sized to the padded level, which returns
    0 beyond its range.  The only stores are the point's own outputs, indexed
    by the point.  lk_cn_f32_kernel (klt_cn_f32.hip) loads through plain
    pointers, each inside `if (gate failed) continue / break / else`, again on
    the converted integers.  The gate now also names NaN, so the integers are
    not even used for one."""
    a = X.to_u16(PAT["binblk"], top).astype(np.float16)
    for kind in ("shift", "inverted"):
        b = X.to_u16(X.pair(PAT["binblk"], kind), top).astype(np.float16)
        g, ex, _, _ = _fp_lk(gpu, a, b, torch.float16)
        _fp_same(f"binblk/{kind} lk_f16 at {top}", g, ex, nan_any=True)
        assert ex[1].sum() == 0, f"the oracle tracks {int(ex[1].sum())} points at {top}"


@pytest.mark.parametrize("name", ["binblk", "check2", "vstripe2", "quadrant"])
def test_f32_at_16_bit_white(gpu, name):
    a, b = X.to_u16(PAT[name], 65535), X.to_u16(X.pair(PAT[name], "shift"), 65535)
    g, ex, (Pa, _), (Ra, _) = _fp_lk(gpu, a, b, torch.float32)
    _fp_pyramid_same(f"{name} fp32 from 16U at 65535", Pa, Ra)
    _fp_same(f"{name}/shift lk fp32 at 65535", g, ex)
    assert (g[1].sum() == 0) == (name == "vstripe2"), name


def test_f32_tiny_scale_fails_the_min_eigenvalue_gate(gpu):
    a = PAT["binblk"].astype(np.float32) * np.float32(1e-30)
    b = X.pair(PAT["binblk"], "shift").astype(np.float32) * np.float32(1e-30)
    g, ex, (Pa, _), (Ra, _) = _fp_lk(gpu, a, b, torch.float32)
    _fp_pyramid_same("binblk fp32 scaled by 1e-30", Pa, Ra)
    _fp_same("binblk/shift lk fp32 scaled by 1e-30", g, ex)
    assert g[1].sum() == 0


def test_f32_overflowing_squares(gpu):
    """pixels of 2.55e20: the derivative planes are finite (4e21) but their squares
    overflow, G is Inf / NaN and so is the step: the rule and the argument of
    test_f16_out_of_range_lk (the fp32 path is the same kernel on fp32 storage)"""
    a = PAT["binblk"].astype(np.float32) * np.float32(1e18)
    for kind in ("shift", "inverted"):
        b = X.pair(PAT["binblk"], kind).astype(np.float32) * np.float32(1e18)
        g, ex, (Pa, _), (Ra, _) = _fp_lk(gpu, a, b, torch.float32)
        assert all(np.isfinite(d).all() for d in Ra.derivs)
        _fp_pyramid_same("binblk fp32 scaled by 1e18", Pa, Ra)
        _fp_same(f"binblk/{kind} lk fp32 scaled by 1e18", g, ex, nan_any=True)
        assert ex[1].sum() == 0
