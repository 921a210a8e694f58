"""No result may depend on what the library's device memory held before the call.

Three ways to put hostile content there, each against the existing oracles, bit
for bit (same_bits; sparse PyrLK results by the suite's rule, assert_exact):

  context scratch     the call runs once so the scratch exists at its size, then
                      Context.debug_fill_scratch(byte) fills every buffer the session
                      context owns over its whole capacity and forgets every cache,
                      and the call runs again.  The reported byte count is at least
                      what the shape needs, so the fill reached the memory.
  history             a larger, brighter, busier frame with other parameters, the
                      small case, the larger frame again: what the scratch holds
                      beyond the small case's extent is the larger call's.
  fresh allocations   a new Context with option alloc_fill: every allocation the
                      library makes for it and for the objects created from it
                      starts as the byte instead of the zeros a new process sees.

The bytes: 0xFF is a float / double NaN, int -1, pixel 255; 0x7F a float 3.39e38,
double 1.4e306, int 2139062143: finite values that win every maximum.

DESIGN.md (test strategy, "Scratch and fresh memory") lists per buffer the kernel
that writes it, the kernels that read it and what bounds the read."""
import numpy as np
import pytest
import torch

import _extreme_cases as X
import _frontend_oracle as FE
import _gftt_f32_oracle as O32
import _gftt_mask_cases as MC
import _gftt_mask_oracle as MO
import _klt_tracker_oracle as KO
import _loop_pair as LP
import _mog2_cases as GC
import _mog2_oracle as M2
import _oracle as O
from test_gpu_extreme import _fp_pyramid_same, dev, host, same_bits
from test_gpu_farneback import _gpu_flow
from test_gpu_hog import _bgr, _hog, _prm
from test_gpu_klt import assert_exact, run_pair
from test_gpu_klt_cn import run_pair_cn
from test_gpu_klt_tracker import assert_state
from test_gpu_lk_fb import back_equal, host as fb_host
from test_gpu_mog2 import assert_model, model_of, run as mog2_run, subtractor

pytestmark = pytest.mark.gpu

BYTES = [0xFF, 0x7F]
byte_param = pytest.mark.parametrize("byte", BYTES, ids=["ff", "7f"])


def K():
    from opencv_amd import klt

    return klt


_cache = {}


def cached(key, make):
    """a reference computed once and shared (read only)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class options:
    """context options on for a block, back at the given defaults after it"""

    def __init__(self, ctx, on, off):
        self.ctx, self.on, self.off = ctx, on, off

    def __enter__(self):
        for k, v in self.on.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.on:
            self.ctx.set_option(k, self.off[k])


DEFAULTS = {"gftt_wide": 0, "gftt_compact": 1, "gftt_inline": 1, "fb_prep_ahead": 1, "hog_level_streams": 3,
            "hog_block_tiled": 1, "lk_dense_case": 1}


def dirty_twice(gpu, byte, call, check, min_bytes, what):
    """call once (the scratch exists), fill, call again; both results checked"""
    check(call(), f"{what}, first call")
    n = gpu.debug_fill_scratch(byte)
    assert n >= min_bytes, f"{what}: {n} bytes filled, the call's scratch alone is {min_bytes}"
    check(call(), f"{what}, after the scratch was filled with {byte:#x}")


# ---- frames ------------------------------------------------------------------------------------------

def small_frame():
    return cached("small", lambda: np.ascontiguousarray(O.synth(20261020, 160, 120, 6, 0, 1)[0][0]))


def large_frame():
    """320x240, brighter and busier: more objects, gain and hashed noise"""
    def make():
        f = O.synth(20261021, 320, 240, 24, 0, 1)[0][0].astype(np.int32)
        n = FE.pattern(320, 240, 1, 911).astype(np.int32) % 41 - 20
        return np.clip(f * 3 // 2 + 50 + n, 0, 255).astype(np.uint8)

    return cached("large", make)


# one ROI touches the right and the bottom edge of the frame, one is 5x5
ROIS = [(101, 71, 59, 49), (7, 9, 5, 5), (20, 15, 77, 51)]
LARGE_ROIS = [(0, 0, 320, 240), (3, 5, 150, 111), (170, 100, 150, 140), (100, 7, 113, 57)]
GFTT_PRM = (200, 0.01, 2.0)
ROI_PX = sum(w * h for _, _, w, h in ROIS)


def gftt_call(ctx, img, rois, prm, mask=None, block=3, harris=False):
    det = K().GoodFeaturesToTrackDetector(prm[0], prm[1], prm[2], block, harris, 0.04)
    c, n = det.detect_rois(img, rois, mask=mask)
    torch.cuda.synchronize()
    return c.cpu().numpy(), n.cpu().numpy()


def lists_same(got, ref, what):
    c, n = got
    assert len(ref) == len(n), what
    for i, r in enumerate(ref):
        assert n[i] == len(r), f"{what} ROI {i}: count {n[i]} vs {len(r)}"
        same_bits(c[i, :n[i]], np.asarray(r, np.float32).reshape(-1, 2), f"{what} ROI {i}")


# ---- context scratch: GFTT ---------------------------------------------------------------------------------

GFTT_U8 = {"default": ({}, 3, False), "wide": ({"gftt_wide": 1}, 3, False), "dense_plane": ({"gftt_compact": 0}, 3, False),
           "table_in_memory": ({"gftt_inline": 0}, 3, False), "block5": ({}, 5, False), "harris": ({}, 3, True)}


@byte_param
@pytest.mark.parametrize("variant", list(GFTT_U8))
def test_scratch_gftt_u8(gpu, variant, byte):
    opts, block, harris = GFTT_U8[variant]
    img = small_frame()
    ref = cached(("gftt", block, harris), lambda: O.gftt_rois(img, ROIS, *GFTT_PRM, block, harris, 0.04))
    assert sum(len(r) for r in ref) > 0
    t = dev(img)
    with options(gpu, opts, DEFAULTS):
        dirty_twice(gpu, byte, lambda: gftt_call(gpu, t, ROIS, GFTT_PRM, None, block, harris),
                    lambda g, what: lists_same(g, ref, what), 4 * ROI_PX, f"GFTT {variant}")


@byte_param
def test_scratch_gftt_masked(gpu, byte):
    img = small_frame()
    mask = MC.checker(160, 120, 8)
    ref = cached("gftt_mask", lambda: MO.gftt_rois_masked(img, mask, ROIS, *GFTT_PRM))
    assert sum(len(r) for r in ref) > 0
    t, m = dev(img), dev(mask)
    dirty_twice(gpu, byte, lambda: gftt_call(gpu, t, ROIS, GFTT_PRM, m), lambda g, what: lists_same(g, ref, what),
                4 * ROI_PX, "GFTT under a mask")


@byte_param
@pytest.mark.parametrize("depth", ["32f", "16u"])
def test_scratch_gftt_and_response_on_float_frames(gpu, depth, byte):
    base = small_frame()
    img = (base.astype(np.float32) * np.float32(1.0 / 255) if depth == "32f"
           else (base.astype(np.uint16) * np.uint16(257)))
    ref = cached(("gftt32", depth), lambda: O32.gftt_rois(img, None, ROIS, *GFTT_PRM, 3, False, 0.04))
    assert sum(len(r) for r in ref) > 0
    t = dev(img)
    dirty_twice(gpu, byte, lambda: gftt_call(gpu, t, ROIS, GFTT_PRM), lambda g, what: lists_same(g, ref, what),
                4 * ROI_PX, f"GFTT {depth}")
    for block, harris in ((3, False), (5, True)):
        def make():
            with np.errstate(over="ignore", invalid="ignore"):
                return O32.response(img, block, harris, 0.04)

        want = cached(("resp32", depth, block, harris), make)
        dirty_twice(gpu, byte, lambda: host(K().corner_response(t, block, harris, 0.04, ctx=gpu)),
                    lambda g, what: same_bits(g, want, what), 4 * 160 * 120,
                    f"corner_response {depth} block {block} harris {harris}")


@byte_param
def test_scratch_corner_min_eigen_val(gpu, byte):
    img = small_frame()
    want = cached("mineig", lambda: O.min_eig(img))
    t = dev(img)
    dirty_twice(gpu, byte, lambda: host(K().corner_min_eigen_val(t, ctx=gpu)), lambda g, what: same_bits(g, want, what),
                4 * 160 * 120, "cornerMinEigenVal")


# ---- context scratch: Farneback ----------------------------------------------------------------------------

FB_W, FB_H = X.SMALL_SIZE  # 97x61
FB_FLAGS = {"box": 0, "gauss": O.FARNEBACK_GAUSSIAN, "box_init": O.OPTFLOW_USE_INITIAL_FLOW,
            "gauss_init": O.FARNEBACK_GAUSSIAN | O.OPTFLOW_USE_INITIAL_FLOW}


def fb_pair():
    def make():
        fr = O.synth(20261022, FB_W, FB_H, 4, 0, 2)[0]
        return np.ascontiguousarray(fr[0]), np.ascontiguousarray(fr[1])

    return cached("fb_pair", make)


def fb_init():
    init = np.empty((FB_H, FB_W, 2), np.float32)
    init[...] = np.float32([1.5, -0.75])
    return init


@byte_param
@pytest.mark.parametrize("ahead", [1, 0])
@pytest.mark.parametrize("levels", [3, 0])
@pytest.mark.parametrize("variant", list(FB_FLAGS))
def test_scratch_farneback(gpu, variant, levels, ahead, byte):
    flags = FB_FLAGS[variant]
    a, b = fb_pair()
    init = fb_init() if flags & O.OPTFLOW_USE_INITIAL_FLOW else None
    ref = cached(("fb", variant, levels), lambda: O.farneback(a, b, levels=levels, iterations=2, flags=flags,
                                                              box_direct=not flags & O.FARNEBACK_GAUSSIAN,
                                                              init_flow=init))
    with options(gpu, {"fb_prep_ahead": ahead}, DEFAULTS):
        dirty_twice(gpu, byte, lambda: _gpu_flow(gpu, a, b, init=init, numLevels=levels, numIters=2, flags=flags),
                    lambda g, what: same_bits(g, ref, what), 15 * 4 * FB_W * FB_H,
                    f"Farneback {variant} levels {levels} fb_prep_ahead {ahead}")


@byte_param
@pytest.mark.parametrize("shape", [(5, 7), (61, 97)])
def test_scratch_farneback_stages(gpu, shape, byte):
    from opencv_amd import farneback as F

    h, w = shape
    img = FE.pattern(w, h, 1, 77)
    lvl = img.astype(np.float32)
    # the small one blurred at its own size (level 0), the other resized by a ragged ratio on both axes
    dst, ks, sigma = ((w, h), 3, 0.0) if shape == (5, 7) else ((31, 20), 9, 1.5)
    want_l = cached(("fbl", shape), lambda: O.fb_level_image(img, dst, ks, sigma))
    want_p = cached(("fbp", shape), lambda: O.fb_poly_exp(lvl, 5, 1.1))
    ti, tl = dev(img), dev(lvl)
    dirty_twice(gpu, byte, lambda: host(F.level_image(ti, dst, ks, sigma, ctx=gpu)),
                lambda g, what: same_bits(g, want_l, what), 0, f"level_image {shape}")
    dirty_twice(gpu, byte, lambda: host(F.poly_exp(tl, 5, 1.1, ctx=gpu)),
                lambda g, what: same_bits(g, want_p, what), 0, f"poly_exp {shape}")


# ---- context scratch: dense PyrLK ---------------------------------------------------------------------------

DW, DH = 64, 48


def dense_pair():
    def make():
        fr = O.synth(20261023, DW, DH, 3, 0, 2)[0]
        return np.ascontiguousarray(fr[0]), np.ascontiguousarray(fr[1])

    return cached("dense_pair", make)


def dense_ref(win):
    def make():
        a, b = dense_pair()
        ys, xs = np.mgrid[0:DH, 0:DW]
        pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
        nx, st, _, _ = O.lk(O.Pyramid(a, win, 2), O.Pyramid(b, win, 2), pts, win=win, max_level=2,
                            accum=O.ACCUM_EXACT, want_err=False)
        return (nx - pts).astype(np.float32), st

    return cached(("dense", win), make)


@byte_param
@pytest.mark.parametrize("win", [(7, 7), (9, 7)], ids=["case_images_7", "per_pixel_9x7"])
def test_scratch_dense_pyrlk(gpu, win, byte):
    a, b = dense_pair()
    ref, st = dense_ref(win)
    assert 0 < st.sum()
    ta, tb = dev(a), dev(b)
    n = DW * DH
    # the case images: level 0 alone is (w + 2 B) (h + 2 B) uint2; the per-pixel scratch 17 n + 256
    need = (DW + 6) * (DH + 6) * 8 if win == (7, 7) else 17 * n + 256

    def call():
        flow, status = K().DensePyrLKOpticalFlow.create(win, 2, 30).calc(ta, tb, want_status=True)
        return host(flow).reshape(-1, 2), host(status).ravel()

    def check(g, what):
        same_bits(g[1], st, f"{what}: status")
        same_bits(g[0][st == 1], ref[st == 1], f"{what}: flow of the tracked pixels")

    dirty_twice(gpu, byte, call, check, need, f"dense PyrLK window {win}")


# ---- context scratch: HOG ------------------------------------------------------------------------------------

# thresholds at which the oracle alone finds windows on these frames (33 and 97 on the small one)
HOG_HIT = {(64, 128): -2.0, (48, 96): -1.0}


def hog_multi(gpu, img, win):
    hit = HOG_HIT[win]
    hg = _hog(gpu, win)
    hg.setNumLevels(15)
    hg.setHitThreshold(hit)
    hg.setGroupThreshold(0)
    t = dev(img)

    def call():
        return sorted(zip(*hg.detectMultiScale(t, confidences=True)))

    def make():
        r, w = O.hog_detect_multiscale(img, _prm(hg), hg.svm, hit_threshold=hit, nlevels=15, scale0=1.05,
                                       group_threshold=0)
        return sorted(zip(map(tuple, r.tolist()), w.tolist()))

    return call, cached(("hogms", img.shape, win, hit), make)


def hog_same(g, ref, what):
    assert len(g) == len(ref), f"{what}: {len(g)} detections vs {len(ref)}"
    assert g == ref, what


@byte_param
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("win", [(64, 128), (48, 96)])
def test_scratch_hog_detect_multiscale(gpu, win, lanes, byte):
    img = cached("hog200", lambda: _bgr(41, 200, 280, cn=3))
    call, ref = hog_multi(gpu, img, win)
    assert len(ref) > 0
    with options(gpu, {"hog_level_streams": lanes}, DEFAULTS):
        dirty_twice(gpu, byte, call, lambda g, what: hog_same(g, ref, what), 14 * 200 * 280,
                    f"HOG detectMultiScale {win} lanes {lanes}")


@byte_param
@pytest.mark.parametrize("win", [(64, 128), (48, 96)])
def test_scratch_hog_detect_every_window(gpu, win, byte):
    w, h = X.HOG_SIZE
    img = cached("hog96", lambda: _bgr(43, w, h, cn=3))
    hg = _hog(gpu, win)
    hg.setHitThreshold(-1e9)
    oxy, osc = cached(("hogdet", win), lambda: O.hog_detect(img, _prm(hg), hg.svm, hit_threshold=-1e9))
    t = dev(img)

    def check(g, what):
        same_bits(np.array(g[0], np.int32).reshape(-1, 2), oxy, f"{what}: window positions")
        same_bits(np.array(g[1], np.float64), osc, f"{what}: window scores")

    dirty_twice(gpu, byte, lambda: hg.detect(t, confidences=True), check, 14 * w * h, f"HOG detect {win}")


@byte_param
@pytest.mark.parametrize("tiled", [0, 1, 2])
def test_scratch_hog_blocks(gpu, tiled, byte):
    from opencv_amd import hog

    img = cached("hogblk", lambda: _bgr(47, 151, 97, cn=1))
    hg = hog.HOG.create(ctx=gpu)
    og, oq = cached("hoggrad", lambda: O.hog_gradient(img, nbins=9))
    want = cached("hogblocks", lambda: O.hog_blocks(og, oq, _prm(hg)))
    G, Q = dev(og), dev(oq)
    with options(gpu, {"hog_block_tiled": tiled}, DEFAULTS):
        dirty_twice(gpu, byte, lambda: host(hog.blocks(G, Q, hg, ctx=gpu)), lambda g, what: same_bits(g, want, what),
                    0, f"HOG blocks hog_block_tiled {tiled}")


# ---- context scratch: the front end ------------------------------------------------------------------------------

@byte_param
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_scratch_resize_linear(gpu, cn, byte):
    src = FE.pattern(90, 70, cn, 800 + cn)
    want = cached(("resize", cn), lambda: FE.resize_linear(src, (31, 20)))
    t = dev(src)
    dirty_twice(gpu, byte, lambda: host(K().resize_linear(t, (31, 20), ctx=gpu)),
                lambda g, what: same_bits(g, want, what), 12 * (31 + 20), f"resize_linear cn {cn}")


@byte_param
@pytest.mark.parametrize("dsize", [(31, 20), (45, 35)], ids=["ragged", "exact2x"])
def test_scratch_cvt_resize_gray(gpu, dsize, byte):
    src = FE.pattern(90, 70, 3, 830)
    want = cached(("cvtresize", dsize), lambda: FE.cvt_resize_gray(src, FE.COLOR_BGR2GRAY, dsize))
    t = dev(src)
    dirty_twice(gpu, byte, lambda: host(K().cvt_resize_gray(t, FE.COLOR_BGR2GRAY, dsize, ctx=gpu)),
                lambda g, what: same_bits(g, want, what), 0, f"cvt_resize_gray to {dsize}")


# ---- history, without the hook ------------------------------------------------------------------------------------

def test_history_gftt(gpu):
    big, small = large_frame(), small_frame()
    big_prm = (1000, 0.001, 0.0)
    ref_big = cached("gftt_big", lambda: O.gftt_rois(big, LARGE_ROIS, *big_prm, 5, True, 0.04))
    ref_small = cached(("gftt", 3, False), lambda: O.gftt_rois(small, ROIS, *GFTT_PRM, 3, False, 0.04))
    tb, ts = dev(big), dev(small)
    lists_same(gftt_call(gpu, tb, LARGE_ROIS, big_prm, None, 5, True), ref_big, "large frame, first")
    lists_same(gftt_call(gpu, ts, ROIS, GFTT_PRM), ref_small, "small case after the large frame")
    lists_same(gftt_call(gpu, tb, LARGE_ROIS, big_prm, None, 5, True), ref_big, "large frame again")


def test_history_gftt_40_rois_then_2(gpu):
    big = large_frame()
    many = [(8 * (i % 10) + 3 * (i // 10), 5 * (i // 10) + (i % 7), 57 + i, 30 + (i * 5) % 23) for i in range(40)]
    assert all(x + w <= 320 and y + h <= 240 for x, y, w, h in many)
    two = [(150, 100, 61, 40), (315, 235, 5, 5)]
    prm = (300, 0.01, 1.0)
    ref_many = cached("gftt_many", lambda: O.gftt_rois(big, many, *prm))
    ref_two = cached("gftt_two", lambda: O.gftt_rois(big, two, *prm))
    t = dev(big)
    for wide in (0, 1):
        with options(gpu, {"gftt_wide": wide}, DEFAULTS):
            lists_same(gftt_call(gpu, t, many, prm), ref_many, f"40 ROIs, gftt_wide {wide}")
            lists_same(gftt_call(gpu, t, two, prm), ref_two, f"2 ROIs after 40, gftt_wide {wide}")


def test_history_farneback(gpu):
    big = large_frame()
    big_b = np.ascontiguousarray(np.roll(big, (2, -3), axis=(0, 1)))
    a, b = fb_pair()
    ref_big = cached("fb_big", lambda: O.farneback(big, big_b, levels=4, iterations=1, poly_n=7, poly_sigma=1.5,
                                                   flags=O.FARNEBACK_GAUSSIAN, box_direct=False))
    ref_small = cached(("fb", "box", 3), lambda: O.farneback(a, b, levels=3, iterations=2, flags=0, box_direct=True,
                                                             init_flow=None))
    big_kw = dict(numLevels=4, numIters=1, polyN=7, polySigma=1.5, flags=O.FARNEBACK_GAUSSIAN)
    same_bits(_gpu_flow(gpu, big, big_b, **big_kw), ref_big, "large pair, first")
    same_bits(_gpu_flow(gpu, a, b, numLevels=3, numIters=2, flags=0), ref_small, "small pair after the large one")
    same_bits(_gpu_flow(gpu, big, big_b, **big_kw), ref_big, "large pair again")


def test_history_dense_pyrlk(gpu):
    big = large_frame()[:120, :160]
    big = np.ascontiguousarray(big)
    big_b = np.ascontiguousarray(np.roll(big, (1, -2), axis=(0, 1)))
    ys, xs = np.mgrid[0:120, 0:160]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)

    def make(win):
        nx, st, _, _ = O.lk(O.Pyramid(big, win, 3), O.Pyramid(big_b, win, 3), pts, win=win, max_level=3,
                            accum=O.ACCUM_EXACT, want_err=False)
        return (nx - pts).astype(np.float32), st

    a, b = dense_pair()
    for win_big, win_small in (((13, 13), (7, 7)), ((11, 5), (9, 7))):
        ref_big = cached(("dense_big", win_big), lambda: make(win_big))
        ref_small = dense_ref(win_small)
        for what, (p, q), win, ml, ref in (("large pair, first", (big, big_b), win_big, 3, ref_big),
                                           ("small pair after the large one", (a, b), win_small, 2, ref_small),
                                           ("large pair again", (big, big_b), win_big, 3, ref_big)):
            flow, status = K().DensePyrLKOpticalFlow.create(win, ml, 30).calc(dev(p), dev(q), want_status=True)
            flow, status = host(flow).reshape(-1, 2), host(status).ravel()
            same_bits(status, ref[1], f"{what}, window {win}: status")
            same_bits(flow[ref[1] == 1], ref[0][ref[1] == 1], f"{what}, window {win}: flow of the tracked pixels")


def test_history_hog_detect_multiscale(gpu):
    big = cached("hog320", lambda: np.clip(_bgr(53, 320, 240, cn=3).astype(np.int32) * 3 // 2 + 40, 0, 255)
                 .astype(np.uint8))
    small = cached("hog200", lambda: _bgr(41, 200, 280, cn=3))
    call_big, ref_big = hog_multi(gpu, big, (48, 96))
    call_small, ref_small = hog_multi(gpu, small, (64, 128))
    assert len(ref_big) > 0 and len(ref_small) > 0
    hog_same(call_big(), ref_big, "large frame, first")
    hog_same(call_small(), ref_small, "small frame after the large one")
    hog_same(call_big(), ref_big, "large frame again")


# ---- the front end's table cache: eviction ------------------------------------------------------------------------

# ten (source, destination) sizes for 8 slots; destinations both larger than any before (the slot
# grows) and smaller (the slot is overwritten in place)
FRONT_PAIRS = [((90, 70), (31, 20)), ((90, 70), (123, 77)), ((64, 48), (40, 30)), ((50, 40), (150, 99)),
               ((97, 61), (33, 21)), ((97, 61), (200, 140)), ((33, 7), (32, 7)), ((120, 80), (61, 41)),
               ((90, 70), (250, 190)), ((40, 30), (17, 11))]


def front_inputs():
    return [(FE.pattern(s[0], s[1], 3, 900 + i), d) for i, (s, d) in enumerate(FRONT_PAIRS)]


def front_refs():
    return cached("front_refs", lambda: [FE.resize_linear(src, d) for src, d in front_inputs()])


def test_front_cache_eviction(gpu):
    ins = [(dev(src), d) for src, d in front_inputs()]
    refs = front_refs()
    for rnd in range(2):  # every lookup of the second round evicts
        for i, (t, d) in enumerate(ins):
            same_bits(K().resize_linear(t, d, ctx=gpu), refs[i], f"round {rnd} pair {i} {FRONT_PAIRS[i]}")


def test_front_cache_eviction_on_two_streams(gpu):
    """the same sequence alternating between two streams with no host synchronisation
    between the calls: an eviction waits for the slot's readers whatever their stream"""
    ins = [(dev(src), d) for src, d in front_inputs()]
    refs = front_refs()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty((d[1], d[0], 3), dtype=torch.uint8, device="cuda") for _ in range(2) for _, d in ins]
    torch.cuda.synchronize()
    k = 0
    for rnd in range(2):
        for i, (t, d) in enumerate(ins):
            s = streams[k % 2]
            with torch.cuda.stream(s):
                K().resize_linear(t, d, dst=outs[k], ctx=gpu, stream=s)
            k += 1
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        i = k % len(ins)
        same_bits(o, refs[i], f"call {k} pair {FRONT_PAIRS[i]} on stream {k % 2}")


# ---- fresh allocations --------------------------------------------------------------------------------------------------

class fresh_context:
    """a new context whose every allocation is born as `byte`; destroyed at the end"""

    def __init__(self, byte):
        self.byte = byte

    def __enter__(self):
        self.ctx = K().Context(0)
        self.ctx.set_option("alloc_fill", self.byte)
        return self.ctx

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.ctx.close()


PW, PH = 77, 124


def pyr_frames():
    def make():
        fr = O.synth(20261024, PW, PH, 4, 0, 2)[0]
        return np.ascontiguousarray(fr[0]), np.ascontiguousarray(fr[1])

    return cached("pyr_frames", make)


def border_points():
    """points on the border rows and columns, and a few inside"""
    xs = np.float32([0, 0.5, 11.25, 38, PW - 1.5, PW - 1])
    ys = np.float32([0, 0.75, 17.5, 62, PH - 1.25, PH - 1])
    g = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    edge = (g[:, 0] < 1) | (g[:, 0] > PW - 2) | (g[:, 1] < 1) | (g[:, 1] > PH - 2)
    return np.ascontiguousarray(np.concatenate([g[edge], g[~edge][:4]]).astype(np.float32))


@byte_param
def test_fresh_pyramids_u8(byte):
    k = K()
    a, b = pyr_frames()
    win, ml = (9, 9), 3
    with fresh_context(byte) as ctx:
        for derivs in (True, False):
            P = k.build_pyramid(dev(a), win, ml, ctx=ctx, derivs=derivs)
            torch.cuda.synchronize()
            R = O.Pyramid(a, win, ml, pad=P.pyr.lv[0].pad)
            assert P.nlevels == R.nlevels
            for i in range(P.nlevels):
                same_bits(P.level(i, True), R.level(i, True), f"u8 derivs {derivs} level {i} with border")
                if derivs:
                    same_bits(P.deriv(i), O.scharr(R.level(i)), f"u8 Scharr plane {i}")
        frame = dev(a)
        B = k.Pyramid(ctx, PW, PH, ml, win, derivs=False).build_borrowed(frame)
        torch.cuda.synchronize()
        Rb = O.Pyramid(a, win, ml, pad=B.pyr.lv[1].pad)
        same_bits(B.level(0), a, "borrowed level 0")
        for i in range(1, B.nlevels):
            same_bits(B.level(i, True), Rb.level(i, True), f"borrowed build level {i} with border")
        a3 = X.to_cn(a, 3)
        P3 = k.build_pyramid(dev(a3), win, ml, ctx=ctx)
        torch.cuda.synchronize()
        R3 = O.Pyramid(a3, win, ml, pad=P3.pyr.lv[0].pad)
        for i in range(P3.nlevels):
            same_bits(P3.level(i, True), R3.level(i, True), f"cn 3 level {i} with border")
            same_bits(P3.deriv(i), O.scharr(R3.level(i)), f"cn 3 Scharr plane {i}")
        del P, B, P3


@byte_param
def test_fresh_pyramids_float(byte):
    k = K()
    a, _ = pyr_frames()
    win, ml = (9, 9), 3
    with fresh_context(byte) as ctx:
        for dt, f32 in ((torch.float16, False), (torch.float32, True)):
            Pf = k.Pyramid(ctx, PW, PH, ml, win, dt).build(dev(a))
            torch.cuda.synchronize()
            _fp_pyramid_same(f"{'fp32' if f32 else 'fp16'} from u8", Pf, O.Pyramid16(a, win, ml, f32=f32))
            del Pf
        u16 = X.to_u16(a, 65535)
        Pu = k.Pyramid(ctx, PW, PH, ml, win, torch.float32).build(dev(u16))
        torch.cuda.synchronize()
        _fp_pyramid_same("fp32 from 16U", Pu, O.Pyramid16(u16, win, ml, f32=True))
        del Pu


@byte_param
def test_fresh_pyramids_sparse_pyrlk_on_the_border(byte):
    k = K()
    a, b = pyr_frames()
    pts = border_points()
    with fresh_context(byte) as ctx:
        for win, ml in (((9, 9), 3), ((21, 21), 2)):
            g, ex, _ = run_pair(ctx, a, b, pts, win, ml)
            assert_exact(g, ex)
            same_bits(g[1], ex[1], f"window {win}: status")
        g, ex, _ = run_pair_cn(ctx, X.to_cn(a, 3), X.to_cn(b, 3), pts, (9, 9), 2)
        assert_exact(g, ex)
        import _fb_oracle as FBO

        win, ml = 9, 2
        lk = k.SparsePyrLKOpticalFlow((win, win), ml, 30)
        Pa, Pb = k.build_pyramid(dev(a), (win, win), ml, ctx=ctx), k.build_pyramid(dev(b), (win, win), ml, ctx=ctx)
        g = fb_host(lk.calc_checked(Pa, Pb, dev(pts), back_threshold=1.0, want_iters=True))
        pad = Pa.pyr.lv[0].pad
        ref = FBO.checked_trace(O.Pyramid(a, (win, win), ml, pad), O.Pyramid(b, (win, win), ml, pad), pts, win, ml, 30,
                                0.01, 1e-4, 1.0, O.ACCUM_EXACT)
        same_bits(g["status"], ref.status, "calc_checked: checked status")
        same_bits(g["iters"], ref.iters, "calc_checked: iters")
        ok = ref.fwd_status == 1
        same_bits(g["next_pts"][ok], ref.next_pts[ok], "calc_checked: next_pts of the points tracked forward")
        back_equal(g, ref)
        del Pa, Pb, lk
        # the fp32 multi-channel pyramids and their PyrLK, from 16U frames
        from test_gpu_f32 import _cn_pyr

        A, B = X.to_u16(X.to_cn(a, 3), 65535), X.to_u16(X.to_cn(b, 3), 65535)
        Pa, Pb = _cn_pyr(ctx, A, (9, 9), 2), _cn_pyr(ctx, B, (9, 9), 2)
        r = k.SparsePyrLKOpticalFlow((9, 9), 2, 30).calc(Pa, Pb, dev(pts), want_iters=True)
        g = (host(r.next_pts), host(r.status), host(r.err), host(r.iters))
        Ra, Rb = O.Pyramid16(A, (9, 9), 2, f32=True), O.Pyramid16(B, (9, 9), 2, f32=True)
        for i in range(Pa.nlevels):
            same_bits(Pa.level(i), Ra.levels[i], f"fp32 cn 3 level {i}")
            same_bits(Pa.deriv(i), Ra.derivs[i], f"fp32 cn 3 derivative plane {i}")
        ex = O.lk16(Ra, Rb, pts, (9, 9), 2)
        for i, part in enumerate(("next_pts", "status", "err", "iters")):
            same_bits(g[i], ex[i], f"klt_cn_f32 cn 3: {part}")
        del Pa, Pb


@byte_param
def test_fresh_tbd_loop(byte):
    """the oracle comparison of tests/test_gpu_tbd_configs.py, default options: once through
    step and once through run (LP.run_pair does both), frames rendered by the fresh context"""
    with fresh_context(byte) as ctx:
        s = LP.run_pair(ctx, 320, 240, 6, 8, 31, 0.1, cfg={"bounds_xmax": 320, "bounds_ymax": 240})
        assert s["preds"] > 0 and s["lk_points"] > 0


@byte_param
def test_fresh_tbd_loop_fb_check_and_ransac(byte):
    """tbd_fb_check and tbd_fit_ransac on (tests/_fb_oracle.py's ransac500 case and its
    oracle): stepped with the next frame, and through run"""
    import _fb_oracle as FB
    import test_gpu_tbd_fb as TF

    c = FB.LOOP_BY_ID["ransac500"]
    ora = FB.loop_oracle(c.seed, c.opt, c.cfg, c.ransac)
    with fresh_context(byte) as ctx:
        for how in ("ahead", "run"):
            got = TF.gpu_loop(ctx, c.seed, c.opt, c.cfg, c.options, c.ransac, how=how)
            assert TF.assert_equals_oracle(got, ora, f"fresh context, {how}") > 0


from test_gpu_tbd_subpix import refined_oracle  # noqa: E402,F401  (the fixture: the refined oracle run, shared)


@byte_param
def test_fresh_tbd_loop_subpix(refined_oracle, byte):
    """tbd_subpix on (tests/test_gpu_tbd_subpix.py's sequence and refined oracle): step and run"""
    import test_gpu_tbd_subpix as TS
    from opencv_amd import tbd

    with fresh_context(byte) as ctx:
        frames, dets, _ = LP.gpu_inputs(ctx, TS.W, TS.H, TS.N, TS.F, TS.SEED, TS.DROP)
        ctx.set_option("tbd_subpix", TS.WIN)
        loop = tbd.TbdLoop(tbd.default_config(TS.W, TS.H, **TS.CFG), ctx=ctx)
        for f in range(TS.F):
            m = loop.step(frames[f], f, dets[f], next_frame=frames[f + 1] if f + 1 < TS.F else None)
            TS.check_frame(loop, m, refined_oracle, f)
        batch = tbd.TbdLoop(tbd.default_config(TS.W, TS.H, **TS.CFG), ctx=ctx)
        ms = batch.run([frames[f] for f in range(TS.F)], 0, dets)
        assert [LP.gpu_metrics(m) for m in ms] == list(refined_oracle.metrics)
        assert LP.gpu_rows(batch.tracks()) == list(refined_oracle.rows[TS.F - 1])
        torch.cuda.synchronize()
        del loop, batch


@byte_param
def test_fresh_klt_tracker(byte):
    case = KO.CASES["small"]  # detect interval 2: tops up at frames 2 and 4
    fr = KO.frames(case.seq)
    ref = KO.run_case(case)
    with fresh_context(byte) as ctx:
        t = K().KltTracker(ctx=ctx, width=fr.shape[2], height=fr.shape[1], **case.cfg)
        d = dev(fr[:6])
        for f in range(6):
            t.step(d[f])
            assert_state(t, ref.states[f], ref.stats[f], f"frame {f}")
        torch.cuda.synchronize()
        del t


@byte_param
@pytest.mark.parametrize("i", [0, 19])
def test_fresh_mog2(i, byte):
    n = 12
    case = dict(GC.cases()[i])
    case.update(n=n, rates=case["rates"][:n], bg=(n,))
    frames = GC.case_frames(GC.cases()[i])[:n]

    def make():
        masks, bgs, m = M2.run_case(case, GC.params(case), frames)
        return masks, bgs, m.model()

    wm, wb, wmodel = cached(("mog2", i), make)
    with fresh_context(byte) as ctx:
        m = subtractor(case["params"], ctx)
        masks, bgs = mog2_run(m, frames, case["rates"], case["bg"])
        same_bits(masks, wm, f"{case['name']}: masks")
        same_bits(bgs[n], wb[n], f"{case['name']}: background after frame {n}")
        assert_model(model_of(m), wmodel, case["name"])
        del m


@byte_param
def test_fresh_step_image(gpu, byte):
    """the attached detector on three 320x240 BGR frames: a fresh context against the session's"""
    import test_gpu_tbd_detect as TD

    frames = TD.bgr_frames((320, 240))[:3]

    def run(ctx):
        loop = TD.gpu_loop(ctx, -1.0)
        loop.attach_detector(TD.gpu_hog(ctx), src_size=(320, 240), make_gray=True, confidence_mode=1)
        out = []
        for f, bgr in enumerate(frames):
            m, dets = loop.step_image(dev(bgr), f)
            out.append((TD.metrics_of(m), np.array(dets).tobytes(), TD.gpu_rows(loop.tracks())))
        torch.cuda.synchronize()
        del loop
        return out

    want = run(gpu)
    assert sum(len(w[2]) for w in want) > 0
    with fresh_context(byte) as ctx:
        got = run(ctx)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], f"frame {f}: metrics {g[0]} vs {w[0]}"
        assert g[1] == w[1], f"frame {f}: detections differ"
        assert g[2] == w[2], f"frame {f}: tracks differ"
