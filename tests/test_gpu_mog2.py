"""GPU BackgroundSubtractorMOG2 (opencv_amd/bgsegm.py, tbdk_mog2_*) against the numpy restatement
(tests/_mog2_oracle.py) and the real reference's recordings (tests/golden/reference_mog2.npz): every mask, every
background image and the model after the last frame, bit for bit; there is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gftt_mask_oracle as GM
import _mog2_cases as GC
import _mog2_oracle as MO
import _reference_cases as RC
import _views as V

pytestmark = pytest.mark.gpu

SETTERS = dict(history="setHistory", nmixtures="setNMixtures", detect_shadows="setDetectShadows",
               shadow_value="setShadowValue", var_threshold="setVarThreshold", var_threshold_gen="setVarThresholdGen",
               var_init="setVarInit", var_min="setVarMin", var_max="setVarMax", background_ratio="setBackgroundRatio",
               complexity_reduction="setComplexityReductionThreshold", shadow_threshold="setShadowThreshold")


def subtractor(params, ctx=None):
    from opencv_amd import bgsegm

    p = dict(GC.DEFAULTS, **params)
    m = bgsegm.BackgroundSubtractorMOG2.create(p["history"], p["var_threshold"], bool(p["detect_shadows"]), ctx=ctx)
    for k, name in SETTERS.items():
        getattr(m, name)(p[k])
    return m


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def run(m, frames, rates=None, bg=(), stream=None):
    masks, bgs = [], {}
    for t, f in enumerate(frames):
        img = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)).cuda()
        masks.append(m.apply(img, learningRate=-1 if rates is None else float(rates[t]), stream=stream))
        if t + 1 in bg:
            bgs[t + 1] = m.getBackgroundImage(stream=stream)
    torch.cuda.synchronize()
    return np.stack([x.cpu().numpy() for x in masks]), {t: b.cpu().numpy() for t, b in bgs.items()}


def model_of(m):
    out = tuple(x.cpu().numpy() for x in m.model())
    torch.cuda.synchronize()
    return out


def assert_model(got, want, what):
    for name, g, w in zip(("weight", "variance", "mean", "modes_used"), got, want):
        assert same(g, w), (what, name)


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("mog2")


@pytest.mark.parametrize("i", range(GC.NCASES))
def test_recorded_cases(gpu, fx, i):
    case = GC.cases()[i]
    m = subtractor(case["params"], gpu)
    masks, bgs = run(m, GC.case_frames(case), case["rates"], case["bg"])
    wm, wb, wmodel, _ = MO.expected(i)
    bad = [t for t in range(case["n"]) if not np.array_equal(masks[t], wm[t])]
    assert not bad, (case["name"], "frames whose mask differs from the restatement", bad[:8])
    assert np.array_equal(GC.stored_masks(case, masks), fx[f"{i}_masks"]), case["name"]
    for t in case["bg"]:
        assert same(bgs[t], wb[t]), (case["name"], "background", t)
        assert np.array_equal(GC.stored_background(bgs[t]), fx[f"{i}_bg{t}"]), (case["name"], "background", t)
    assert_model(model_of(m), wmodel, case["name"])
    nframes = 0
    for r in case["rates"]:
        nframes = 1 if nframes == 0 or r >= 1 else nframes + 1
    assert m.frames() == nframes


VIEW_CASES = [0, 2, 17, 19]  # 8UC1, 8UC3, 32FC1, 32FC3 on the base sequence


@pytest.mark.parametrize("layout", sorted(V.LAYOUTS))
@pytest.mark.parametrize("i", VIEW_CASES)
def test_pitched_unaligned_views(gpu, i, layout):
    case = GC.cases()[i]
    frames = GC.case_frames(case)
    wm, wb, wmodel, _ = MO.expected(i)
    m = subtractor(case["params"], gpu)
    h, w = case["h"], case["w"]
    mparent, mview = V.window(np.full((h, w), 77, np.uint8), layout, 5, "cuda")
    bparent, bview = V.window(np.zeros_like(frames[0]), layout, 6, "cuda")
    mbefore, bbefore = V.snapshot(mparent), V.snapshot(bparent)
    for t in range(case["n"]):
        fparent, fview = V.window(frames[t], layout, 100 + t, "cuda")
        fbefore = V.snapshot(fparent)
        out = m.apply(fview, mview, float(case["rates"][t]))
        assert out.data_ptr() == mview.data_ptr()
        assert np.array_equal(V.host(mview), wm[t]), (case["name"], layout, "mask", t)
        assert torch.equal(fparent, fbefore), "the frame's allocation was written"
        if t + 1 in case["bg"]:
            m.getBackgroundImage(bview)
            assert same(V.host(bview), wb[t + 1]), (case["name"], layout, "background", t + 1)
    assert V.guards_intact(mparent, mbefore, mview), "bytes outside the mask view were written"
    assert V.guards_intact(bparent, bbefore, bview), "bytes outside the background view were written"
    assert_model(model_of(m), wmodel, (case["name"], layout))


@pytest.mark.parametrize("content,cn", [("u8", 1), ("u8", 3), ("frac", 1), ("frac", 3)])
@pytest.mark.parametrize("width", [1, 3, 63, 64, 65, 67, 130])
def test_row_tails(gpu, width, content, cn):
    # the tails of the four-pixel groups and of the 256-lane workgroups
    frames = GC.frames(width, 5, 6, cn, content)
    params = dict(history=4)
    ref = MO.MOG2(**dict(GC.DEFAULTS, **params))
    m = subtractor(params, gpu)
    masks, bgs = run(m, frames, bg=(6,))
    for t in range(6):
        assert np.array_equal(masks[t], ref.apply(frames[t])), (width, content, cn, t)
    assert same(bgs[6], ref.background_image())
    assert_model(model_of(m), ref.model(), (width, content, cn))


def test_a_frame_over_all_xcds(gpu):
    frames = GC.frames(1242, 375, 3, 3)
    ref = MO.MOG2()
    m = subtractor({}, gpu)
    masks, bgs = run(m, frames, bg=(3,))
    for t in range(3):
        assert np.array_equal(masks[t], ref.apply(frames[t])), t
    assert same(bgs[3], ref.background_image())
    assert_model(model_of(m), ref.model(), "1242x375")


def test_two_subtractors_interleaved_on_two_streams(gpu):
    ia, ib = 0, 2
    ca, cb = GC.cases()[ia], GC.cases()[ib]
    fa = [torch.from_numpy(f).cuda() for f in GC.case_frames(ca)]
    fb = [torch.from_numpy(f).cuda() for f in GC.case_frames(cb)]
    ma, mb = subtractor(ca["params"], gpu), subtractor(cb["params"], gpu)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ga, gb = [], []
    for t in range(GC.NFRAMES):
        ga.append(ma.apply(fa[t], stream=sa))
        gb.append(mb.apply(fb[t], stream=sb))
    torch.cuda.synchronize()
    assert np.array_equal(np.stack([x.cpu().numpy() for x in ga]), MO.expected(ia)[0])
    assert np.array_equal(np.stack([x.cpu().numpy() for x in gb]), MO.expected(ib)[0])
    assert_model(model_of(ma), MO.expected(ia)[2], "stream a")
    assert_model(model_of(mb), MO.expected(ib)[2], "stream b")


def test_reset_gives_the_first_run_again(gpu):
    case = GC.cases()[0]
    frames = GC.case_frames(case)
    m = subtractor(case["params"], gpu)
    first, _ = run(m, frames[:20])
    assert m.frames() == 20
    m.reset()
    assert m.frames() == 0
    again, _ = run(m, frames[:20])
    assert np.array_equal(first, again) and np.array_equal(first, MO.expected(0)[0][:20])


def test_the_schedule(gpu):
    case = GC.cases()[0]  # history 12
    frames = GC.case_frames(case)[:30]
    want = MO.expected(0)[0][:30]
    auto, _ = run(subtractor(case["params"], gpu), frames)
    assert np.array_equal(auto, want)
    # the automatic rate of frame n is 1 / min(2 n, history): given explicitly from frame 2 on it changes nothing
    rates = np.array([1.0 / min(2 * n, 12) for n in range(1, 31)])
    explicit, _ = run(subtractor(case["params"], gpu), frames, np.concatenate([[-1.0], rates[1:]]))
    assert np.array_equal(explicit, want)
    # ... and a run that lacks it (1 / history from frame 2 on) gives other masks while the schedule is still rising
    flat, _ = run(subtractor(case["params"], gpu), frames, np.concatenate([[-1.0], np.full(29, 1.0 / 12)]))
    differ = [t for t in range(30) if not np.array_equal(flat[t], want[t])]
    assert differ and differ[0] < 6, differ
    # the first frame ignores the given rate
    first, _ = run(subtractor(case["params"], gpu), frames[:3], np.array([0.25, -1.0, -1.0]))
    assert np.array_equal(first, want[:3])
    # learning_rate >= 1 re-initialises: from there on the masks are a fresh subtractor's
    m = subtractor(case["params"], gpu)
    rr = np.full(30, -1.0)
    rr[20] = 1.0
    re, _ = run(m, frames, rr)
    fresh, _ = run(subtractor(case["params"], gpu), frames[20:])
    assert np.array_equal(re[:20], want[:20]) and np.array_equal(re[20:], fresh)
    assert not np.array_equal(re[20:], want[20:])
    assert m.frames() == 10


def test_error_paths(gpu):
    from opencv_amd import _lib, bgsegm

    lib = gpu.lib
    cfg = _lib.Mog2Config()
    for depth, cn, k in ((2, 1, 5), (bgsegm.DEPTH_8U, 4, 5), (bgsegm.DEPTH_8U, 2, 5), (bgsegm.DEPTH_8U, 1, 0),
                         (bgsegm.DEPTH_32F, 3, 9)):
        assert lib.tbdk_mog2_config_default(64, 48, depth, cn, C.byref(cfg)) == _lib.TBDK_OK
        cfg.nmixtures = k
        h = C.c_void_p()
        assert lib.tbdk_mog2_create(gpu.handle, C.byref(cfg), C.byref(h)) == _lib.TBDK_EINVAL and not h.value
    frame = torch.from_numpy(GC.frames(n=1)[0]).cuda()
    with pytest.raises(_lib.TbdkError):
        subtractor({}, gpu).apply(frame.to(torch.int16))
    with pytest.raises(_lib.TbdkError):
        subtractor({}, gpu).apply(torch.zeros((48, 64, 4), dtype=torch.uint8, device="cuda"))
    for k in (0, 9):
        with pytest.raises(_lib.TbdkError):
            subtractor(dict(nmixtures=k), gpu).apply(frame)
    m = subtractor(dict(history=12), gpu)
    mask = m.apply(frame).clone()
    torch.cuda.synchronize()
    before = model_of(m)
    # another size, another type, a mask of another size, a NaN rate, set_params with another size: nothing runs
    with pytest.raises(_lib.TbdkError):
        m.apply(frame[:, :60])
    with pytest.raises(_lib.TbdkError):
        m.apply(frame.to(torch.float32))
    with pytest.raises(_lib.TbdkError):
        m.apply(frame, torch.zeros((48, 60), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.TbdkError):
        m.apply(frame, learningRate=float("nan"))
    with pytest.raises(_lib.TbdkError):
        m.setNMixtures(3)
    with pytest.raises(_lib.TbdkError):
        m.setHistory(0)
    assert m.getHistory() == 12
    other = _lib.Mog2Config.from_buffer_copy(m.cfg)
    other.width = 60
    assert lib.tbdk_mog2_set_params(m.handle, C.byref(other)) == _lib.TBDK_EINVAL
    assert lib.tbdk_mog2_apply(m.handle, None, 64, C.c_void_p(mask.data_ptr()), 64, -1.0, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_mog2_apply(m.handle, C.c_void_p(frame.data_ptr()), 63, C.c_void_p(mask.data_ptr()), 64, -1.0,
                               None) == _lib.TBDK_EINVAL
    assert m.frames() == 1
    assert_model(model_of(m), before, "after the refused calls")
    assert not m.apply(frame).any()  # the same frame again: all background
    assert m.frames() == 2


def test_the_mask_feeds_the_corner_detector(gpu):
    """frame 40 of the base sequence with shadow value 0: the mask, where it lies, as detect_rois' mask.  That
    mask holds 12 foreground pixels (the rectangle's edge) and no corner; frames 30 (the brightness step: 1505
    pixels, 64 corners) and 32 (51 pixels, 5 corners) are checked on the way so that corner lists are compared
    too"""
    from opencv_amd import klt

    frames = GC.frames()
    m = subtractor(dict(history=12, shadow_value=0), gpu)
    rois = [(0, 0, GC.W, GC.H)]
    det = klt.GoodFeaturesToTrackDetector(64, 0.01, 2.0)
    corners = {}
    for t in range(41):
        img = torch.from_numpy(frames[t]).cuda()
        mask = m.apply(img)
        if t in (30, 32, 40):
            c, n = det.detect_rois(img, rois, mask=mask)
            torch.cuda.synchronize()
            mh = mask.cpu().numpy()
            assert np.isin(mh, (0, 255)).all() and (mh == 255).any() and (mh == 0).any()
            ref = GM.gftt_rois_masked(frames[t], mh, rois, 64, 0.01, 2.0)
            n0 = int(n.cpu().numpy()[0])
            assert n0 == len(ref[0]), t
            assert np.array_equal(c.cpu().numpy()[0, :n0], ref[0]), t
            corners[t] = n0
    assert corners[30] > 0 and corners[32] > 0
