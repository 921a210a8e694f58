"""GPU BackgroundSubtractorKNN (opencv_amd/bgsegm.py, tbdk_knn_*) against the numpy restatement
(tests/_knn_oracle.py) and the real reference's recordings (tests/golden/reference_knn.npz): every mask, every
background image, and the model, counters and RNG state after the last frame, bit for bit; there is no
tolerance in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

import _knn_cases as KC
import _knn_oracle as KO
import _reference_cases as RC
import _views as V

pytestmark = pytest.mark.gpu

SETTERS = dict(history="setHistory", nsamples="setNSamples", knn_samples="setkNNSamples",
               detect_shadows="setDetectShadows", shadow_value="setShadowValue",
               dist2_threshold="setDist2Threshold", shadow_threshold="setShadowThreshold")


def subtractor(params, ctx=None):
    from opencv_amd import bgsegm

    p = dict(KC.DEFAULTS, **params)
    m = bgsegm.createBackgroundSubtractorKNN(p["history"], p["dist2_threshold"], bool(p["detect_shadows"]), ctx=ctx,
                                             rngState=p["rng_state"])
    for k, name in SETTERS.items():
        getattr(m, name)(p[k])
    return m


def run(m, frames, rates=None, bg=(), stream=None):
    masks, bgs = [], {}
    for t, f in enumerate(frames):
        img = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)).cuda()
        masks.append(m.apply(img, learningRate=-1 if rates is None else float(rates[t]), stream=stream))
        if t + 1 in bg:
            bgs[t + 1] = m.getBackgroundImage(stream=stream)
    torch.cuda.synchronize()
    return np.stack([x.cpu().numpy() for x in masks]), {t: b.cpu().numpy() for t, b in bgs.items()}


def model_of(m, stream=None):
    """(samples, index, next, counters, rng state as a Python int)"""
    out = m.model(stream=stream)
    torch.cuda.synchronize()
    s, i, n, c, r = (x.cpu().numpy() for x in out)
    return s, i, n, c, int(r.view(np.uint64)[0])


def assert_model(got, want, what):
    for name, g, w in zip(("samples", "index", "next", "counters"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, name)
    assert got[4] == want[4], (what, "rng state", hex(got[4]), hex(want[4]))


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("knn")


@pytest.mark.parametrize("i", range(KC.NCASES))
def test_recorded_cases(gpu, fx, i):
    case = KC.cases()[i]
    m = subtractor(case["params"], gpu)
    masks, bgs = run(m, KC.case_frames(case), case["rates"], case["bg"])
    wm, wb, wmodel = KO.expected(i)[:3]
    bad = [t for t in range(case["n"]) if not np.array_equal(masks[t], wm[t])]
    assert not bad, (case["name"], "frames whose mask differs from the restatement", bad[:8])
    assert np.array_equal(KC.stored_masks(case, masks), fx[f"{i}_masks"]), case["name"]
    for t in case["bg"]:
        assert bgs[t].shape == wb[t].shape and np.array_equal(bgs[t], wb[t]), (case["name"], "background", t)
        assert np.array_equal(KC.stored_background(case, bgs[t]), fx[f"{i}_bg{t}"]), (case["name"], "background", t)
    got = model_of(m)
    assert_model(got, wmodel, case["name"])
    assert got[4] == KC.join_state(fx[f"{i}_state"]), (case["name"], "the recorded RNG state")
    nframes = 0
    for r in case["rates"]:
        nframes = 1 if nframes == 0 or r >= 1 else nframes + 1
    assert m.frames() == nframes


VIEW_CASES = [0, 2]  # 8UC1 and 8UC3 on the base sequence
VIEW_FRAMES = 16


@pytest.mark.parametrize("layout", sorted(V.LAYOUTS))
@pytest.mark.parametrize("i", VIEW_CASES)
def test_pitched_unaligned_views(gpu, i, layout):
    case = KC.cases()[i]
    frames = KC.case_frames(case)
    wm, wb = KO.expected(i)[:2]
    m = subtractor(case["params"], gpu)
    h, w = case["h"], case["w"]
    mparent, mview = V.window(np.full((h, w), 77, np.uint8), layout, 5, "cuda")
    bparent, bview = V.window(np.zeros_like(frames[0]), layout, 6, "cuda")
    mbefore, bbefore = V.snapshot(mparent), V.snapshot(bparent)
    for t in range(VIEW_FRAMES):
        fparent, fview = V.window(frames[t], layout, 100 + t, "cuda")
        fbefore = V.snapshot(fparent)
        out = m.apply(fview, mview, float(case["rates"][t]))
        assert out.data_ptr() == mview.data_ptr()
        assert np.array_equal(V.host(mview), wm[t]), (case["name"], layout, "mask", t)
        assert torch.equal(fparent, fbefore), "the frame's allocation was written"
        if t + 1 in case["bg"]:
            m.getBackgroundImage(bview)
            assert np.array_equal(V.host(bview), wb[t + 1]), (case["name"], layout, "background", t + 1)
    assert V.guards_intact(mparent, mbefore, mview), "bytes outside the mask view were written"
    assert V.guards_intact(bparent, bbefore, bview), "bytes outside the background view were written"


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("width", [1, 3, 63, 64, 65, 67, 130])
def test_row_tails(gpu, width, cn):
    # the tails of the four-pixel groups and of the 256-lane workgroups; 130 x 9 is a block and a tail of the fill
    frames = KC.GC.frames(width, 9, 6, cn)
    params = dict(history=4, rng_state=12345)
    ref = KO.KNN(**dict(KC.DEFAULTS, **params))
    m = subtractor(params, gpu)
    masks, bgs = run(m, frames, bg=(6,))
    for t in range(6):
        assert np.array_equal(masks[t], ref.apply(frames[t])), (width, cn, t)
    assert np.array_equal(bgs[6], ref.background_image())
    assert_model(model_of(m), ref.model(), (width, cn))


def test_a_frame_over_all_xcds(gpu):
    # 1242 x 375: 455 blocks of the fill, 456 with the tail
    frames = KC.GC.frames(1242, 375, 3, 3)
    ref = KO.KNN()
    m = subtractor({}, gpu)
    masks, bgs = run(m, frames, bg=(3,))
    for t in range(3):
        assert np.array_equal(masks[t], ref.apply(frames[t])), t
    assert np.array_equal(bgs[3], ref.background_image())
    assert_model(model_of(m), ref.model(), "1242x375")


def test_reset_mid_sequence(gpu):
    """reset() empties the model and the counters and leaves the RNG where it is: the run equals the restatement
    treated the same way, and differs from a fresh object's, whose RNG starts over"""
    case = KC.cases()[2]
    frames = KC.case_frames(case)
    m, ref = subtractor(case["params"], gpu), KO.KNN(**KC.params(case))
    first, _ = run(m, frames[:20])
    assert m.frames() == 20
    m.reset()
    assert m.frames() == 0
    again, _ = run(m, frames[20:40])
    want = [ref.apply(f) for f in frames[:20]]
    ref.reset()
    want += [ref.apply(f) for f in frames[20:40]]
    assert np.array_equal(np.concatenate([first, again]), np.stack(want))
    assert_model(model_of(m), ref.model(), "after reset")
    fresh = subtractor(case["params"], gpu)
    run(fresh, frames[20:40])
    assert model_of(fresh)[4] != ref.model()[4]


def test_set_params_mid_sequence(gpu):
    case = KC.cases()[2]
    frames = KC.case_frames(case)
    m, ref = subtractor(case["params"], gpu), KO.KNN(**KC.params(case))
    a, _ = run(m, frames[:16])
    m.setDist2Threshold(100.0)
    m.setkNNSamples(3)
    m.setShadowValue(90)
    m.setShadowThreshold(0.7)
    m.setHistory(20)
    b, _ = run(m, frames[16:32])
    m.setDetectShadows(False)
    c, _ = run(m, frames[32:])
    want = [ref.apply(f) for f in frames[:16]]
    ref.Tb, ref.nkNN, ref.shadow_value, ref.tau, ref.history = np.float32(100.0), 3, 90, np.float32(0.7), 20
    want += [ref.apply(f) for f in frames[16:32]]
    ref.detect_shadows = False
    want += [ref.apply(f) for f in frames[32:]]
    got = np.concatenate([a, b, c])
    bad = [t for t in range(len(frames)) if not np.array_equal(got[t], want[t])]
    assert not bad, bad[:8]
    assert (b == 90).any() and not np.isin(c, (90, 127)).any()
    assert_model(model_of(m), ref.model(), "after the setters")


def test_two_subtractors_with_different_seeds_interleaved_on_one_stream(gpu):
    ia, ib = 2, 16  # the same frames and parameters, two seeds
    ca, cb = KC.cases()[ia], KC.cases()[ib]
    assert KC.params(ca)["rng_state"] != KC.params(cb)["rng_state"]
    fr = [torch.from_numpy(f).cuda() for f in KC.case_frames(ca)]
    ma, mb = subtractor(ca["params"], gpu), subtractor(cb["params"], gpu)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ga, gb = [], []
    for t in range(KC.NFRAMES):
        ga.append(ma.apply(fr[t], stream=s))
        gb.append(mb.apply(fr[t], stream=s))
    torch.cuda.synchronize()
    assert np.array_equal(np.stack([x.cpu().numpy() for x in ga]), KO.expected(ia)[0])
    assert np.array_equal(np.stack([x.cpu().numpy() for x in gb]), KO.expected(ib)[0])
    assert_model(model_of(ma), KO.expected(ia)[2], "seed a")
    assert_model(model_of(mb), KO.expected(ib)[2], "seed b")
    assert not np.array_equal(KO.expected(ia)[2][2], KO.expected(ib)[2][2])


def test_the_schedule(gpu):
    case = KC.cases()[1]  # 8UC1, history 12
    frames = KC.case_frames(case)[:30]
    want = KO.expected(1)[0][:30]
    # the automatic rate of frame n is 1 / min(2 n, history): given explicitly from frame 2 on it changes nothing
    rates = np.array([1.0 / min(2 * n, 12) for n in range(1, 31)])
    explicit, _ = run(subtractor(case["params"], gpu), frames, np.concatenate([[-1.0], rates[1:]]))
    assert np.array_equal(explicit, want)
    # a rate of exactly 1 initialises the model (the RNG goes on), with the periods 1, 1, 1
    m, ref = subtractor(case["params"], gpu), KO.KNN(**KC.params(case))
    rr = np.full(30, -1.0)
    rr[20] = 1.0
    re, _ = run(m, frames, rr)
    assert np.array_equal(re, np.stack([ref.apply(f, r) for f, r in zip(frames, rr)]))
    assert ref.periods[20] == (1, 1, 1) and m.frames() == 10
    assert_model(model_of(m), ref.model(), "rate 1")


def test_error_paths(gpu):
    from opencv_amd import _lib

    lib = gpu.lib
    cfg = _lib.KnnConfig()
    for cn, k in ((4, 7), (2, 7), (1, 0), (3, 17)):
        assert lib.tbdk_knn_config_default(64, 48, cn, C.byref(cfg)) == _lib.TBDK_OK
        cfg.nsamples = k
        h = C.c_void_p()
        assert lib.tbdk_knn_create(gpu.handle, C.byref(cfg), C.byref(h)) == _lib.TBDK_EINVAL and not h.value
    frame = torch.from_numpy(KC.GC.frames(n=1)[0]).cuda()
    with pytest.raises(_lib.TbdkError):
        subtractor({}, gpu).apply(frame.to(torch.float32))
    with pytest.raises(_lib.TbdkError):
        subtractor({}, gpu).apply(torch.zeros((48, 64, 4), dtype=torch.uint8, device="cuda"))
    m = subtractor(dict(history=12), gpu)
    mask = m.apply(frame).clone()
    m.apply(frame)
    torch.cuda.synchronize()
    before = model_of(m)
    # another size, a mask of another size, the undefined rates, set_params with another size: nothing runs
    with pytest.raises(_lib.TbdkError):
        m.apply(frame[:, :60])
    with pytest.raises(_lib.TbdkError):
        m.apply(frame, torch.zeros((48, 60), dtype=torch.uint8, device="cuda"))
    for rate in (float("nan"), 0.0, 1.5, float("inf"), 1e-12):
        with pytest.raises(_lib.TbdkError):
            m.apply(frame, learningRate=rate)
    with pytest.raises(_lib.TbdkError):
        m.setNSamples(3)
    with pytest.raises(_lib.TbdkError):
        m.setHistory(0)
    assert m.getHistory() == 12
    other = _lib.KnnConfig.from_buffer_copy(m.cfg)
    other.width = 60
    assert lib.tbdk_knn_set_params(m.handle, C.byref(other)) == _lib.TBDK_EINVAL
    assert lib.tbdk_knn_apply(m.handle, None, 64, C.c_void_p(mask.data_ptr()), 64, -1.0, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_knn_apply(m.handle, C.c_void_p(frame.data_ptr()), 63, C.c_void_p(mask.data_ptr()), 64, -1.0,
                              None) == _lib.TBDK_EINVAL
    assert lib.tbdk_knn_get_background(m.handle, C.c_void_p(mask.data_ptr()), 63, None) == _lib.TBDK_EINVAL
    assert m.frames() == 2
    assert_model(model_of(m), before, "after the refused calls")
    # a rate that is small but defined goes through
    m.apply(frame, learningRate=1e-6)
    assert m.frames() == 3
