"""The HIP kernels against what the real reference returned
(tests/golden/reference_<op>.npz, recorded by tools/record_reference_cases.py),
directly: nothing here calls the CPU oracle's functions (tests/test_reference_pins.py
pins those to the same fixtures; O.synth only renders input frames).

Bit-exact: pyramid levels and Scharr planes (1 to 4 channels), warpAffine, the
GFTT corner lists of isolated ROIs, the cornerMinEigenVal / cornerHarris maps,
the Gaussian Farneback variant, HOG gradients, window scores and grouped rects.
PyrLK sums its windows in exact order where the reference sums in SSE2 lanes, so
it meets test_gpu_klt.assert_tolerance's default bars (0.995, 1e-2 px) with the
recording in the place of the SSE2-order oracle run.  The box Farneback variant
meets the three bars of test_box_variant_vs_reference_running_sums.

The fixtures hold, per operation, the reference's dispatch state named in
README.md's numerics paragraph."""
import os

import numpy as np
import pytest
import torch

import _reference_cases as RC
from test_gpu_klt import assert_tolerance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def fx():
    return {op: RC.fixture(op) for op in ("pyramid", "pyrlk", "warpaffine", "gftt", "cornermaps", "farneback",
                                          "farneback_box", "hog")}


@pytest.mark.parametrize("i", range(len(RC.PYR_CASES)))
def test_pyramid_and_scharr(gpu, fx, i):
    from opencv_amd import klt

    f = fx["pyramid"]
    w, h, cn, win, maxl, seed = RC.PYR_CASES[i]
    P = klt.build_pyramid(dev(RC.noise(w, h, cn, seed)), win, maxl, ctx=gpu)
    torch.cuda.synchronize()
    assert P.nlevels == int(f["meta"][i][7]) and P.channels == cn
    for lv in range(P.nlevels):
        RC.assert_pinned(RC.rows(P.level(lv)), f[f"{i}_L{lv}"], f"level {lv}")
        RC.assert_pinned(RC.rows(P.deriv(lv)), f[f"{i}_D{lv}"], f"derivatives {lv}")


@pytest.mark.parametrize("pair", RC.LK_PAIRS)
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_pyrlk_within_tolerance_of_the_reference(gpu, fx, pair, cn):
    from opencv_amd import klt

    f = fx["pyrlk"]
    a, b = RC.lk_pair(pair, cn)
    A, B, pts = dev(a), dev(b), dev(f[f"pts_{pair}"])
    ran = 0
    for i, (p, c, win, lev, flags, want_err) in enumerate(RC.lk_cases()):
        if (p, c) != (pair, cn):
            continue
        lk = klt.SparsePyrLKOpticalFlow(win, lev, 30, bool(flags & RC.OPTFLOW_USE_INITIAL_FLOW), epsilon=0.01,
                                        getMinEigenVals=bool(flags & RC.OPTFLOW_LK_GET_MIN_EIGENVALS))
        Pa, Pb = klt.build_pyramid(A, win, lev, ctx=gpu), klt.build_pyramid(B, win, lev, ctx=gpu)
        init = dev(f[f"init_{pair}"]) if flags & RC.OPTFLOW_USE_INITIAL_FLOW else None
        r = lk.calc(Pa, Pb, pts, init, want_err=bool(want_err))
        torch.cuda.synchronize()
        assert (r.err is None) == (not want_err)
        try:
            assert_tolerance((r.next_pts.cpu().numpy(), r.status.cpu().numpy()), (f[f"{i}_q"], f[f"{i}_st"]))
        except AssertionError as e:
            raise AssertionError(f"case {i}: win {win} levels {lev} flags {flags} err {want_err}: {e}") from e
        ran += 1
    assert ran >= 8


def test_warp_affine(gpu, fx):
    from opencv_amd import klt

    f = fx["warpaffine"]
    for i, (flags, border, bval, sw, sh, dw, dh) in enumerate(f["meta"].tolist()):
        src, dst = RC.warp_inputs(i, sw, sh, dw, dh)
        out = klt.warp_affine(dev(src), f["M"][i], (dw, dh), flags, border, bval, dst=dev(dst), ctx=gpu)
        torch.cuda.synchronize()
        RC.assert_pinned(out.cpu().numpy(), f[f"{i}_w"], (i, flags, border))


def test_gftt_roi_corner_lists(gpu, fx):
    """ROIs of the frames, as the loop passes them; each is detected as an isolated image"""
    from opencv_amd import klt

    f = fx["gftt"]
    cases = RC.gftt_cases()
    frames = {name: dev(RC.gftt_frame(name)) for name in {r[0] for r in RC.GFTT_ROIS}}
    for params in sorted({c[1:] for c in cases}):
        maxc, ql, md, block, harris = params
        det = klt.GoodFeaturesToTrackDetector(maxc, ql, md, block, bool(harris), RC.HARRIS_K)
        for name, frame in frames.items():
            idx = [r for r, roi in enumerate(RC.GFTT_ROIS) if roi[0] == name]
            c, n = det.detect_rois(frame, [RC.GFTT_ROIS[r][1:] for r in idx])
            torch.cuda.synchronize()
            c, n = c.cpu().numpy(), n.cpu().numpy()
            for k, r in enumerate(idx):
                x, y = RC.GFTT_ROIS[r][1:3]
                want = f[f"{cases.index((r,) + params)}_c"].astype(np.float32).reshape(-1, 2) + np.float32([x, y])
                assert n[k] == len(want), (params, r, int(n[k]), len(want))
                assert np.array_equal(c[k, :n[k]], want), (params, r)


@pytest.mark.parametrize("i", range(len(RC.CMAP_SHAPES) * len(RC.CMAP_MODES)))
def test_corner_maps(gpu, fx, i):
    from opencv_amd import klt

    f = fx["cornermaps"]
    w, h, seed = RC.CMAP_SHAPES[i // len(RC.CMAP_MODES)]
    block, harris = RC.CMAP_MODES[i % len(RC.CMAP_MODES)]
    img = dev(RC.noise(w, h, 1, seed))
    got = klt.corner_response(img, block, bool(harris), RC.HARRIS_K, ctx=gpu).cpu().numpy()
    RC.assert_pinned(got, f[f"{i}_e"], (w, h, block, harris))
    if block == 3 and not harris:  # the GFTT eigenvalue kernel
        RC.assert_pinned(klt.corner_min_eigen_val(img, ctx=gpu).cpu().numpy(), f[f"{i}_e"], (w, h, "min_eig"))


def gpu_flow(gpu, case):
    from opencv_amd import farneback as F

    w, h, ps, pn, ws, flags, use_init = case
    a, b = RC.fb_pair(w, h)
    fb = F.FarnebackOpticalFlow.create(ctx=gpu, numLevels=RC.FB_LEVELS, pyrScale=ps, winSize=ws, numIters=RC.FB_ITERS,
                                       polyN=pn, polySigma=RC.fb_sigma(pn),
                                       flags=flags | (F.OPTFLOW_USE_INITIAL_FLOW if use_init else 0))
    out = fb.calc(dev(a), dev(b), dev(RC.fb_init(w, h)) if use_init else None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("i", range(len(RC.FB_CASES)))
def test_farneback_gaussian(gpu, fx, i):
    w, h = RC.FB_CASES[i][:2]
    RC.assert_pinned(gpu_flow(gpu, RC.FB_CASES[i]).reshape(h, w * 2), fx["farneback"][f"{i}_f"], RC.FB_CASES[i])


def test_farneback_box_vs_reference_running_sums(gpu, fx):
    """the bars of test_gpu_farneback.test_box_variant_vs_reference_running_sums:
    1 - CCORR_NORMED < 1e-5, >= 99 % of pixels within 1e-2 px, max 0.5 px; on
    both sizes and all three parameter rows"""
    f = fx["farneback_box"]
    ran = 0
    for i, case in enumerate(RC.FB_BOX_CASES):
        w, h = case[:2]
        ref = f[f"{i}_f"].reshape(h, w, 2)
        got = gpu_flow(gpu, case)
        d = np.abs(got - ref).max(axis=2)
        a, b = ref.astype(np.float64).ravel(), got.astype(np.float64).ravel()
        sim = abs(float(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b)) - 1.0)
        print(f"box {case}: similarity {sim:.3g} within 1e-2 {np.mean(d <= 1e-2):.4f} max {d.max():.3g}")
        assert sim < 1e-5, case
        assert np.mean(d <= 1e-2) >= 0.99, (case, np.mean(d <= 1e-2))
        assert d.max() <= 0.5, (case, d.max())
        ran += 1
    assert ran == 6


def make_hog(gpu, win=(64, 128)):
    from opencv_amd import hog

    hg = hog.HOG.create(win, ctx=gpu)
    hg.setSVMDetector(hg.getDefaultPeopleDetector())
    return hg


@pytest.mark.parametrize("i", range(len(RC.HOG_GRAD_CASES)))
def test_hog_gradient(gpu, fx, i):
    from opencv_amd import hog

    w, h, cn, gamma, signed, _ = RC.HOG_GRAD_CASES[i]
    hg = make_hog(gpu)
    hg.setGammaCorrection(bool(gamma))
    hg.setSignedGradient(bool(signed))
    g, q = hog.gradient(dev(RC.hog_grad_image(i)), hg, ctx=gpu)
    RC.assert_pinned(q.cpu().numpy().reshape(h, w * 2), fx["hog"][f"{i}_qa"], "qangle")
    RC.assert_pinned(g.cpu().numpy().reshape(h, w * 2), fx["hog"][f"{i}_g"], "gradient")


@pytest.mark.parametrize("k", range(len(RC.HOG_DET_CASES)))
def test_hog_scores_and_rects(gpu, fx, k):
    f = fx["hog"]
    i = len(RC.HOG_GRAD_CASES) + k
    win, cn, group = RC.HOG_DET_CASES[k]
    hg = make_hog(gpu, win)
    hg.setHitThreshold(float(f["hit"][k]))
    hg.setNumLevels(64)
    hg.setScaleFactor(1.05)
    hg.setGroupThreshold(group)
    img = dev(RC.hog_image(160, 256, cn, 300 + win[0] + cn))
    xy, sc = hg.detect(img, confidences=True)
    RC.assert_pinned(np.array(xy, np.int32).reshape(-1, 2), f[f"{i}_loc"], "window positions")
    RC.assert_pinned(np.array(sc, np.float64), f[f"{i}_wt"], "window scores")
    rects, wts = hg.detectMultiScale(img, confidences=True)
    want = sorted(zip(map(tuple, f[f"{i}_r"].reshape(-1, 4).tolist()), f[f"{i}_rw"].tolist()))
    assert len(want) >= 1 and sorted(zip(rects, wts)) == want
