#!/usr/bin/env python3
"""Records the real reference (buildOpticalFlowPyramid, calcOpticalFlowPyrLK,
goodFeaturesToTrack, cornerMinEigenVal / cornerHarris, warpAffine,
calcOpticalFlowFarneback, HOGDescriptor) on the cases of tests/_reference_cases.py
(goodFeaturesToTrack under a mask: tests/_gftt_mask_cases.py; the corner maps and
goodFeaturesToTrack on CV_32F images: tests/_gftt_f32_cases.py; cornerSubPix:
tests/_subpix_cases.py; goodFeaturesToTrack on whole frames:
tests/_gftt_frame_cases.py; remap and warpPerspective: tests/_remap_cases.py;
findHomography: tests/_homography_cases.py; estimateAffine2D and
estimateAffinePartial2D: tests/_affine2d_cases.py; erode, dilate and
morphologyEx: tests/_morph_cases.py; connectedComponentsWithStats:
tests/_cc_cases.py; GaussianBlur on 8-bit images and threshold:
tests/_blur_cases.py)
into tests/golden/reference_<op>.npz, through tools/reference_driver.cpp (how to
build it: tools/record_reference_cases.md).

    python tools/record_reference_cases.py /path/to/reference_driver [op ...] [--out DIR]

Every case runs twice, in child processes: `default` (the reference's own
runtime dispatch) and `noavx2` (OPENCV_CPU_DISABLE=AVX2,AVX512_SKX in the
child's environment only).  The driver prints checkHardwareSupport; a run whose
flags do not show the intended state is an error, so a host without AVX2 cannot
record.  Where the two recordings are byte-identical one copy is stored
(state "both"); this is asserted for the pyramid, PyrLK, warpAffine, remap,
warpPerspective, morph, cc, knn, blur and threshold.  Where
they differ, the state the oracle models is stored in full, and for the other
one: whether the integer-valued results were equal (and those results where
they were not), the share of equal 32-bit words and the largest absolute
difference, per case.  The script prints that
summary as the table kept in tools/record_reference_cases.md.

Nothing in the test suite runs this; the fixtures are committed."""
import io
import os
import subprocess
import sys
import tempfile
import zipfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle as O  # noqa: E402
import _reference_cases as RC  # noqa: E402
import _gftt_mask_cases as MC  # noqa: E402
import _gftt_f32_cases as FC  # noqa: E402
import _subpix_cases as SC  # noqa: E402
import _gftt_frame_cases as WC  # noqa: E402
import _klt_tracker_oracle as KT  # noqa: E402
import _remap_cases as PC  # noqa: E402
import _homography_cases as HC  # noqa: E402
import _affine2d_cases as AC  # noqa: E402
import _mog2_cases as GC  # noqa: E402
import _knn_cases as KC  # noqa: E402
import _morph_cases as BC  # noqa: E402
import _cc_cases as LC  # noqa: E402
import _blur_cases as UC  # noqa: E402
import _blur_oracle as UO  # noqa: E402

LIMIT = 256 * 1024
STATES = ("default", "noavx2")
# the state each oracle file models where the two differ (README, numerics)
MODELLED = {"pyramid": "both", "pyrlk": "both", "warpaffine": "both", "gftt": "noavx2", "gftt_mask": "noavx2",
            "cornermaps": "noavx2", "gftt_f32": "noavx2", "subpix": "both", "gftt_frame": "noavx2",
            "circle": "both", "remap": "both", "warpperspective": "both", "farneback": "noavx2",
            "farneback_box": "noavx2", "hog": "default", "homography": "noavx2", "affine2d": "noavx2", "mog2": "both",
            "morph": "both", "cc": "both", "knn": "both", "blur": "both", "threshold": "both"}


class Driver:
    def __init__(self, path, state, tmp):
        self.path, self.state, self.tmp = path, state, tmp
        self.env = {k: v for k, v in os.environ.items() if k != "OPENCV_CPU_DISABLE"}
        if state == "noavx2":
            self.env["OPENCV_CPU_DISABLE"] = "AVX2,AVX512_SKX"

    def run(self, op, files, **kw):
        """files: name -> array written raw and passed as name=<path>.  Returns
        (the driver's output lines after the flags line, reader(name, dtype))."""
        args = []
        for name, arr in files.items():
            p = os.path.join(self.tmp, f"in.{name}")
            np.ascontiguousarray(arr).tofile(p)
            args.append(f"{name}={p}")
        args += [f"{k}={v!r}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()]
        prefix = os.path.join(self.tmp, "out")
        txt = subprocess.run([self.path, op, prefix, *args], check=True, capture_output=True, text=True,
                             env=self.env).stdout.splitlines()
        flags = dict(kv.split("=") for kv in txt[0].split())
        want = "1" if self.state == "default" else "0"
        if flags["AVX2"] != want or flags["SSE4_1"] != "1":
            raise SystemExit(f"state {self.state}: the driver reports {txt[0]}")
        return txt[1:], lambda name, dt: np.fromfile(f"{prefix}.{name}", dt)


def img_kw(img):
    return dict(w=img.shape[1], h=img.shape[0], cn=1 if img.ndim == 2 else img.shape[2])


# Each recorder returns (cases, extra): cases a list of (ints, floats), two dicts
# name -> array of one case's integer-valued and float results; extra: arrays
# that describe the cases (the same in both states).

def rec_pyramid(d):
    cases, meta = [], []
    for w, h, cn, win, maxl, seed in RC.PYR_CASES:
        img = RC.noise(w, h, cn, seed)
        out, rd = d.run("pyr", dict(a=img), **img_kw(img), winw=win[0], winh=win[1], maxl=maxl)
        n = int(out[0].split()[1])
        ints = {}
        for i in range(n):
            lw, lh = map(int, out[1 + i].split())
            ints[f"L{i}"] = rd(f"L{i}", np.uint8).reshape(lh, lw * cn)
            ints[f"D{i}"] = rd(f"D{i}", np.int16).reshape(lh, lw * cn * 2)
        cases.append((ints, {}))
        meta.append((w, h, cn, win[0], win[1], maxl, seed, n))
    return cases, dict(meta=np.array(meta, np.int32))


def lk_points(d):
    """per pair: the frame's own GFTT corners plus the fixed edge points, and an initial guess"""
    extra = {}
    for pair in RC.LK_PAIRS:
        a, _ = RC.lk_pair(pair, 1)
        _, rd = d.run("gftt", dict(a=a), **img_kw(a), maxc=150, ql=0.01, md=5.0, block=3, harris=0, k=0.04)
        pts = np.concatenate([rd("c", np.float32).reshape(-1, 2), RC.LK_EDGE_POINTS])
        n = RC.noise(len(pts), 1, 2, 55).astype(np.float32).reshape(-1, 2)
        extra[f"pts_{pair}"] = pts
        extra[f"init_{pair}"] = pts + (n - np.float32(128)) / np.float32(64)  # a guess within 2 px
    return extra


def rec_pyrlk(d, extra):
    cases = []
    for pair, cn, win, lev, flags, want_err in RC.lk_cases():
        a, b = RC.lk_pair(pair, cn)
        pts = extra[f"pts_{pair}"]
        files = dict(a=a, b=b, pts=pts)
        if flags & RC.OPTFLOW_USE_INITIAL_FLOW:
            files["init"] = extra[f"init_{pair}"]
        _, rd = d.run("lk", files, **img_kw(a), winw=win[0], winh=win[1], maxl=lev, flags=flags, n=len(pts),
                      err=want_err)
        floats = dict(q=rd("q", np.float32).reshape(-1, 2))
        if want_err:
            floats["err"] = rd("err", np.float32)
        cases.append((dict(st=rd("st", np.uint8)), floats))
    return cases, extra


def lk_exact_order_check(cases, extra):
    """O.lk(..., accum=ACCUM_EXACT), the order the kernels are proven equal to,
    meets test_gpu_klt.assert_tolerance's default bars against every recorded
    case; returns per pair the points that spoil a case (to be replaced)."""
    from test_gpu_klt import assert_tolerance

    spoil = {p: set() for p in RC.LK_PAIRS}
    for (pair, cn, win, lev, flags, want_err), (ints, floats) in zip(RC.lk_cases(), cases):
        a, b = RC.lk_pair(pair, cn)
        Pa, Pb = O.Pyramid(a, win, lev, RC.lk_pad(win)), O.Pyramid(b, win, lev, RC.lk_pad(win))
        init = extra[f"init_{pair}"] if flags & RC.OPTFLOW_USE_INITIAL_FLOW else None
        ex = O.lk(Pa, Pb, extra[f"pts_{pair}"], win, lev, 30, 0.01, flags, accum=O.ACCUM_EXACT, init=init,
                  want_err=bool(want_err))
        try:
            assert_tolerance(ex, (floats["q"], ints["st"]))
        except AssertionError:
            both = (ex[1] == 1) & (ints["st"] == 1)
            far = both & (np.abs(ex[0] - floats["q"]).max(1) > 1e-2)
            spoil[pair] |= set(np.flatnonzero((ex[1] != ints["st"]) | far).tolist())
    return spoil


def rec_gftt(d):
    cases, meta = [], []
    for r, maxc, ql, md, block, harris in RC.gftt_cases():
        roi = RC.gftt_roi(r)
        _, rd = d.run("gftt", dict(a=roi), **img_kw(roi), maxc=maxc, ql=ql, md=md, block=block, harris=harris,
                      k=RC.HARRIS_K)
        c = rd("c", np.float32).reshape(-1, 2)
        assert np.array_equal(c, c.astype(np.uint16))  # corners are pixel positions: stored as uint16, exactly
        cases.append((dict(c=c.astype(np.uint16)), {}))
        meta.append((r, maxc, block, harris))
    return cases, dict(meta=np.array(meta, np.int32))


def rec_gftt_mask(d):
    """goodFeaturesToTrack with its mask argument (tests/_gftt_mask_cases.py); the
    masks travel in the fixture, bit-packed"""
    entries = MC.masks()
    masks = [MC.mask_of(e) for e in entries]
    extra = {}
    for m, mask in enumerate(masks):
        extra[f"mask_{m}_bits"], extra[f"mask_{m}_val"] = MC.pack_mask(mask)
    cases = []
    for r, m, maxc, ql, md, block, harris in MC.cases():
        roi = MC.roi_image(r)
        _, rd = d.run("gftt", dict(a=roi, mask=masks[m]), **img_kw(roi), maxc=maxc, ql=ql, md=md, block=block,
                      harris=harris, k=MC.HARRIS_K)
        c = rd("c", np.float32).reshape(-1, 2)
        assert np.array_equal(c, c.astype(np.uint16))
        cases.append((dict(c=c.astype(np.uint16)), {}))
    extra["case_mask"] = np.array([c[1] for c in MC.cases()], np.int32)
    return cases, extra


def rec_cornermaps(d):
    cases, meta = [], []
    for w, h, seed in RC.CMAP_SHAPES:
        img = RC.noise(w, h, 1, seed)
        for block, harris in RC.CMAP_MODES:
            _, rd = d.run("cmap", dict(a=img), **img_kw(img), block=block, harris=harris, k=RC.HARRIS_K)
            cases.append(({}, dict(e=rd("e", np.float32).reshape(h, w))))
            meta.append((w, h, seed, block, harris))
    return cases, dict(meta=np.array(meta, np.int32))


def rec_gftt_f32(d):
    """cornerMinEigenVal / cornerHarris and goodFeaturesToTrack on CV_32F images
    (tests/_gftt_f32_cases.py): the maps first, then the lists"""
    cases = []
    for h, w, kind, block, harris in FC.map_cases():
        img = np.ascontiguousarray(FC.map_image(h, w, kind), dtype=np.float32)
        _, rd = d.run("cmap", dict(a=img), w=w, h=h, depth="32f", block=block, harris=harris, k=FC.HARRIS_K)
        cases.append(({}, dict(e=rd("e", np.float32).reshape(h, w))))
    for kind, r, mk, maxc, ql, md, block, harris in FC.list_cases():
        roi = np.ascontiguousarray(FC.list_image(kind, r), dtype=np.float32)
        h, w = roi.shape
        files = dict(a=roi)
        if mk != "none":
            files["mask"] = FC.list_mask(mk, w, h)
        _, rd = d.run("gftt", files, w=w, h=h, depth="32f", maxc=maxc, ql=ql, md=md, block=block, harris=harris,
                      k=FC.HARRIS_K)
        c = rd("c", np.float32).reshape(-1, 2)
        assert np.array_equal(c, c.astype(np.uint16))
        cases.append((dict(c=c.astype(np.uint16)), {}))
    return cases, dict(nmaps=np.array(len(FC.map_cases()), np.int32))


def rec_gftt_frame(d):
    """goodFeaturesToTrack on whole frames (tests/_gftt_frame_cases.py): the lists whole, as int16 pairs"""
    cases = []
    for name, mk, maxc, ql, md, block, harris, _ in WC.CASES:
        img = WC.frame(name)
        h, w = img.shape
        files = dict(a=img)
        if mk != "none":
            files["mask"] = WC.mask(mk, name)
        kw = dict(depth="32f") if img.dtype == np.float32 else dict(cn=1)
        _, rd = d.run("gftt", files, w=w, h=h, **kw, maxc=maxc, ql=ql, md=md, block=block, harris=harris,
                      k=WC.HARRIS_K)
        c = rd("c", np.float32).reshape(-1, 2)
        assert np.array_equal(c, c.astype(np.int16))
        cases.append((dict(c=c.astype(np.int16)), {}))
    return cases, {}


def rec_subpix(d):
    """cornerSubPix (tests/_subpix_cases.py): per image its point set (the 8-bit
    image's goodFeaturesToTrack corners, moved copies, special points), stored in
    the fixture; per case the refined points; and the driver's expf table"""
    extra = {}
    for name, _, _, _ in SC.IMAGES:
        img = SC.image(name)
        _, rd = d.run("gftt", dict(a=img), **img_kw(img), maxc=SC.GFTT[0], ql=SC.GFTT[1], md=SC.GFTT[2], block=3,
                      harris=0, k=0.04)
        extra[f"pts_{name}"] = SC.points(name, rd("c", np.float32).reshape(-1, 2))
    cases = []
    for name, depth, win, zero, crit in SC.cases():
        img, pts = SC.image(name, depth), extra[f"pts_{name}"]
        out, rd = d.run("subpix", dict(a=img, pts=pts), w=img.shape[1], h=img.shape[0], depth=depth, n=len(pts),
                        winw=win[0], winh=win[1], zw=zero[0], zh=zero[1], ctype=crit[0], cmax=crit[1],
                        ceps=float(crit[2]))
        cases.append(({}, dict(c=rd("c", np.float32).reshape(-1, 2))))
        table = np.zeros((15, 16), np.float32)
        for line in out:
            f = line.split()
            assert f[0] == "expf" and len(f) == int(f[1]) + 3, line
            table[int(f[1]) - 1, :len(f) - 2] = np.array([int(b, 16) for b in f[2:]], np.uint32).view(np.float32)
        assert "expf" not in extra or np.array_equal(extra["expf"].view(np.uint32), table.view(np.uint32))
        extra["expf"] = table
    return cases, extra


def rec_circle(d):
    """circle(img, c, r, Scalar(0), -1) on a 255-filled image (tests/_klt_tracker_oracle.py: CIRCLE_CASES): the
    drawn pixels, bit-packed"""
    w, h = KT.CIRCLE_SIZE
    cases = []
    for cx, cy, r in KT.CIRCLE_CASES:
        _, rd = d.run("circle", {}, w=w, h=h, cx=cx, cy=cy, r=r)
        m = rd("m", np.uint8).reshape(h, w)
        assert np.isin(m, (0, 255)).all()
        cases.append((dict(m=np.packbits(m == 0)), {}))
    return cases, {}


def warp_table():
    """(flags, border, bval, sw, sh, dw, dh, M) per case: 4 interpolations x 6 borders x
    the inverse flag on matrices drawn from a fixed seed, then the degenerate matrices"""
    rng = np.random.default_rng(20261019)
    rows, i = [], 0
    for inter in range(4):
        for border in range(6):
            for inv in (0, O.WARP_INVERSE_MAP):
                (sw, sh), (dw, dh) = RC.WARP_SRC[i % len(RC.WARP_SRC)], RC.WARP_DST[i % len(RC.WARP_DST)]
                ang, sc = np.deg2rad(rng.uniform(-180, 180)), rng.uniform(0.4, 2.0)
                al, be = np.cos(ang) * sc, np.sin(ang) * sc
                M = np.array([[al, be, (1 - al) * sw / 2 - be * sh / 2], [-be, al, be * sw / 2 + (1 - al) * sh / 2]])
                M[:, 2] += rng.uniform(-10, 10, 2)
                rows.append((inter | inv, border, int(rng.integers(0, 256)), sw, sh, dw, dh, M))
                i += 1
    for M in RC.WARP_DEGENERATE:
        for inter in (O.INTER_LINEAR, O.INTER_CUBIC):
            rows.append((inter, O.BORDER_CONSTANT, 3, 96, 61, 70, 50, np.asarray(M, np.float64)))
    return rows


def rec_warpaffine(d):
    cases, meta, mats = [], [], []
    for i, (flags, border, bval, sw, sh, dw, dh, M) in enumerate(warp_table()):
        src, dst = RC.warp_inputs(i, sw, sh, dw, dh)
        _, rd = d.run("warp", dict(a=src, m=M, dst=dst), w=sw, h=sh, dw=dw, dh=dh, flags=flags, border=border,
                      bval=bval)
        cases.append((dict(w=rd("w", np.uint8).reshape(dh, dw)), {}))
        meta.append((flags, border, bval, sw, sh, dw, dh))
        mats.append(M)
    return cases, dict(meta=np.array(meta, np.int32), M=np.array(mats, np.float64))


def _bv_kw(bv):
    return {f"bv{k}": float(v) for k, v in enumerate(bv)}


def rec_remap(d):
    """remap into a pre-filled destination (tests/_remap_cases.py: remap_cases)"""
    cases = []
    for i, (depth, cn, s, dd, gen, kind, inter, border) in enumerate(PC.remap_cases()):
        src, dst, m1, m2, _, bv = PC.remap_inputs(i)
        files = dict(a=src, dst=dst, m1=m1)
        if m2 is not None:
            files["m2"] = m2
        _, rd = d.run("remap", files, w=src.shape[1], h=src.shape[0], cn=cn, depth=depth, dw=dst.shape[1],
                      dh=dst.shape[0], kind=kind.rstrip("f") if kind.startswith("16") else kind, inter=inter,
                      border=border, **_bv_kw(bv))
        out = rd("w", dst.dtype).reshape(dst.shape)
        cases.append((dict(w=out), {}) if depth == "8u" else ({}, dict(w=out)))
    return cases, {}


def rec_warpperspective(d):
    """warpPerspective into a pre-filled destination, and invert(M) (tests/_remap_cases.py: persp_cases)"""
    cases = []
    for i, (depth, cn, s, dd, name, flags, border) in enumerate(PC.persp_cases()):
        src, dst, M, bv = PC.persp_inputs(i)
        _, rd = d.run("warpperspective", dict(a=src, dst=dst, m=M), w=src.shape[1], h=src.shape[0], cn=cn, depth=depth,
                      dw=dst.shape[1], dh=dst.shape[0], flags=flags, border=border, **_bv_kw(bv))
        out = rd("w", dst.dtype).reshape(dst.shape)
        minv = rd("minv", np.float64)
        cases.append((dict(w=out), dict(minv=minv)) if depth == "8u" else ({}, dict(w=out, minv=minv)))
    return cases, {}


def rec_homography(d):
    """findHomography on the status != 0 pairs (tests/_homography_cases.py): the mask bit-packed, the validity flag,
    H as raw float64 (the identity where the result is empty); the point sets go in as extras"""
    cases, extra = [], {}
    assert len(HC.cases()) == HC.NCASES
    for i in range(HC.NCASES):
        src, dst, st, method, thr, iters, conf = HC.inputs(i)
        extra[f"src_{i}"], extra[f"dst_{i}"] = src, dst
        if st is not None:
            extra[f"status_{i}"] = st
        s, q = HC.compact(src, dst, st)
        txt, rd = d.run("homography", dict(src=s, dst=q) if len(s) else {}, n=len(s), method=method, thr=float(thr),
                        iters=iters, conf=float(conf))
        valid = int(txt[0].split()[1])
        h = rd("h", np.float64).reshape(3, 3) if valid else np.eye(3)
        mask = rd("mask", np.uint8)
        assert mask.size == len(s) and np.isin(mask, (0, 1)).all()
        cases.append((dict(mask=np.packbits(mask), valid=np.array([valid, int(mask.sum())], np.int32)), dict(H=h)))
    return cases, extra


def rec_affine2d(d):
    """estimateAffine2D / estimateAffinePartial2D on the status != 0 pairs (tests/_affine2d_cases.py), with
    refineIters 0 and 10: the mask bit-packed, the validity flag, M as raw float64 (the identity where the result is
    empty); the distinct point sets go in as extras"""
    cases, extra = [], {}
    assert len(AC.cases()) == AC.NCASES
    ids, keys = AC.set_ids()
    for k, key in enumerate(keys):
        extra[f"set_{k}_src"], extra[f"set_{k}_dst"] = AC.points(*key)
    for i in range(AC.NCASES):
        src, dst, st, model, method, thr, iters, conf = AC.inputs(i)
        assert np.array_equal(src, extra[f"set_{ids[i]}_src"]) and np.array_equal(dst, extra[f"set_{ids[i]}_dst"])
        s, q = AC.compact(src, dst, st)
        ints, floats = {}, {}
        for refine in (0, 10):
            txt, rd = d.run("affine2d", dict(src=s, dst=q) if len(s) else {}, n=len(s), model=model, method=method,
                            thr=float(thr), iters=iters, conf=float(conf), refine=refine)
            valid = int(txt[0].split()[1])
            mask = rd("mask", np.uint8)
            assert mask.size == len(s) and np.isin(mask, (0, 1)).all()
            ints[f"r{refine}_mask"] = np.packbits(mask)
            ints[f"r{refine}_valid"] = np.array([valid, int(mask.sum())], np.int32)
            floats[f"r{refine}_M"] = rd("m", np.float64).reshape(2, 3) if valid else np.eye(2, 3)
        cases.append((ints, floats))
    return cases, extra


def rec_mog2(d):
    """BackgroundSubtractorMOG2 over the sequences of tests/_mog2_cases.py: every frame's mask (2 bits a pixel
    for the base rows, one CRC-32 per frame for the others) and the background images after the marked frames
    (8-bit whole, 32F as row CRCs)"""
    cases = []
    rows = GC.cases()
    assert len(rows) == GC.NCASES
    for case in rows:
        p, fr = GC.params(case), GC.case_frames(case)
        n, h, w, cn = case["n"], case["h"], case["w"], case["cn"]
        want = np.array([t + 1 in case["bg"] for t in range(n)], np.uint8)
        _, rd = d.run("mog2", dict(a=fr, rates=case["rates"].astype(np.float64), bg=want), w=w, h=h, cn=cn, n=n,
                      depth="8u" if fr.dtype == np.uint8 else "32f", history=p["history"], nmix=p["nmixtures"],
                      shadows=p["detect_shadows"], sval=p["shadow_value"], vt=float(p["var_threshold"]),
                      vtg=float(p["var_threshold_gen"]), vinit=float(p["var_init"]), vmin=float(p["var_min"]),
                      vmax=float(p["var_max"]), bgr=float(p["background_ratio"]),
                      ct=float(p["complexity_reduction"]), tau=float(p["shadow_threshold"]))
        masks = rd("masks", np.uint8).reshape(n, h, w)
        bgs = rd("bg", fr.dtype).reshape((len(case["bg"]),) + fr.shape[1:])
        ints = dict(masks=GC.stored_masks(case, masks))
        for k, t in enumerate(case["bg"]):
            ints[f"bg{t}"] = GC.stored_background(bgs[k])
        cases.append((ints, {}))
    return cases, {}


def rec_knn(d):
    """BackgroundSubtractorKNN over the sequences of tests/_knn_cases.py, with cv::theRNG() of the calling thread
    set to the case's seed: every frame's mask and the background images after the marked frames (whole for the
    base rows, CRC-32s for the others), the update periods of every frame, and theRNG().state after the last
    frame (two int32 words), which pins the number of steps the fills consumed"""
    cases = []
    rows = KC.cases()
    assert len(rows) == KC.NCASES
    for case in rows:
        p, fr = KC.params(case), KC.case_frames(case)
        n, h, w, cn = case["n"], case["h"], case["w"], case["cn"]
        want = np.array([t + 1 in case["bg"] for t in range(n)], np.uint8)
        _, rd = d.run("knn", dict(a=fr, rates=case["rates"].astype(np.float64), bg=want), w=w, h=h, cn=cn, n=n,
                      seed=p["rng_state"], history=p["history"], nsamples=p["nsamples"], knn=p["knn_samples"],
                      shadows=p["detect_shadows"], sval=p["shadow_value"], d2t=float(p["dist2_threshold"]),
                      tau=float(p["shadow_threshold"]))
        masks = rd("masks", np.uint8).reshape(n, h, w)
        bgs = rd("bg", np.uint8).reshape((len(case["bg"]),) + fr.shape[1:])
        ints = dict(masks=KC.stored_masks(case, masks), periods=rd("periods", np.int32).reshape(n, 3),
                    state=KC.split_state(int(rd("state", np.uint64)[0])))
        for k, t in enumerate(case["bg"]):
            ints[f"bg{t}"] = KC.stored_background(case, bgs[k])
        cases.append((ints, {}))
    return cases, {}


def rec_morph(d):
    """erode / dilate / morphologyEx on the cases of tests/_morph_cases.py, and the getStructuringElement table
    (bit-packed).  The CROSS and ELLIPSE elements the cases use are checked against the reference's own"""
    extra = {}
    for k, (shape, kw, kh, anchor) in enumerate(BC.strel_cases()):
        _, rd = d.run("strel", {}, shape=shape, kw=kw, kh=kh, ax=anchor[0], ay=anchor[1])
        e = rd("e", np.uint8).reshape(kh, kw)
        assert np.isin(e, (0, 1)).all()
        extra[f"strel_{k}"] = np.packbits(e)
    elems = BC.elements()
    for name, (shape, kw, kh, anchor) in BC.shaped().items():
        _, rd = d.run("strel", {}, shape=shape, kw=kw, kh=kh, ax=anchor[0], ay=anchor[1])
        assert np.array_equal(rd("e", np.uint8).reshape(kh, kw), elems[name]), name
    cases = []
    for c in BC.cases():
        img, e = BC.image(c["w"], c["h"], c["content"]), elems[c["elem"]]
        files, kw = dict(a=img), {}
        if e is not None:
            files["elem"] = e
            kw = dict(kw=e.shape[1], kh=e.shape[0])
        _, rd = d.run("morph", files, w=c["w"], h=c["h"], mop=c["op"], ax=c["anchor"][0], ay=c["anchor"][1],
                      it=c["it"], border=c["border"], bval=c["bval"], inplace=int(c["inplace"]), **kw)
        cases.append((dict(d=rd("d", np.uint8).reshape(c["h"], c["w"])), {}))
    return cases, extra


def rec_cc(d):
    """connectedComponentsWithStats on the cases of tests/_cc_cases.py: per case `s`, N rows of nine int32 (the
    five stats, then the two centroids' 64-bit words, low half first: row 0 of an image without background is
    0/0), always whole, and the labels whole or as row CRCs"""
    cases = []
    for content, w, h, conn, t in LC.cases():
        out, rd = d.run("cc", dict(a=LC.image(content, w, h)), w=w, h=h, conn=conn, type=t)
        n = int(out[0].split()[1])
        ints = dict(labels=LC.stored_labels(rd("labels", np.int32).reshape(h, w)),
                    s=LC.stored_stats(rd("stats", np.int32).reshape(n, 5), rd("cent", np.float64).reshape(n, 2)))
        cases.append((ints, {}))
    return cases, {}


def rec_blur(d):
    """GaussianBlur on the cases of tests/_blur_cases.py, and the coefficient sweep: every (n, sigma) pair's
    response to the two impulses of the one-row sweep image (2 n bytes a pair), which determines the n 8.8
    coefficients.  The host table's restatement is checked against every response"""
    pairs = UC.sweep_pairs()
    img = UC.sweep_image()
    _, rd = d.run("blurk", dict(a=img, pairs=np.array(pairs, np.float64)), w=UC.SWEEP_W, n=len(pairs))
    resp = rd("resp", np.uint8).reshape(len(pairs), UC.SWEEP_W)
    rows, sums = [], []
    for (n, sigma), r in zip(pairs, resp):
        win = np.concatenate([r[p - n // 2:p + n // 2 + 1] for p in (UC.SWEEP_P0, UC.SWEEP_P1)])
        keep = np.zeros(UC.SWEEP_W, bool)
        for p in (UC.SWEEP_P0, UC.SWEEP_P1):
            keep[p - n // 2:p + n // 2 + 1] = True
        assert not r[~keep].any(), (n, sigma, "a response outside the kernel's reach")
        k = UO.gaussian_kernel_u8(n, sigma)
        assert np.array_equal(UC.sweep_response(k), win), (n, sigma, "the restated coefficients miss the response")
        assert np.array_equal(UC.sweep_decode(win, n), k), (n, sigma)
        rows.append(win)
        sums.append(int(k.sum()))
    sums = np.array(sums)
    if d.state == "default":
        print(f"blur: coefficient sweep of {len(pairs)} pairs: {int((sums >= 258).sum())} sum to 258 or more, "
              f"{int((sums > 256).sum())} to more than 256, {int((sums < 256).sum())} to less; the largest sum is "
              f"{int(sums.max())} at (n, sigma) = {pairs[int(sums.argmax())]}, the smallest {int(sums.min())}")
    extra = dict(coef_pairs=np.array(pairs, np.float64), coef_resp=np.concatenate(rows))
    kernels = UC.kernels()
    cases = []
    for c in UC.cases():
        kw, kh, sx, sy = kernels[c["kernel"]]
        _, rd = d.run("blur", dict(a=UC.case_image(c)), w=c["w"], h=c["h"], cn=c["cn"], kw=kw, kh=kh, sx=float(sx),
                      sy=float(sy), border=c["border"], inplace=int(c["inplace"]))
        shape = (c["h"], c["w"]) if c["cn"] == 1 else (c["h"], c["w"], c["cn"])
        cases.append((dict(d=rd("d", np.uint8).reshape(shape)), {}))
    return cases, extra


def rec_threshold(d):
    """threshold on the cases of tests/_blur_cases.py: the output and the returned value"""
    cases = []
    for c in UC.thresh_cases():
        img = UC.thresh_image(c)
        _, rd = d.run("threshold", dict(a=img), w=img.shape[1], h=img.shape[0], cn=1,
                      depth="32f" if img.dtype == np.float32 else "8u", thresh=float(c["thresh"]),
                      maxval=float(c["maxval"]), type=c["type"])
        out = rd("d", img.dtype).reshape(img.shape)
        ints = dict(d=out.view(np.int32) if img.dtype == np.float32 else out, t=rd("t", np.float64).view(np.int64))
        cases.append((ints, {}))
    return cases, {}


def rec_farneback(d, table=None):
    cases, meta = [], []
    for w, h, ps, pn, ws, flags, use_init in table or RC.FB_CASES:
        a, b = RC.fb_pair(w, h)
        files = dict(a=a, b=b)
        if use_init:
            files["init"] = RC.fb_init(w, h)
        _, rd = d.run("fb", files, w=w, h=h, ps=float(ps), lv=RC.FB_LEVELS, ws=ws, it=RC.FB_ITERS, pn=pn,
                      sg=RC.fb_sigma(pn), flags=flags | (O.OPTFLOW_USE_INITIAL_FLOW if use_init else 0))
        cases.append(({}, dict(f=rd("f", np.float32).reshape(h, w * 2))))
        meta.append((w, h, int(round(ps * 10)), pn, ws, flags, use_init))
    return cases, dict(meta=np.array(meta, np.int32))


def rec_farneback_box(d):
    return rec_farneback(d, RC.FB_BOX_CASES)


def hog_thresholds(d):
    """per detection case a hit threshold (a multiple of 1/64) at which detect()
    and the ungrouped detectMultiScale() both return between 10 and 500 windows:
    the lowest of a few quantiles of the image's window scores that does"""
    hits = []
    for win, cn, _ in RC.HOG_DET_CASES:
        img = RC.hog_image(160, 256, cn, 300 + win[0] + cn)
        _, rd = d.run("hogdet", dict(a=img), **img_kw(img), win=win[0], hit=-1e9, group=0)
        scores = rd("wt", np.float64)
        for q in (0.5, 2 / 3, 0.8, 0.9, 0.95):
            hit = float(np.floor(np.quantile(scores, q) * 64) / 64)
            out, _ = d.run("hogdet", dict(a=img), **img_kw(img), win=win[0], hit=hit, group=0)
            nwin, nrect = int(out[0].split()[1]), int(out[0].split()[3])
            if 10 <= nwin <= 500 and 10 <= nrect <= 500:
                break
        else:
            raise SystemExit(f"hog {win} cn {cn}: no threshold gives 10 to 500 windows")
        hits.append(hit)
    return np.array(hits, np.float64)


def rec_hog(d, extra):
    cases = []
    for i, (w, h, cn, gamma, signed, _) in enumerate(RC.HOG_GRAD_CASES):
        img = RC.hog_grad_image(i)
        _, rd = d.run("hoggrad", dict(a=img), **img_kw(img), gamma=gamma, signed=signed)
        cases.append((dict(qa=rd("qa", np.uint8).reshape(h, w * 2)), dict(g=rd("g", np.float32).reshape(h, w * 2))))
    for (win, cn, group), hit in zip(RC.HOG_DET_CASES, extra["hit"]):
        img = RC.hog_image(160, 256, cn, 300 + win[0] + cn)
        _, rd = d.run("hogdet", dict(a=img), **img_kw(img), win=win[0], hit=float(hit), group=group)
        loc, r = rd("loc", np.int32).reshape(-1, 2), rd("r", np.int32).reshape(-1, 4)
        if not (10 <= len(loc) <= 500 and (len(r) >= 1 if group else 10 <= len(r) <= 500)):
            raise SystemExit(f"hog {win} cn {cn} group {group}: {len(loc)} windows, {len(r)} rects at {hit}")
        svm = rd("svm", np.float32)
        mine = np.fromfile(os.path.join(ROOT, "opencv_amd", "data", f"hog_people_{win[0]}x{win[1]}.f32"), np.float32)
        if not np.array_equal(svm.view(np.uint32), mine.view(np.uint32)):
            raise SystemExit(f"the {win} detector differs from opencv_amd/data")
        extra[f"svm_crc_{win[0]}"] = np.array([zlib.crc32(svm.tobytes()), svm.size], np.uint32)
        cases.append((dict(loc=loc, r=r), dict(wt=rd("wt", np.float64), rw=rd("rw", np.float64))))
    return cases, extra


def words(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def merge(op, rec, whole_limit):
    """rec: state -> (cases, extra).  Returns (arrays, table rows)."""
    modelled = MODELLED[op]
    (c0, extra), (c1, extra1) = rec["default"], rec["noavx2"]
    assert extra.keys() == extra1.keys() and all(np.array_equal(extra[k], extra1[k]) for k in extra), op
    n = len(c0)
    ints_eq, share, maxabs = np.ones(n, np.uint8), np.ones(n), np.zeros(n)
    for i, ((i0, f0), (i1, f1)) in enumerate(zip(c0, c1)):
        ints_eq[i] = all(i0[k].shape == i1[k].shape and np.array_equal(i0[k], i1[k]) for k in i0)
        same = [f0[k].shape == f1[k].shape for k in f0]
        if f0 and all(same):
            eq = np.concatenate([words(f0[k]) == words(f1[k]) for k in f0])
            share[i] = eq.mean() if eq.size else 1.0
            maxabs[i] = max([float(np.abs(f0[k].astype(np.float64) - f1[k]).max()) for k in f0 if f0[k].size] or [0.0])
        elif f0:
            share[i], maxabs[i] = 0.0, np.inf  # another number of results
    identical = bool(ints_eq.all() and (share == 1.0).all())
    if modelled == "both" and not identical:
        raise SystemExit(f"{op}: the two dispatch states differ: ints {ints_eq.tolist()} share {share.tolist()}")
    state = "both" if identical else modelled
    keep, other = (c1, c0) if state == "noavx2" else (c0, c1)
    arrays = {k: v for k, v in extra.items()}
    for i, (ints, floats) in enumerate(keep):
        for k, v in {**ints, **floats}.items():
            arrays[f"{i}_{k}"] = RC.pack(v, whole_limit)
        if not ints_eq[i]:  # the other state's integer-valued results, where they are not the same
            for k, v in other[i][0].items():
                arrays[f"other_{i}_{k}"] = RC.pack(v, whole_limit)
    arrays["state"] = np.array(state)
    arrays["other_ints_equal"], arrays["other_share"], arrays["other_maxabs"] = ints_eq, share, maxabs
    return arrays, (state, ints_eq, share, maxabs)


RECORDERS = {"pyramid": rec_pyramid, "pyrlk": rec_pyrlk, "gftt": rec_gftt, "gftt_mask": rec_gftt_mask,
             "cornermaps": rec_cornermaps, "gftt_f32": rec_gftt_f32, "subpix": rec_subpix, "gftt_frame": rec_gftt_frame,
             "circle": rec_circle, "warpaffine": rec_warpaffine, "remap": rec_remap,
             "warpperspective": rec_warpperspective, "farneback": rec_farneback, "farneback_box": rec_farneback_box,
             "hog": rec_hog, "homography": rec_homography, "affine2d": rec_affine2d, "mog2": rec_mog2,
             "morph": rec_morph, "cc": rec_cc, "knn": rec_knn, "blur": rec_blur, "threshold": rec_threshold}
# bytes up to which an output is stored whole (tests/_reference_cases.py: WHOLE_LIMIT).  The kernels are
# compared with the box Farneback flows within a tolerance, so all six stay whole (about 7 KB under LIMIT)
WHOLE = {"farneback": 20480, "farneback_box": 72800, "pyrlk": 1 << 20, "gftt": 1 << 20, "gftt_mask": 1 << 20,
         "hog": 16384, "subpix": 1 << 20, "gftt_frame": 1 << 20, "remap": PC.WHOLE_LIMIT,
         "warpperspective": PC.WHOLE_LIMIT, "homography": 1 << 20, "affine2d": 1 << 20, "mog2": 1 << 20,
         "morph": BC.WHOLE_LIMIT, "cc": 1 << 20, "knn": 1 << 20, "blur": UC.WHOLE_LIMIT,
         "threshold": UC.WHOLE_LIMIT}
# (gftt_f32: maps above RC.WHOLE_LIMIT as row CRCs; its corner lists are far below it)


def save(path, arrays):
    """np.savez_compressed with fixed member times, so a re-recording gives the same file"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       zipfile.ZIP_DEFLATED)


def case_label(op, i):
    if op == "pyrlk":
        pair, cn, win, lev, flags, err = RC.lk_cases()[i]
        return f"{pair} cn {cn} win {win[0]}x{win[1]} levels {lev} flags {flags}" + ("" if err else " no err")
    if op == "gftt":
        r, maxc, ql, md, block, harris = RC.gftt_cases()[i]
        return f"roi {r} ({maxc}, {ql}, {md}) block {block}" + (" harris" if harris else "")
    if op == "gftt_mask":
        r, m, maxc, ql, md, block, harris = MC.cases()[i]
        return f"roi {r} mask {MC.masks()[m][1]} ({maxc}, {ql}, {md}) block {block}" + (" harris" if harris else "")
    if op == "gftt_f32":
        nm = len(FC.map_cases())
        if i < nm:
            h, w, kind, block, harris = FC.map_cases()[i]
            return f"{kind} {h}x{w} block {block} " + ("harris" if harris else "minEigenVal")
        kind, r, mk, maxc, ql, md, block, harris = FC.list_cases()[i - nm]
        return f"{kind} roi {r} mask {mk} ({maxc}, {ql}, {md}) block {block}" + (" harris" if harris else "")
    if op == "subpix":
        return SC.label(i)
    if op == "gftt_frame":
        return WC.label(i)
    if op == "remap":
        return PC.remap_label(i)
    if op == "warpperspective":
        return PC.persp_label(i)
    if op == "homography":
        return HC.label(i)
    if op == "affine2d":
        return AC.label(i)
    if op == "mog2":
        return GC.label(i)
    if op == "knn":
        return KC.label(i)
    if op == "morph":
        return BC.label(i)
    if op == "cc":
        return LC.label(i)
    if op == "blur":
        return UC.label(i)
    if op == "threshold":
        return UC.thresh_label(i)
    if op == "circle":
        return "centre ({}, {}) radius {}".format(*KT.CIRCLE_CASES[i])
    if op == "cornermaps":
        w, h, _ = RC.CMAP_SHAPES[i // len(RC.CMAP_MODES)]
        block, harris = RC.CMAP_MODES[i % len(RC.CMAP_MODES)]
        return f"{h}x{w} block {block} " + ("harris" if harris else "minEigenVal")
    if op in ("farneback", "farneback_box"):
        w, h, ps, pn, ws, flags, init = (RC.FB_CASES if op == "farneback" else RC.FB_BOX_CASES)[i]
        return f"{w}x{h} scale {ps} polyN {pn} win {ws} " + ("gaussian" if flags else "box") + (" init" if init else "")
    if op == "hog":
        g = len(RC.HOG_GRAD_CASES)
        if i < g:
            return "computeGradient {}x{} cn {} gamma {} signed {}".format(*RC.HOG_GRAD_CASES[i])
        win, cn, group = RC.HOG_DET_CASES[i - g]
        return f"detect / detectMultiScale {win[0]}x{win[1]} cn {cn} group {group}"
    return f"case {i}"


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(ROOT, "tests", "golden")
    if "--out" in argv:
        k = argv.index("--out")
        out_dir = argv[k + 1]
        del argv[k:k + 2]
    driver, ops = argv[0], argv[1:] or list(RECORDERS)
    table = []
    with tempfile.TemporaryDirectory() as tmp:
        drv = {s: Driver(driver, s, tmp) for s in STATES}
        for op in ops:
            rec = {}
            if op == "pyrlk":
                extra = lk_points(drv["noavx2"])
                assert all(np.array_equal(v, lk_points(drv["default"])[k]) for k, v in extra.items())
                for _ in range(8):
                    rec = {s: rec_pyrlk(drv[s], dict(extra)) for s in STATES}
                    spoil = lk_exact_order_check(rec["default"][0], extra)
                    if not any(spoil.values()):
                        break
                    for pair, idx in spoil.items():  # other points: drop the ones that spoil a case
                        if not idx:
                            continue
                        n_gftt = len(extra[f"pts_{pair}"]) - len(RC.LK_EDGE_POINTS)
                        assert all(i < n_gftt for i in idx), (pair, "an edge point misses the bars", sorted(idx))
                        keep = np.array([i not in idx for i in range(len(extra[f"pts_{pair}"]))])
                        print(f"pyrlk: {pair}: dropping points {sorted(idx)}")
                        for k in (f"pts_{pair}", f"init_{pair}"):
                            extra[k] = extra[k][keep]
                else:
                    raise SystemExit("pyrlk: no point set meets the bars")
                assert all(len(extra[f"pts_{p}"]) <= 400 for p in RC.LK_PAIRS)
            elif op == "hog":
                hit = hog_thresholds(drv["default"])
                rec = {s: rec_hog(drv[s], dict(hit=hit)) for s in STATES}
            else:
                rec = {s: RECORDERS[op](drv[s]) for s in STATES}
            arrays, row = merge(op, rec, WHOLE.get(op, RC.WHOLE_LIMIT))
            if op == "homography":  # the refined H is compared between the states by what it does to points: keep both
                for i, ((_, f0), (_, f1)) in enumerate(zip(rec["default"][0], rec["noavx2"][0])):
                    if f0["H"].tobytes() != f1["H"].tobytes():
                        arrays[f"other_{i}_H"] = f0["H"]
            if op == "affine2d" and row[0] != "both":  # both states' M wherever they differ
                for i, ((_, f0), (_, f1)) in enumerate(zip(rec["default"][0], rec["noavx2"][0])):
                    for k in f0:
                        if f0[k].tobytes() != f1[k].tobytes():
                            arrays[f"other_{i}_{k}"] = f0[k]
            path = os.path.join(out_dir, f"reference_{op}.npz")
            save(path, arrays)
            size = os.path.getsize(path)
            print(f"{path}: {len(rec['default'][0])} cases, state {row[0]}, {size} bytes")
            assert size <= LIMIT, (op, size)
            table.append((op, *row))
    print("\n| fixture | case | stored state | integer results equal in the other state | equal 32-bit words | "
          "largest difference |\n|---|---|---|---|---|---|")
    for op, state, ints_eq, share, maxabs in table:
        if state == "both":
            print(f"| {op} | all {len(share)} | both | yes | 100 % | 0 |")
            continue
        same = ints_eq.astype(bool) & (share == 1.0)
        if same.any():
            print(f"| {op} | {int(same.sum())} cases of {len(share)} | {state} | yes | 100 % | 0 |")
        for i in np.flatnonzero(~same):
            print(f"| {op} | {case_label(op, i)} | {state} | {'yes' if ints_eq[i] else 'NO'} | "
                  f"{100 * share[i]:.1f} % | {maxabs[i]:.3g} |")


if __name__ == "__main__":
    main()
