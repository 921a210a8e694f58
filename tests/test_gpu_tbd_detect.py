"""The detection-driven step end to end (tbdk_tbd_step_image): BGR frames in,
HOG detections, tracks out, against an independent CPU pipeline:
tests/_frontend_oracle.py (cvtColor / resize) -> O.hog_detect_multiscale ->
oracle/tbd_loop_oracle.KltTbdLoop stepped with those detections.  Nothing of
the GPU's output feeds the oracle.

Inputs: 8 frames of O.synth(7, W, H, 6, 0, 8); each BGR channel is
clip(g + rng.integers(-30, 30)) with default_rng(7) drawn frame by frame,
channel by channel.  The 48x96 detector, nlevels 15, scale 1.05, group 2, hit
threshold -1.0; loop bounds (0, 320, 0, 240).

Per frame: the detections returned equal the oracle's, unsorted (rects, and
weights when they are the confidences); metrics, KLT predictions (1e-4 px,
the box fit's tolerance) and track rows are compared as
tests/test_gpu_tbd_e2e.py compares them.

What keeps the comparison honest is checked on the oracle alone first
(test_oracle_meets_the_conditions): every frame has >= 8 detections; with
track_confidence_threshold -1 at least 10 tracks are alive after the last
frame, which predicted >= 10 of them by KLT; with the threshold 0.2 the two
confidence modes differ in their track counts (the sample's -1.0 confidence
makes deleteLostTracks drop every detected track, tbd.cpp:913-929, 1025-1026).
The resized case (400x300 -> 320x240) meets them at hit threshold -1.0 as well
(no lowering was needed)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import tbd_loop_oracle as L  # noqa: E402
import _frontend_oracle as F  # noqa: E402

O, T = L.O, L.T

NF, W, H = 8, 320, 240
HIT = -1.0          # every case, the resized one included (see the module docstring)
NLEVELS, SCALE0, GROUP = 15, 1.05, 2
BOUNDS = (0, W, 0, H)
METRIC_KEYS = ("tp", "fn", "fp", "gt", "ntracks", "lk_points", "klt_points", "klt_predicted", "redetected")
# name -> (source size, make_gray)
CASES = {"plain": ((320, 240), True), "resized": ((400, 300), True), "colour": ((320, 240), False)}
# (case, confidence_mode, track_confidence_threshold)
RUNS = [("plain", 0, 0.2), ("plain", 1, 0.2), ("plain", 0, -1.0), ("plain", 1, -1.0), ("resized", 1, -1.0),
        ("colour", 1, -1.0)]


def svm48():
    return np.fromfile(os.path.join(ROOT, "opencv_amd", "data", "hog_people_48x96.f32"), dtype="<f4")


@functools.lru_cache(maxsize=None)
def bgr_frames(size):
    g, _ = O.synth(7, size[0], size[1], 6, 0, NF)
    rng = np.random.default_rng(7)
    out = []
    for f in range(NF):
        ch = [np.clip(g[f].astype(np.int64) + rng.integers(-30, 30, g[f].shape), 0, 255).astype(np.uint8)
              for _ in range(3)]
        out.append(np.ascontiguousarray(np.stack(ch, 2)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_front(case):
    """per frame: (the loop's gray frame, detection rects, weights), CPU only"""
    size, make_gray = CASES[case]
    prm, svm = O.hog_params(win=(48, 96)), svm48()
    out = []
    for bgr in bgr_frames(size):
        if make_gray:
            gray = F.cvt_resize_gray(bgr, F.COLOR_BGR2GRAY, (W, H))
            img = gray
        else:
            img = F.resize_linear(bgr, (W, H))
            gray = F.cvt_color(img, F.COLOR_BGR2GRAY)
        r, w = O.hog_detect_multiscale(np.ascontiguousarray(img), prm, svm, hit_threshold=HIT, nlevels=NLEVELS,
                                       scale0=SCALE0, group_threshold=GROUP)
        out.append((np.ascontiguousarray(gray), r.copy(), w.copy()))
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(case, mode, thr):
    """per frame: (metrics, predictions, track rows) of the oracle loop on the oracle's detections"""
    ora = L.KltTbdLoop(W, H, bounds=BOUNDS, nthreads=min(16, os.cpu_count() or 1), track_confidence_threshold=thr)
    out = []
    for f, (gray, rects, wts) in enumerate(oracle_front(case)):
        dets = [T.Detection(-1, f, T.Rect(*(int(v) for v in r)), float(wts[i]) if mode == 1 else -1.0)
                for i, r in enumerate(rects)]
        m = dict(ora.step(gray, f, dets))
        out.append((m, dict(ora.preds), ora.track_rows()))
    return out


def test_oracle_meets_the_conditions():
    """CPU only: the inputs exercise what the GPU comparison is about."""
    check_conditions()


@functools.lru_cache(maxsize=None)
def check_conditions():
    for case in CASES:
        counts = [len(r) for _, r, _ in oracle_front(case)]
        assert min(counts) >= 8, (case, counts)
    for case, mode, thr in RUNS:
        if thr < 0:
            m, _, rows = oracle_run(case, mode, thr)[-1]
            assert len(rows) >= 10 and m["klt_predicted"] >= 10, (case, mode, m)
    a = [m["ntracks"] for m, _, _ in oracle_run("plain", 0, 0.2)]
    b = [m["ntracks"] for m, _, _ in oracle_run("plain", 1, 0.2)]
    assert a != b, (a, b)


def gpu_hog(gpu):
    from opencv_amd import hog as Hg

    hg = Hg.HOG.create((48, 96), ctx=gpu)
    hg.setSVMDetector(hg.getDefaultPeopleDetector())
    hg.setNumLevels(NLEVELS)
    hg.setHitThreshold(HIT)
    hg.setScaleFactor(SCALE0)
    hg.setGroupThreshold(GROUP)
    return hg


def gpu_loop(gpu, thr):
    from opencv_amd import tbd

    cfg = tbd.default_config(W, H, bounds_xmin=BOUNDS[0], bounds_xmax=BOUNDS[1], bounds_ymin=BOUNDS[2],
                             bounds_ymax=BOUNDS[3], track_confidence_threshold=thr)
    return tbd.TbdLoop(cfg, ctx=gpu)


def gpu_rows(tracks):
    return [(t["id"], t["x"], t["y"], t["width"], t["height"], t["pred_x"], t["pred_y"], t["pred_w"],
             t["pred_h"], t["age"], t["total_visible"], t["npoints"]) for t in tracks]


def metrics_of(m):
    return {k: getattr(m, k) for k in METRIC_KEYS}


pytestmark_gpu = pytest.mark.gpu


@pytestmark_gpu
@pytest.mark.parametrize("case,mode,thr", RUNS)
def test_step_image_equals_oracle_pipeline(gpu, case, mode, thr):
    check_conditions()  # on the oracle alone, before anything is compared with the GPU
    size, make_gray = CASES[case]
    loop = gpu_loop(gpu, thr)
    loop.attach_detector(gpu_hog(gpu), src_size=size, make_gray=make_gray, confidence_mode=mode)
    front, ref = oracle_front(case), oracle_run(case, mode, thr)
    for f, bgr in enumerate(bgr_frames(size)):
        m, dets = loop.step_image(torch.from_numpy(bgr).cuda(), f)
        _, rects, wts = front[f]
        # (a) the detections, in the detector's output order
        got = np.stack([dets["x"], dets["y"], dets["width"], dets["height"]], 1) if len(dets) else np.zeros((0, 4))
        assert np.array_equal(got, rects), f"frame {f}: rects differ"
        assert (dets["id"] == -1).all()
        want_conf = wts if mode == 1 else np.full(len(rects), -1.0)
        assert np.array_equal(dets["confidence"], want_conf), f"frame {f}: confidences differ"
        # (b) the loop
        om, op, orows = ref[f]
        assert metrics_of(m) == om, f"frame {f}: metrics {metrics_of(m)} vs oracle {om}"
        gp = loop.predictions()
        assert gp.keys() == op.keys(), f"frame {f}: predicted tracks differ"
        for k, (cx, cy) in gp.items():
            assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= 1e-4, f"frame {f} track {k}"
        assert gpu_rows(loop.tracks()) == orows, f"frame {f}: tracks differ"


@pytestmark_gpu
def test_confidence_modes_differ_at_the_default_threshold(gpu):
    """The reference quirk on the GPU itself: with the sample's -1.0 confidence
    every detected track is dropped again; the HOG weights keep some."""
    counts = []
    for mode in (0, 1):
        loop = gpu_loop(gpu, 0.2)
        loop.attach_detector(gpu_hog(gpu), confidence_mode=mode)
        counts.append([loop.step_image(torch.from_numpy(b).cuda(), f)[0].ntracks
                       for f, b in enumerate(bgr_frames((320, 240)))])
    assert counts[0] != counts[1], counts
    assert counts[0] == [m["ntracks"] for m, _, _ in oracle_run("plain", 0, 0.2)]
    assert counts[1] == [m["ntracks"] for m, _, _ in oracle_run("plain", 1, 0.2)]


@pytestmark_gpu
@pytest.mark.parametrize("case", ["resized", "colour"])
def test_step_image_equals_the_public_calls(gpu, case):
    """step_image == cvt_color -> resize_linear -> HOG.detectMultiScale -> TbdLoop.step."""
    from opencv_amd import klt, tbd

    size, make_gray = CASES[case]
    hg = gpu_hog(gpu)
    a, b = gpu_loop(gpu, -1.0), gpu_loop(gpu, -1.0)
    a.attach_detector(hg, src_size=size, make_gray=make_gray, confidence_mode=1)
    for f, bgr in enumerate(bgr_frames(size)):
        d = torch.from_numpy(bgr).cuda()
        ma, dets = a.step_image(d, f)
        if make_gray:
            gray = klt.resize_linear(klt.cvt_color(d, klt.COLOR_BGR2GRAY, ctx=gpu), (W, H), ctx=gpu)
            img = gray
        else:
            img = klt.resize_linear(d, (W, H), ctx=gpu)
            gray = klt.cvt_color(img, klt.COLOR_BGR2GRAY, ctx=gpu)
        rects, wts = hg.detectMultiScale(img, confidences=True)
        mine = np.zeros(len(rects), tbd.DET_DTYPE)
        mine["id"] = -1
        for i, (r, w) in enumerate(zip(rects, wts)):
            mine[i]["x"], mine[i]["y"], mine[i]["width"], mine[i]["height"] = r
            mine[i]["confidence"] = w
        assert np.array_equal(dets, mine), f"frame {f}: detections differ"
        mb = b.step(gray, f, mine)
        assert metrics_of(ma) == metrics_of(mb), f"frame {f}"
        pa, pb = a.predictions(), b.predictions()
        assert pa.keys() == pb.keys(), f"frame {f}"
        assert all(max(abs(pa[k][0] - pb[k][0]), abs(pa[k][1] - pb[k][1])) <= 1e-4 for k in pa), f"frame {f}"
        assert gpu_rows(a.tracks()) == gpu_rows(b.tracks()), f"frame {f}"


def write_p6(path, bgr, comment=False):
    h, w = bgr.shape[:2]
    with open(path, "wb") as fh:
        fh.write(b"P6\n" + (b"# a frame\n" if comment else b"") + f"{w} {h}\n255\n".encode())
        fh.write(np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())  # P6 is R, G, B


@pytestmark_gpu
def test_run_app_images_equals_step_image(gpu, tmp_path):
    from opencv_amd import _lib, tbd

    frames = bgr_frames((320, 240))
    names = []
    for f, bgr in enumerate(frames):
        names.append(f"f{f:03d}.ppm")
        write_p6(tmp_path / names[-1], bgr, comment=f == 1)
    lst = tmp_path / "frames.txt"
    lst.write_text("\n".join(names) + "\n")
    out_app, out_py = tmp_path / "app.txt", tmp_path / "py.txt"
    hg = gpu_hog(gpu)
    r = tbd.run_app_images(lst, hg, tracking_filepath=out_app, num_tracking_frames=NF, confidence_mode=1,
                           track_confidence_threshold=-1.0, bounds_xmin=BOUNDS[0], bounds_xmax=BOUNDS[1],
                           bounds_ymin=BOUNDS[2], bounds_ymax=BOUNDS[3])
    loop = gpu_loop(gpu, -1.0)
    loop.set_trajectories(tbd.Trajectories())
    loop.attach_detector(hg, confidence_mode=1)
    ndet = sum(len(loop.step_image(torch.from_numpy(b).cuda(), f)[1]) for f, b in enumerate(frames))
    loop.write_tracking_output(NF, path=out_py)
    assert r["frames"] == NF and r["detections"] == ndet
    assert out_app.read_bytes() == out_py.read_bytes() and out_app.stat().st_size > 0
    # a missing file anywhere in the list: an error before anything runs, nothing written
    bad = tmp_path / "bad.txt"
    bad.write_text("\n".join(names[:3] + ["missing.ppm"]) + "\n")
    out_bad = tmp_path / "bad_out.txt"
    with pytest.raises(_lib.TbdkError):
        tbd.run_app_images(bad, hg, tracking_filepath=out_bad, num_tracking_frames=NF)
    assert not out_bad.exists()
    # a truncated frame is refused the same way
    (tmp_path / "short.ppm").write_bytes((tmp_path / names[0]).read_bytes()[:-5])
    bad.write_text("\n".join(names[:2] + ["short.ppm"]) + "\n")
    with pytest.raises(_lib.TbdkError):
        tbd.run_app_images(bad, hg, tracking_filepath=out_bad, num_tracking_frames=NF)
    assert not out_bad.exists()
