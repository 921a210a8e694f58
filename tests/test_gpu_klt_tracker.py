"""The device-resident KLT point tracker (tbdk_klt_tracker_*, opencv_amd.klt.KltTracker)
and tbdk_mask_circles_u8 against tests/_klt_tracker_oracle.py: ids, lengths and
counts equal, last points and whole histories equal bit for bit, statistics equal,
after every step.  tests/test_klt_tracker_oracle.py checks on the CPU that the
cases exercise what they are meant to."""
import ctypes as C

import numpy as np
import pytest

import _klt_tracker_oracle as KO

pytestmark = pytest.mark.gpu


def klt():
    from opencv_amd import klt as K

    return K


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tracker(gpu, w, h, **cfg):
    return klt().KltTracker(ctx=gpu, width=w, height=h, **cfg)


def assert_state(t, want_state, want_stats, what=""):
    """the tracker's read() against an oracle state() and Stats"""
    s = t.read()
    ids, last, lens, hist = want_state
    assert s.stats == want_stats._asdict(), (what, s.stats, want_stats)
    assert np.array_equal(s.ids, ids), what
    assert np.array_equal(s.lens, lens), what
    assert np.array_equal(s.last_pts.view(np.uint32), last.view(np.uint32)), what
    assert np.array_equal(s.hist.view(np.uint32), hist.view(np.uint32)), what
    return s


@pytest.mark.parametrize("cid", list(KO.CASES))
def test_cases_frame_by_frame(gpu, cid):
    case = KO.CASES[cid]
    fr = KO.frames(case.seq)
    ref = KO.run_case(case)
    d = dev(fr)
    t = tracker(gpu, fr.shape[2], fr.shape[1], **case.cfg)
    for f in range(case.nframes):
        t.step(d[f])
        assert_state(t, ref.states[f], ref.stats[f], f"{cid} frame {f}")
    tr = t.tracks()
    assert sorted(tr) == ref.states[-1][0].tolist()
    k = len(tr) // 2
    i = int(ref.states[-1][0][k])
    assert np.array_equal(tr[i], ref.states[-1][3][k, :ref.states[-1][2][k]])


def test_enqueued_without_reading(gpu):
    """all 13 steps enqueued, one read at the end: nothing depends on the host reading in between"""
    import torch

    case = KO.CASES["lk_track"]
    fr = KO.frames(case.seq)
    ref = KO.run_case(case)
    d = dev(fr)
    t = tracker(gpu, fr.shape[2], fr.shape[1], **case.cfg)
    for f in range(case.nframes):
        t.step(d[f])
    s = assert_state(t, ref.states[-1], ref.stats[-1])
    # the device views of the same state
    cnt, ids, last, lens, hist = t.device_state()
    torch.cuda.synchronize()
    n = int(cnt.cpu()[0])
    assert n == len(s.ids)
    assert np.array_equal(ids[:n].cpu().numpy(), s.ids) and np.array_equal(lens[:n].cpu().numpy(), s.lens)
    assert np.array_equal(last[:n].cpu().numpy(), s.last_pts) and np.array_equal(hist[:n].cpu().numpy(), s.hist)


@pytest.mark.parametrize("override", [dict(subpix_win=5), dict(mask_radius=-1), dict(mask_radius=0),
                                      dict(use_harris=1, block_size=5), dict(win=8, max_level=1)],
                         ids=["subpix5", "no_mask", "radius0", "harris_block5", "win8"])
def test_small_variants(gpu, override):
    case = KO.CASES["small"]
    fr = KO.frames(case.seq)
    ref = KO.run_case(case, **override)
    if "subpix_win" in override:  # the refinement moved the corners off the pixel grid
        assert any(np.any(st[3] != np.round(st[3])) for st in ref.states[:1])
    d = dev(fr)
    t = tracker(gpu, fr.shape[2], fr.shape[1], **dict(case.cfg, **override))
    for f in range(case.nframes):
        t.step(d[f])
        assert_state(t, ref.states[f], ref.stats[f], f"{override} frame {f}")


def test_detect_now_add_points_and_reset(gpu):
    """detect_now on a non-detection frame; add_points with points at the frame's
    corners, at (-0.7, 3.2) (truncates to (0, 3)) and outside the frame, before the
    first step and between steps; reset() and the same sequence again give the
    same states with ids restarting at 0"""
    case = KO.CASES["small"]
    fr = KO.frames(case.seq)
    h, w = fr.shape[1:]
    d = dev(fr)
    pts = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [-0.7, 3.2], [w + 80, 100], [-50, -50],
                    [100.25, 80.5], [200.5, 120.75]], np.float32)
    more = np.array([[60.5, 60.5], [-3.5, 100.0], [150.0, h + 2.5]], np.float32)
    o = KO.KltTracker(w, h, **case.cfg)
    t = tracker(gpu, w, h, **case.cfg)
    for rnd in range(2):
        o.add_points(pts)
        t.add_points(pts)
        for f in range(5):
            now = f in (1, 3)  # frame 1 and 3 are no detection frames at interval 2
            st = o.step(fr[f], detect_now=now)
            t.step(d[f], detect_now=now)
            if f == 1:
                assert st.detected > 0
            if f == 2:
                o.add_points(more)
                t.add_points(dev(more))
            assert_state(t, o.state(), o.stats, f"round {rnd} frame {f}")
        # the mask the first detection saw had the added points' discs cut out, (0, 3)'s included
        assert o.det_log[0][2] >= 5
        o.reset()
        t.reset()
        assert_state(t, o.state(), o.stats, "after reset")
        assert t.read().stats["next_id"] == 0 and t.read().stats["frame_idx"] == -1


def test_capacity_with_add_points(gpu):
    """add_points beyond max_tracks: the first that fit are appended, the rest dropped"""
    w, h = 64, 48
    o = KO.KltTracker(w, h, max_tracks=10, max_corners=10, win=9)
    t = tracker(gpu, w, h, max_tracks=10, max_corners=10, win=9)
    rng = np.random.default_rng(5)
    for n in (7, 7, 3):
        p = rng.uniform(0, 40, (n, 2)).astype(np.float32)
        o.add_points(p)
        t.add_points(p)
        assert_state(t, o.state(), o.stats, f"add {n}")
    assert o.stats.dropped == 7 and len(o.ids) == 10


def run_pair(gpu, frames, **cfg):
    h, w = frames.shape[1:]
    o = KO.KltTracker(w, h, **cfg)
    t = tracker(gpu, w, h, **cfg)
    d = dev(frames)
    out = []
    for f in range(len(frames)):
        o.step(frames[f])
        t.step(d[f])
        assert_state(t, o.state(), o.stats, f"frame {f}")
        out.append(o.stats)
    return out


def test_constant_frame(gpu):
    """no corners: the count stays 0 and the PyrLK launches over a count of 0 do nothing"""
    st = run_pair(gpu, np.full((4, 48, 64), 77, np.uint8), detect_interval=1)
    assert all(s.detected == 0 and s.kept == 0 for s in st)


def test_small_frame_pyramid_stop_rule(gpu):
    """40 x 32 with window 9: the pyramid ends at level 1 though max_level is 2"""
    import _frontend_oracle as FO

    a = FO.pattern(40, 32, 1, 11).reshape(32, 40)
    fr = np.stack([a, np.roll(a, 1, 1), np.roll(a, (1, 1), (0, 1))]).astype(np.uint8)
    fr = np.stack([KO.O.pyr_down(np.kron(f, np.ones((2, 2), np.uint8))) for f in fr])  # smoothed: trackable
    assert fr.shape == (3, 32, 40)
    assert KO.O.Pyramid(fr[0], (9, 9), 2).nlevels == 2
    st = run_pair(gpu, fr, win=9, max_corners=40, quality_level=0.01, min_distance=2.0, block_size=3,
                  detect_interval=2, mask_radius=2, max_tracks=64)
    assert st[0].detected > 0


def test_unrelated_second_frame(gpu):
    """the second frame is unrelated noise: (nearly) everything is lost, then detected again"""
    import _frontend_oracle as FO

    case = KO.CASES["small"]
    fr = KO.frames(case.seq)[:3].copy()
    fr[1] = FO.pattern(fr.shape[2], fr.shape[1], 1, 99).reshape(fr.shape[1:])
    fr[2] = fr[1]
    st = run_pair(gpu, fr, **dict(case.cfg, detect_interval=1))
    assert st[1].kept <= st[1].tracks_in // 10 and st[1].detected > 0 and st[2].kept > 0


def mask_points(rng, w, h, n):
    p = np.concatenate([rng.uniform([-80, -80], [w + 80, h + 80], (n - 12, 2)),
                        [[-0.7, 3.2], [0, 0], [w - 1, h - 1], [w - 0.01, h - 0.01], [-1.0, -1.0], [-0.99, 5.99],
                         [1e6, 10], [10, -1e6], [3e9, 3e9], [np.nan, 5], [np.inf, 5], [w / 2, h / 2]]])
    return p.astype(np.float32)


@pytest.mark.parametrize("w,h", [(64, 48), (333, 251)])
@pytest.mark.parametrize("radius", [0, 1, 5, 9, 64])
def test_mask_circles(gpu, w, h, radius):
    """500 points, negative, fractional and far outside ones included; a pitch
    larger than the width (padding untouched); a device count smaller than n"""
    import torch

    K = klt()
    rng = np.random.default_rng(1000 * radius + w)
    pts = mask_points(rng, w, h, 500)
    for value, count in ((0, None), (7, 123)):
        buf = torch.full((h, w + 29), 200, dtype=torch.uint8, device="cuda")
        m = buf[:, 3:3 + w]
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
        K.mask_circles(m, dev(pts), radius, value, count=cnt, ctx=gpu)
        torch.cuda.synchronize()
        want = np.full((h, w + 29), 200, np.uint8)
        KO.draw_discs(want[:, 3:3 + w], pts[:count], radius, value)
        assert np.array_equal(buf.cpu().numpy(), want), (value, count)
        assert (want[:, 3:3 + w] == value).any()


def test_einval(gpu):
    K = klt()
    from opencv_amd import _lib

    bad = [dict(track_len=0), dict(track_len=65), dict(detect_interval=0), dict(mask_radius=65),
           dict(max_corners=200, max_tracks=100), dict(max_tracks=0), dict(max_tracks=65537),
           dict(win=2), dict(win=64), dict(max_level=-1), dict(back_threshold=0.0),  # tbdk_lk_sparse_fb's
           dict(max_corners=0), dict(quality_level=0.0), dict(min_distance=-1.0), dict(block_size=0),
           dict(block_size=64), dict(use_harris=2),  # tbdk_gftt_rois_masked's
           dict(subpix_win=16), dict(subpix_win=-1), dict(subpix_win=15, width=34, height=48),  # tbdk_corner_sub_pix's
           dict(width=0)]
    for kw in bad:
        with pytest.raises(_lib.TbdkError):
            tracker(gpu, kw.pop("width", 64), kw.pop("height", 48), **kw)
    # step: a refusal enqueues nothing and leaves the state as it was
    case = KO.CASES["small"]
    fr = KO.frames(case.seq)
    ref = KO.run_case(case)
    d = dev(fr)
    t = tracker(gpu, fr.shape[2], fr.shape[1], **case.cfg)
    t.step(d[0])
    lib, hnd = gpu.lib, t.handle
    ptr = C.c_void_p(d[1].data_ptr())
    assert lib.tbdk_klt_tracker_step(hnd, None, 320, 0, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_klt_tracker_step(hnd, ptr, 319, 0, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_klt_tracker_step(hnd, ptr, 320, 2, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_klt_tracker_add_points(hnd, None, 3, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_klt_tracker_add_points(hnd, ptr, -1, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_klt_tracker_read(hnd, None, None, None, None, -1, None, None) == _lib.TBDK_EINVAL
    with pytest.raises(_lib.TbdkError):
        t.step(d[1][:, :300])
    for r in (-1, 65):
        with pytest.raises(_lib.TbdkError):
            K.mask_circles(d[0].clone(), dev(np.zeros((2, 2), np.float32)), r, ctx=gpu)
    assert_state(t, ref.states[0], ref.stats[0], "after the refusals")
    t.step(d[1])
    assert_state(t, ref.states[1], ref.stats[1], "the step after the refusals")


def test_more_tracks_than_one_tile(gpu):
    """2,500 added points plus a detection, at the largest capacity and history
    length: the compaction's carried prefix over three 1024-wide tiles with losses
    in each, and an append of more than 1024 points"""
    case = KO.CASES["small"]
    fr = KO.frames(case.seq)[:4]
    h, w = fr.shape[1:]
    rng = np.random.default_rng(77)
    pts = rng.uniform([-4, -4], [w + 4, h + 4], (2500, 2)).astype(np.float32)
    cfg = dict(case.cfg, max_tracks=65536, track_len=64, detect_interval=100)
    o = KO.KltTracker(w, h, **cfg)
    t = tracker(gpu, w, h, **cfg)
    d = dev(fr)
    o.add_points(pts)
    t.add_points(pts)
    lost = []
    for f in range(4):
        o.step(fr[f])
        t.step(d[f])
        assert_state(t, o.state(), o.stats, f"frame {f}")
        lost.append(o.stats.tracks_in - o.stats.kept)
        if f == 1:  # losses in every tile of the first tracked frame: ids below 1024, 1024..2047, from 2048 on
            gone = np.setdiff1d(np.arange(2560), o.state()[0])
            assert all(((gone >= a) & (gone < b)).sum() > 5 for a, b in ((0, 1024), (1024, 2048), (2048, 2560)))
    assert o.stats.kept > 2048 and all(n > 20 for n in lost[1:])


def test_timing_names(gpu):
    """the tracker's own launches are timed as klt_compact, klt_mask and klt_append"""
    case = KO.CASES["small"]
    fr = KO.frames(case.seq)
    d = dev(fr)
    t = tracker(gpu, fr.shape[2], fr.shape[1], **case.cfg)
    names = ["klt_compact", "klt_mask", "klt_append"]
    gpu.timing_select(names)
    gpu.timing_enable(True)
    try:
        before = {k: gpu.timing_calls(k) for k in names}
        for f in range(3):  # detections on frames 0 and 2
            t.step(d[f])
        t.read()
        after = {k: gpu.timing_calls(k) for k in names}
    finally:
        gpu.timing_enable(False)
        gpu.timing_select(None)
    assert {k: after[k] - before[k] for k in names} == {"klt_compact": 3, "klt_mask": 2, "klt_append": 2}
