"""CPU checks of tests/_klt_tracker_oracle.py, the reference of the KLT point
tracker's GPU tests: its circle restatement against the real cv::circle
(tests/golden/reference_circle.npz, recorded by tools/record_reference_cases.py),
and, from the oracle alone, the conditions that keep a case of
tests/test_gpu_klt_tracker.py from passing by doing nothing."""
import os

import numpy as np
import pytest

import _gftt_mask_oracle as GM
import _klt_tracker_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def circles():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_circle.npz"))


def test_fixture_cases(circles):
    """radii 0..16 at the centre; radius 5 and 9 at centres on, across and beyond every edge; both dispatch states"""
    assert str(circles["state"]) == "both"
    assert sum(1 for k in circles.files if k.endswith("_m")) == len(KO.CIRCLE_CASES) == 31
    assert [c[2] for c in KO.CIRCLE_CASES[:17]] == list(range(17))
    assert {c[:2] for c in KO.CIRCLE_CASES[17:]} == {(-3, 2), (0, 0), (47, 39), (53, 20), (20, -6), (-9, -9), (24, 45)}


def test_circle_restatement_equals_cv_circle(circles):
    w, h = KO.CIRCLE_SIZE
    for i, (cx, cy, r) in enumerate(KO.CIRCLE_CASES):
        want = np.unpackbits(circles[f"{i}_m"])[:w * h].reshape(h, w).astype(bool)
        # fractional parts that truncate toward zero to the recorded integer centre
        fx, fy = (cx + 0.75 if cx >= 0 else cx - 0.75), (cy + 0.5 if cy >= 0 else cy - 0.5)
        got = KO.draw_discs(np.full((h, w), 255, np.uint8), np.float32([[fx, fy]]), r) == 0
        assert np.array_equal(got, want), (cx, cy, r)
        if i < 17:
            assert want.any()
    assert KO.circle_half_widths(5).tolist() == [5, 4, 4, 4, 3, 0]


def test_truncation_toward_zero():
    assert KO.trunc_centres([[-0.7, 3.2], [-1.0, -1.99], [5.99, 0.0]]).tolist() == [[0, 3], [-1, -1], [5, 0]]


def test_half_widths_up_to_64():
    for r in range(65):
        hw = KO.circle_half_widths(r)
        assert hw[0] == r and hw[r] >= 0 and (np.diff(hw) <= 0).all()


def test_lk_track_case():
    case = KO.CASES["lk_track"]
    run = KO.run_case(case)
    det = {f: (n, clipped) for f, n, clipped in run.det_log}
    assert sorted(det) == [0, 5, 10] and all(n > 0 for n, _ in det.values())
    # the mask matters: without it frame 5 returns another number of corners
    fr = KO.frames(case.seq)
    c = KO.DEFAULTS
    unmasked = GM.gftt_masked(fr[5], None, c["max_corners"], c["quality_level"], c["min_distance"], c["block_size"])
    assert len(unmasked) != det[5][0]
    assert (run.masks[5] == 0).any() and run.masks[4] is None
    # the check drops points of all three kinds, and most points survive
    fwd, back, far, kept = np.array(run.log).sum(0)
    assert fwd > 0 and back > 0 and far > 0 and kept > 10 * (fwd + back + far)
    # tracks reach track_len and are trimmed: a track older than track_len frames holds track_len positions
    lens = run.states[-1][2]
    assert lens.max() == c["track_len"] and run.states[-1][0][lens == c["track_len"]].min() < det[0][0]
    assert case.nframes > c["track_len"] + 1
    # discs are clipped at the frame edge on the later detections
    assert det[5][1] > 0 and det[10][1] > 0
    # survivors keep their order, new ids follow
    for ids, *_ in run.states:
        assert (np.diff(ids) > 0).all()


def test_small_case():
    case = KO.CASES["small"]
    run = KO.run_case(case)
    assert [f for f, _, _ in run.det_log] == [0, 2, 4, 6, 8]
    assert all(n == case.cfg["max_corners"] for _, n, _ in run.det_log)
    fwd, back, far, kept = np.array(run.log).sum(0)
    assert fwd > 0 and back > 0 and far > 0 and kept > 0
    assert all(st[2].max() <= 3 for st in run.states) and (run.states[-1][2] == 3).sum() > 10
    # a trimmed history is the tail of the positions: it ends at the last point
    ids, last, lens, hist = run.states[-1]
    assert np.array_equal(hist[np.arange(len(ids)), lens - 1], last)


def test_cap_case():
    case = KO.CASES["cap"]
    run = KO.run_case(case)
    cap = case.cfg["max_tracks"]
    dropped = {s.frame_idx: s.dropped for s in run.stats}
    assert dropped[2] > 0 and dropped[4] > 0 and dropped[6] > 0 and dropped[0] == 0
    for s, st in zip(run.stats, run.states):
        assert len(st[0]) <= cap and s.detected == s.appended + s.dropped
        if s.dropped:
            assert len(st[0]) == cap
    assert run.stats[-1].next_id == sum(s.appended for s in run.stats)

