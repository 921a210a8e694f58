"""tbdk_box_propagate_ransac vs the restatement of cv::estimateRigidTransform's
point-set branch (tests/_rigid_oracle.py, itself pinned to the real function by
tests/test_rigid_oracle.py).

The consensus search is integer-valued apart from two kinds of floating-point
comparisons: the inlier test |residual| < thr and the collinearity test.  The
kernel solves the 3-point hypotheses in closed form, the restatement by an eigen
solve, so the two agree to double rounding (~1e-12 px at these coordinates);
the random-box tests first assert that in the restatement no residual comes
within 1e-4 px of the threshold and no collinearity comparison within 1e-9
relative, and then require valid, iters, npoints and the inlier mask to be
EXACT, M within 64 eps cond(A_inliers) max(1, |M|) and the centre within
1e-4 px."""
import numpy as np
import pytest
import torch

import _rigid_oracle as R
from _rigid_oracle import BF

pytestmark = pytest.mark.gpu

FRACTIONS = (0.0, 0.2, 0.4, 0.6, 0.9)

# Seeds chosen on the CPU, from the restatement alone, as the first for which the
# margins asserted in check() hold with a factor 2 to spare.  With ~10^6
# residuals per case the closest one is typically 1e-5..1e-4 px from the
# threshold, so most seeds miss the 1e-4 px margin (15 of the first 16 here).
SEED_RANDOM = 16   # margins 5.2e-4 px, 1.8e-3 relative; 28 of 48 boxes get a transform
SEED_BIG = 1       # 8.0e-2 px, 0.95
SEED_PARAMS = 2    # 1.8e-3 px, 4.0e-4; 8 / 20 of 24 boxes get a transform


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(gpu, prev, nxt, status, offsets, boxes, min_points=4, **kw):
    from opencv_amd import klt

    return klt.box_propagate_ransac(d(prev), d(nxt), None if status is None else d(status.astype(np.uint8)),
                                    d(np.asarray(offsets, np.int32)), d(np.asarray(boxes, np.int32).reshape(-1, 4)),
                                    min_points, ctx=gpu, **kw)


def make_box(rng, n, frac, shift=40.0):
    """n pairs under a true similarity + 0.3 px noise; a fraction frac moved by up to +-shift px"""
    x, y = rng.uniform(0, 1700), rng.uniform(0, 900)
    w, h = int(rng.integers(20, 220)), int(rng.integers(20, 220))
    a = np.stack([rng.uniform(x, x + w, n), rng.uniform(y, y + h, n)], 1)
    ang, s = rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.1)
    Rm = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    b = a @ Rm.T + rng.uniform(-8, 8, 2) + rng.normal(0, 0.3, (n, 2))
    out = rng.random(n) < frac
    b[out] += rng.uniform(-shift, shift, (int(out.sum()), 2))
    return a.astype(np.float32), b.astype(np.float32), (int(x), int(y), w, h)


def make_boxes(seed, nboxes, max_pts, masked=True):
    rng = np.random.default_rng(seed)
    prev, nxt, st, offs, boxes = [], [], [], [0], []
    for _ in range(nboxes):
        n = int(rng.integers(0, max_pts + 1))
        a, b, box = make_box(rng, n, FRACTIONS[int(rng.integers(0, len(FRACTIONS)))])
        prev.append(a)
        nxt.append(b)
        st.append((rng.random(n) > 0.15).astype(np.uint8) if masked else np.ones(n, np.uint8))
        offs.append(offs[-1] + n)
        boxes.append(box)
    return np.concatenate(prev), np.concatenate(nxt), np.concatenate(st), np.array(offs), boxes


def check(got, prev, nxt, st, offs, boxes, min_points, max_iters=500, good_ratio=0.5, margins=True):
    fit, iters, inl = got
    found = 0
    for i, box in enumerate(boxes):
        sl = slice(offs[i], offs[i + 1])
        sel = (st[sl] != 0) if st is not None else np.ones(offs[i + 1] - offs[i], bool)
        a, b = prev[sl][sel], nxt[sl][sel]
        r = R.estimate(a, b, max_iters, good_ratio)
        if margins:  # the precondition of an exact comparison (module docstring); asserted, never skipped
            assert r.resid_margin >= 1e-4, (i, r.resid_margin)
            assert r.collin_margin >= 1e-9, (i, r.collin_margin)
        want_mask = np.zeros(len(sel), np.uint8)
        want_mask[np.flatnonzero(sel)[r.inliers]] = 1
        assert iters[i] == r.k, (i, iters[i], r.k)
        assert np.array_equal(inl[sl], want_mask), i
        assert fit["npoints"][i] == int(r.inliers.sum()), i
        gm = fit["m"][i].reshape(2, 3)
        if not r.found:
            assert fit["valid"][i] == 0 and np.array_equal(gm, [[1, 0, 0], [0, 1, 0]]), (i, gm)
            continue
        found += 1
        cx, cy = BF.propagate_box(r.M, box)
        scale = np.hypot(r.M[0, 0], r.M[1, 0])
        want_valid = int(r.inliers.sum()) >= min_points and 0.5 < scale < 2.0
        assert bool(fit["valid"][i]) == want_valid, (i, scale)
        tol = R.tolerance(a[r.inliers], b[r.inliers], r.M)
        assert np.all(np.abs(gm - r.M) <= tol), (i, gm - r.M, tol)
        assert abs(fit["cx"][i] - cx) <= 1e-4 and abs(fit["cy"][i] - cy) <= 1e-4, i
    return found


def test_random_boxes_match_estimate_rigid_transform(gpu):
    # 48 boxes of 0..256 points, outlier fraction from {0, .2, .4, .6, .9}, status mask of 85 %
    prev, nxt, st, offs, boxes = make_boxes(SEED_RANDOM, 48, 256)
    found = check(run(gpu, prev, nxt, st, offs, boxes), prev, nxt, st, offs, boxes, 4)
    assert 20 <= found < 48  # both outcomes occur


def degenerate_sets():
    sets = []
    rng = np.random.default_rng(5)
    for n in range(8):  # n = 0..7, clean
        a, b, box = make_box(rng, n, 0.0)
        sets.append((a, b, box, 500))
    p = np.array([[120.5, 77.25]], np.float32)
    sets.append((np.repeat(p, 9, 0), np.repeat(p + 2, 9, 0), (100, 60, 40, 40), 8))  # all points equal
    t = np.arange(12, dtype=np.float32)[:, None]
    line = np.concatenate([100 + 4 * t, 50 + 2 * t], 1).astype(np.float32)
    sets.append((line, line + np.float32(3), (100, 50, 50, 30), 8))  # exactly collinear
    two = np.array([[10, 10], [90, 40]], np.float32)[np.arange(10) % 2]
    sets.append((two, two + np.float32(1), (10, 10, 80, 30), 8))  # two distinct points repeated
    return sets


def test_small_and_degenerate_sets(gpu):
    sets = degenerate_sets()
    for mi in (500, 8):
        grp = [s for s in sets if s[3] == mi]
        prev = np.concatenate([s[0] for s in grp])
        nxt = np.concatenate([s[1] for s in grp])
        offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in grp])])
        boxes = [s[2] for s in grp]
        got = run(gpu, prev, nxt, None, offs, boxes, max_iters=mi)
        check(got, prev, nxt, None, offs, boxes, 4, max_iters=mi, margins=(mi == 500))
        if mi == 8:  # the degenerate ones: no transform, as the restatement
            assert np.all(got[1] == -1) and not got[2].any() and not got[0]["valid"].any()
        else:
            assert np.all(got[1][:3] == -1)  # n = 0, 1, 2


def test_status_null_vs_mask_multichunk_and_overflow(gpu):
    rng = np.random.default_rng(SEED_BIG)
    a0, b0, box0 = make_box(rng, 600, 0.2)    # several 64-point chunks, > 256 pairs
    a1, b1, box1 = make_box(rng, 1100, 0.0)   # more than 1024 tracked pairs
    a2, b2, box2 = make_box(rng, 1100, 0.2)   # 1100 points, under the budget once masked
    prev, nxt = np.concatenate([a0, a1, a2]), np.concatenate([b0, b1, b2])
    offs = np.array([0, 600, 1700, 2800])
    boxes = [box0, box1, box2]
    st = (rng.random(2800) > 0.3).astype(np.uint8)
    st[600:1700] = 1
    assert st[1700:].sum() <= 1024
    # status == NULL: boxes 1 and 2 overflow; box 0 is checked against the restatement
    fit, iters, inl = run(gpu, prev, nxt, None, offs, boxes)
    assert list(fit["npoints"][1:]) == [-1, -1] and not fit["valid"][1:].any()
    assert list(iters[1:]) == [-1, -1] and not inl[600:].any()
    check((fit[:1], iters[:1], inl[:600]), prev[:600], nxt[:600], None, offs[:2], boxes[:1], 4)
    # with the mask: box 1 still overflows, boxes 0 and 2 equal the restatement on their status-1 pairs
    fit, iters, inl = run(gpu, prev, nxt, st, offs, boxes)
    assert fit["npoints"][1] == -1 and fit["valid"][1] == 0 and iters[1] == -1 and not inl[600:1700].any()
    assert np.array_equal(fit["m"][1], [1, 0, 0, 0, 1, 0])
    check((fit[:1], iters[:1], inl[:600]), prev[:600], nxt[:600], st[:600], offs[:2], boxes[:1], 4)
    check((fit[2:], iters[2:], inl[1700:]), prev[1700:], nxt[1700:], st[1700:], np.array([0, 1100]), boxes[2:], 4)
    assert fit["valid"][0] == 1 and fit["valid"][2] == 1


@pytest.mark.parametrize("max_iters,good_ratio", [(20, 0.8), (500, 0.3)])
def test_max_iters_and_good_ratio(gpu, max_iters, good_ratio):
    prev, nxt, st, offs, boxes = make_boxes(SEED_PARAMS, 24, 96)
    got = run(gpu, prev, nxt, st, offs, boxes, max_iters=max_iters, good_ratio=good_ratio)
    found = check(got, prev, nxt, st, offs, boxes, 4, max_iters, good_ratio)
    assert 0 < found < 24


def test_bad_parameters_are_einval(gpu):
    from opencv_amd import _lib

    prev, nxt, st, offs, boxes = make_boxes(3, 2, 8)
    for kw in ({"max_iters": 0}, {"max_iters": 10001}, {"max_iters": -5}, {"good_ratio": -0.01},
               {"good_ratio": 1.01}, {"good_ratio": float("nan")}):
        with pytest.raises(_lib.TbdkError, match="TBDK_EINVAL"):
            run(gpu, prev, nxt, st, offs, boxes, **kw)
    run(gpu, prev, nxt, st, offs, boxes, max_iters=1, good_ratio=0.0)  # the ends of the ranges are accepted
    run(gpu, prev, nxt, st, offs, boxes, max_iters=10000, good_ratio=1.0)


def test_outliers_drag_least_squares_but_not_ransac(gpu):
    # why it exists: 40 points under a pure translation, 8 of them shifted by 30 px
    from opencv_amd import klt

    rng = np.random.default_rng(11)
    box = (400, 300, 120, 160)
    a = np.stack([rng.uniform(400, 520, 40), rng.uniform(300, 460, 40)], 1).astype(np.float32)
    t = np.array([3.0, -2.0])
    b = (a + t + rng.normal(0, 0.05, (40, 2))).astype(np.float32)
    b[:8] += np.float32([30.0, 0.0])
    truth = np.array([400 + 60, 300 + 80]) + t
    offs = np.array([0, 40])
    fit, iters, inl = run(gpu, a, b, None, offs, [box])
    lsq = klt.box_propagate(d(a), d(b), None, d(offs.astype(np.int32)), d(np.asarray([box], np.int32)), 4, ctx=gpu)
    assert fit["valid"][0] == 1 and iters[0] >= 0 and not inl[:8].any() and inl[8:].all()
    err_ransac = np.hypot(fit["cx"][0] - truth[0], fit["cy"][0] - truth[1])
    err_lsq = np.hypot(lsq["cx"][0] - truth[0], lsq["cy"][0] - truth[1])
    print(f"centre error: RANSAC {err_ransac:.4f} px, least squares {err_lsq:.4f} px")
    assert err_ransac < 0.2
    assert err_lsq > 1.0
