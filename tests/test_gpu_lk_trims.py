"""The several-points-per-wave PyrLK kernel's trimmed per-step and per-level work
against the exact-order oracle, bit for bit on nextPts, status, err and iters:
the border masks of the Scharr-on-the-fly setup taken only by waves with a
window over a level's edge, the single-precision stopping tests, and the b sums
without the per-step idle-lane select (plain-scan and lo/hi-split paths, with
and without the one-point steps)."""
import numpy as np
import pytest
import torch

import _oracle as O

pytestmark = pytest.mark.gpu


def klt():
    from opencv_amd import klt as K

    return K


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def textured_pair(w, h, seed):
    """a smooth random texture and the same moved by (1.3, -0.8) px roughly (an
    integer roll of a 2x finer texture, box-filtered), with a little noise"""
    rng = np.random.default_rng(seed)
    fine = rng.integers(0, 256, (2 * h + 8, 2 * w + 8)).astype(np.float32)
    k = np.ones(5, np.float32) / 5
    for ax in (0, 1):
        fine = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), ax, fine)
    fine = (fine - fine.min()) / (fine.max() - fine.min()) * 255

    def down(f):
        return f.reshape(f.shape[0] // 2, 2, f.shape[1] // 2, 2).mean((1, 3))

    a = down(fine)[2:2 + h, 2:2 + w]
    b = down(np.roll(fine, (-2, 3), (0, 1)))[2:2 + h, 2:2 + w] + rng.normal(0, 1.0, (h, w))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8), np.clip(np.rint(b), 0, 255).astype(np.uint8)


def crosses(pts, win, level, w, h):
    """the kernel's rule for the masked setup: the window of derivative rows
    ipy .. ipy + win and columns ipx .. ipx + win leaves the level"""
    half = np.float32((win - 1) * 0.5)
    sc = np.float32(1.0 / (1 << level))
    lw, lh = w, h
    for _ in range(level):
        lw, lh = (lw + 1) // 2, (lh + 1) // 2
    ipx = np.floor(pts[:, 0] * sc - half).astype(np.int64)
    ipy = np.floor(pts[:, 1] * sc - half).astype(np.int64)
    return (ipx < 0) | (ipx + win >= lw) | (ipy < 0) | (ipy + win >= lh)


def run(gpu, a, b, pts, win, maxlev, iters=30, eps=0.01, borrow=False):
    K = klt()
    h, w = a.shape
    lk = K.SparsePyrLKOpticalFlow((win, win), maxlev, iters, epsilon=eps, impl=3)
    Pa = K.Pyramid(gpu, w, h, maxlev, (win, win), derivs=False)
    Pb = K.Pyramid(gpu, w, h, maxlev, (win, win), derivs=False)
    fa, fb = to_dev(a), to_dev(b)
    if borrow:
        Pa.build_borrowed(fa)
        Pb.build_borrowed(fb)
    else:
        Pa.build(fa)
        Pb.build(fb)
    r = lk.calc(Pa, Pb, to_dev(pts), want_iters=True)
    torch.cuda.synchronize()
    return r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()


_ORACLE = {}


def oracle(key, a, b, pts, win, maxlev, iters=30, eps=0.01):
    """the exact-order oracle's result, computed once per case"""
    if key not in _ORACLE:
        Ra, Rb = O.Pyramid(a, (win, win), maxlev), O.Pyramid(b, (win, win), maxlev)
        _ORACLE[key] = O.lk(Ra, Rb, pts, (win, win), maxlev, iters, eps, 0, accum=O.ACCUM_EXACT)
    return _ORACLE[key]


def assert_exact(g, ex):
    nx, st, er, it = g
    assert np.array_equal(st, ex[1]), f"status mismatch at {np.flatnonzero(st != ex[1])[:10]}"
    ok = st == 1
    assert np.array_equal(nx[ok].view(np.uint32), ex[0][ok].view(np.uint32)), \
        f"next_pts mismatch at {np.flatnonzero((nx != ex[0]).any(1) & ok)[:10]}"
    assert np.array_equal(er[ok].view(np.uint32), ex[2][ok].view(np.uint32))
    assert np.array_equal(it, ex[3])


def border_points(win, w, h, maxlev):
    """A point list whose waves (64 // win consecutive points each) are of three
    kinds: every window interior at every level; exactly one point's window over
    the left / right / top / bottom edge of level 0 (such a window is over the
    edge of every coarser level as well: x - half < 0 implies x / 2^L - half < 0,
    and likewise on the far side), its wave's other windows interior everywhere;
    exactly one point's window over an edge at the top level only.  Returns the
    points and the kind of each wave (-1 where the geometry has no such wave:
    window 21 has no interior window on a 24 x 20 top level)."""
    P = 64 // win
    rng = np.random.default_rng(win * 1000 + w)
    cand = rng.uniform([0, 0], [w - 1, h - 1], (20000, 2)).astype(np.float32)
    c0 = crosses(cand, win, 0, w, h)
    ctop = crosses(cand, win, maxlev, w, h)
    cany = np.zeros(len(cand), bool)
    for lv in range(maxlev + 1):
        cany |= crosses(cand, win, lv, w, h)
    half = (win - 1) * 0.5
    interior = cand[~cany]
    top_only = cand[ctop & ~c0 & ~crosses(cand, win, 1, w, h)] if maxlev >= 2 else cand[:0]
    sides = [cand[c0 & (cand[:, 0] - half < 0)], cand[c0 & (cand[:, 0] + half + 1 >= w)],
             cand[c0 & (cand[:, 1] - half < 0)], cand[c0 & (cand[:, 1] + half + 1 >= h)]]
    # where no window is interior at every level, the other points of a wave are
    # the ones interior at level 0
    rest = interior if len(interior) >= 4 * P else cand[~c0]
    waves, kinds, it = [], [], 0

    def fill(special, kind, slot):
        nonlocal it
        wv = [rest[(it + j) % len(rest)] for j in range(P)]
        it += P
        if special is not None:
            wv[slot % P] = special
        waves.append(np.stack(wv))
        kinds.append(kind)

    for j in range(6):
        fill(None, 0 if len(interior) >= 4 * P else -1, 0)
    for s, side in enumerate(sides):
        for j in range(3):
            fill(side[j], 1, s + j)
    for j in range(min(6, len(top_only))):
        fill(top_only[j], 2 if len(interior) >= 4 * P else -1, j)
    return np.concatenate(waves).astype(np.float32), np.array(kinds)


@pytest.mark.parametrize("win,size", [(21, (96, 80)), (7, (96, 80)), (21, (384, 320))])
@pytest.mark.parametrize("borrow", [False, True], ids=["padded", "borrowed"])
def test_border_masks_only_where_needed(gpu, win, size, borrow):
    """Case 1: a 96 x 80 textured pair, 3 levels, windows 21 and 7, one launch
    holding waves with every window interior, waves with one window over an edge
    of level 0, and waves with one window over an edge of the top level only; on
    a padded pyramid and on a borrowed level 0.  Window 21 cannot be interior on
    the 24 x 20 top level of that pair (every wave is masked there, and level 0
    has both kinds), so it also runs on a 384 x 320 pair where all three kinds
    exist."""
    w, h = size
    a, b = textured_pair(w, h, 7)
    pts, kinds = border_points(win, w, h, 2)
    if (win, size) != (21, (96, 80)):
        assert {0, 1, 2} <= set(kinds.tolist())
    P = 64 // win
    c0 = crosses(pts, win, 0, w, h).reshape(-1, P)
    assert (c0.sum(1)[kinds == 1] == 1).all() and (c0.sum(1)[kinds != 1] == 0).all()
    ex = oracle(("border", win, size), a, b, pts, win, 2)
    g = run(gpu, a, b, pts, win, 2, borrow=borrow)
    assert_exact(g, ex)
    assert (g[1] == 1).mean() > 0.5


@pytest.mark.parametrize("eps", [0.0, 1e-6, 0.01, 0.5])
@pytest.mark.parametrize("iters", [1, 30])
def test_stopping_criteria(gpu, eps, iters):
    """Case 2: the same pair with criteria epsilon in {0, 1e-6, 0.01, 0.5} and
    maxCount in {1, 30} (epsilon 0 and 1e-6 lie outside the single-precision
    prefilter's range or near its floor: every step there takes the double
    expression)"""
    a, b = textured_pair(96, 80, 7)
    ys, xs = np.mgrid[3:78:5, 3:94:5]
    pts = (np.stack([xs.ravel(), ys.ravel()], 1) + np.float32([0.31, 0.57])).astype(np.float32)
    for win in (21, 7):
        ex = oracle(("stop", win, eps, iters), a, b, pts, win, 2, iters, eps)
        assert_exact(run(gpu, a, b, pts, win, 2, iters, eps), ex)


@pytest.mark.parametrize("solo", [4, 2])
def test_b_sums_split_and_plain(gpu, solo):
    """Case 3: a saturated 0/255 checkerboard pair (2 px cells), whose per-lane
    b partials pass 2^26 (the lo/hi-split sums), and a low-contrast pair (values
    100..110, the plain scans), with the default hand-over to the one-point steps
    and with lk_solo 2, so that one-point steps run on both.  (Every step keeps
    seg_sum_exact's range test; a per-level no-check flag is not built: DESIGN.md
    section 3, round 7.)"""
    yy, xx = np.mgrid[0:80, 0:96]
    chk = (((yy // 2 + xx // 2) & 1) * 255).astype(np.uint8)
    rng = np.random.default_rng(11)
    chk_b = np.roll(chk, (1, 0), (0, 1))
    chk_b[rng.random(chk_b.shape) < 0.05] ^= 255
    la, lb = textured_pair(96, 80, 9)
    low_a = (100 + la.astype(np.int32) * 10 // 255).astype(np.uint8)
    low_b = (100 + lb.astype(np.int32) * 10 // 255).astype(np.uint8)
    assert low_a.min() >= 100 and low_a.max() <= 110
    ys, xs = np.mgrid[2:79:4, 2:95:4]
    pts = (np.stack([xs.ravel(), ys.ravel()], 1) + np.float32([0.43, 0.27])).astype(np.float32)
    gpu.set_option("lk_solo", solo)
    try:
        for name, (a, b) in (("checker", (chk, chk_b)), ("low", (low_a, low_b))):
            for win in (21, 7):
                ex = oracle((name, win), a, b, pts, win, 2)
                assert_exact(run(gpu, a, b, pts, win, 2), ex)
    finally:
        gpu.set_option("lk_solo", 4)
