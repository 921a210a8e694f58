"""CPU-only proof that the pictures of _extreme_cases.py do what
test_gpu_extreme.py relies on them for: they reach the ends of the value range,
overflow a 32-bit whole-window sum where stated, are singular where stated and
trackable where stated, tie enough corners to need the wide GFTT path, make
cubic interpolation saturate at both ends, and mark the finite domain of the
fp16 pixel path.  Oracles only, so a GPU comparison can never pass on a case
that turned out trivial.  The figures in the messages are the measured ones."""
import numpy as np
import pytest

import _extreme_cases as X
import _oracle as O

W, H = X.LK_SIZE
PAT = X.patterns(W, H)
GRID = X.grid(W, H) + np.float32(0.37)  # the 221 in-frame points the tracked shares are counted on


def _lk(a, b, win, maxlev, pts=GRID):
    return O.lk(O.Pyramid(a, (win, win), maxlev), O.Pyramid(b, (win, win), maxlev), pts, (win, win), maxlev,
                accum=O.ACCUM_EXACT)


@pytest.mark.parametrize("name", ["vstripe2", "hstripe2", "binary", "binblk", "quadrant"])
def test_scharr_reaches_both_ends(name):
    d = O.scharr(PAT[name]).astype(np.int32)
    assert d.max() == 4080 and d.min() == -4080, f"{name}: Scharr range {d.min()} .. {d.max()}"
    if name == "vstripe2":
        assert (np.abs(d[1:-1, 1:-1, 0]) == 4080).all() and not d[..., 1].any(), "vstripe2: |Ix| 4080, Iy 0 everywhere"
    if name == "hstripe2":
        assert (np.abs(d[1:-1, 1:-1, 1]) == 4080).all() and not d[..., 0].any(), "hstripe2: |Iy| 4080, Ix 0 everywhere"


def test_check1_has_no_derivative():
    assert PAT["check1"].min() == 0 and PAT["check1"].max() == 255
    assert not O.scharr(PAT["check1"])[1:-1, 1:-1].any(), "check1: Scharr is 0 in the interior"


def test_window_sums_against_int32():
    """which window sizes can catch a 32-bit whole-window sum"""
    ix = O.scharr(PAT["binary"])[..., 0].astype(np.int64)
    sq = np.pad((ix * ix).cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    sums = lambda n: sq[n:, n:] - sq[:-n, n:] - sq[n:, :-n] + sq[:-n, :-n]  # noqa: E731  every n x n window
    s63, s21 = sums(63), sums(21)
    assert s63.min() > 2 ** 31, f"binary: 63x63 sums of Ix^2 {s63.min():.3e} .. {s63.max():.3e} (measured 1.47e10 .. 1.64e10)"
    # a 21x21 window stays below 2^31 but for a few of the densest ones, so only 63 is relied on
    assert s21.mean() < 2 ** 31 and (s21 > 2 ** 31).mean() < 0.01, \
        f"binary: 21x21 sums of Ix^2 mean {s21.mean():.3e}, max {s21.max():.3e} (measured mean 1.71e9, max 2.16e9)"


@pytest.mark.parametrize("win", [5, 21, 63])
@pytest.mark.parametrize("name", X.SINGULAR)
def test_singular_windows_give_status_0(name, win):
    pts = X.points(W, H)
    for kind in X.PAIRS:
        _, st, _, _ = _lk(PAT[name], X.pair(PAT[name], kind), win, 0, pts)
        assert not st.any(), f"{name}/{kind} win {win}: {int(st.sum())} of {len(st)} points tracked"


@pytest.mark.parametrize("win,maxlev", [(21, 2), (63, 0)])
@pytest.mark.parametrize("name", ["check2", "binblk", "binary"])
def test_shift_pairs_track(name, win, maxlev):
    nx, st, _, _ = _lk(PAT[name], X.pair(PAT[name], "shift"), win, maxlev)
    assert st.mean() >= 0.9, f"{name} win {win}: {int(st.sum())} of {len(st)} tracked (measured 219-221 of 221)"
    assert np.isfinite(nx[st == 1]).all()


@pytest.mark.parametrize("win,maxlev", [(21, 2), (63, 0)])
@pytest.mark.parametrize("name", ["check2", "binblk", "binary"])
def test_inverted_pairs_run_the_mismatch_loop(name, win, maxlev):
    nx, st, _, it = _lk(PAT[name], X.pair(PAT[name], "inverted"), win, maxlev)
    ok = (st == 1) & np.isfinite(nx).all(1)
    assert ok.mean() >= 0.8, f"{name} win {win}: {int(ok.sum())} of {len(st)} finite at status 1 (measured 202-221 of 221)"
    assert it[ok].mean() > 20, f"{name} win {win}: mean iterations {it[ok].mean():.1f} (measured 22-71)"


def test_window_63_error_sums_pass_2_to_the_24():
    """err is a float running sum of |J - I| (x32) in window order: exact up to
    2^24, rounded at every addition beyond.  A 31x31 window cannot get there
    (961 * 8160 = 7.8e6); a 63x63 one does on full-contrast mismatch, so only
    there can a kernel that adds the window in another order differ."""
    for name, kind in (("binblk", "inverted"), ("quadrant", "inverted"), ("impulse", "inverted")):
        _, st, err, _ = _lk(PAT[name], X.pair(PAT[name], kind), 63, 0, X.points(W, H))
        s = err[st == 1].astype(np.float64) * (32 * 63 * 63)
        assert (s > 2 ** 24).any(), f"{name}/{kind}: largest |J - I| sum {s.max():.3e}, 2^24 is 1.678e7"
    assert 31 * 31 * 8160 < 2 ** 24 < 63 * 63 * 8160


def test_check2_ties_more_corners_than_one_workgroup_holds():
    n = {k: len(O.gftt_ex(PAT[k], 100000, 0.01, 0.0)) for k in ("check2", "blocks", "binblk")}
    assert n["check2"] > 16384, f"check2: {n['check2']} corners (measured 18,096)"
    assert 0 < n["blocks"] < 16384 and 0 < n["binblk"] < 16384, f"{n} (measured 2,046 and 1,043)"
    c = O.gftt_ex(PAT["check2"], 100000, 0.01, 0.0).astype(int)
    v, cnt = np.unique(O.corner_response(PAT["check2"])[c[:, 1], c[:, 0]], return_counts=True)
    assert cnt.max() > 16384, f"check2: corner responses {v} occur {cnt} times (measured 18,092 exact ties)"


@pytest.mark.parametrize("name", X.SINGULAR)
def test_zero_response_pictures_have_no_corner(name):
    assert len(O.gftt_ex(PAT[name], 100000, 0.01, 0.0)) == 0, name


@pytest.mark.parametrize("name", ["binblk", "blocks", "vstripe2"])
def test_cubic_saturates_at_both_ends(name):
    src = X.patterns(*X.SMALL_SIZE)[name]
    c, s = 1.3 * np.cos(0.3), 1.3 * np.sin(0.3)
    M = np.array([[c, -s, 3.25], [s, c, -20.5]])
    out = O.warp_affine(src, M, (80, 50), O.INTER_CUBIC, O.BORDER_REFLECT_101)
    n0, n255 = int((out == 0).sum()), int((out == 255).sum())
    mid = out.size - n0 - n255
    assert min(n0, n255, mid) > 400, f"{name}: {n0} / {n255} / {mid} pixels at 0 / 255 / between " \
                                     f"(measured 1,033-1,413 / 1,031-1,720 / 958-1,936 of 4,000)"


@pytest.mark.parametrize("flags", [0, O.FARNEBACK_GAUSSIAN], ids=["box", "gauss"])
def test_farneback_on_extremes(flags):
    """finite everywhere; pure cancellation on stripes; a large flow on an inverted pair"""
    P = X.patterns(*X.SMALL_SIZE)
    box = flags == 0
    for name, a in P.items():
        for kind in X.PAIRS:
            f = O.farneback(a, X.pair(a, kind), levels=3, iterations=3, flags=flags, box_direct=box)
            assert np.isfinite(f).all(), f"{name}/{kind}: non-finite flow"
            if kind == "inverted" and name in ("blocks", "quadrant"):
                # quadrant carries the large-flow condition (55 .. 109 px); blocks gives whole pixels (3.1 .. 3.7)
                least = 10 if name == "quadrant" else 1
                assert np.abs(f).max() > least, f"{name}/inverted: max |flow| {np.abs(f).max():.1f} px"
    for name in ("vstripe2", "hstripe2"):
        f = np.abs(O.farneback(P[name], P[name], levels=3, iterations=3, flags=flags, box_direct=box))
        assert 0 < f.max() < 1e-6, f"{name}/same: max |flow| {f.max():.3e} (measured 6e-12 .. 7.9e-11)"


@pytest.mark.parametrize("top,finite", [(4094, True), (4095, False), (4096, False), (65504, False)])
def test_fp16_derivative_domain(top, finite):
    edge = np.zeros((16, 16), np.float16)
    edge[:, 8:] = top
    d = O.scharr16(edge).astype(np.float32)
    assert np.isfinite(d).all() == finite, f"top {top}: max |d| {np.abs(d).max()}"
    if finite:
        assert d.max() == 65504.0, f"top {top}: max {d.max()} (16 * 4094 = 65504, the largest finite fp16)"


def _lk16(top, f32=False):
    a, b = X.to_u16(PAT["binblk"], top), X.to_u16(X.pair(PAT["binblk"], "shift"), top)
    if not f32:
        a, b = a.astype(np.float16), b.astype(np.float16)
    Pa, Pb = O.Pyramid16(a, (21, 21), 2, f32=f32), O.Pyramid16(b, (21, 21), 2, f32=f32)
    return O.lk16(Pa, Pb, GRID, (21, 21), 2)


def test_fp16_lk_in_and_out_of_range():
    nx, st, _, _ = _lk16(4094)
    assert st.mean() >= 0.9 and np.isfinite(nx[st == 1]).all(), f"top 4094: {int(st.sum())} of {len(st)} (measured 221)"
    nx, st, _, _ = _lk16(4095)
    bad = (st == 1) & ~np.isfinite(nx).all(1)
    assert not bad.any(), f"top 4095: {int(bad.sum())} points at status 1 with a non-finite position"
    assert st.sum() == 0, f"top 4095: {int(st.sum())} tracked (measured 0)"


def test_fp32_lk_at_16_bit_white():
    nx, st, _, _ = _lk16(65535, f32=True)
    assert st.mean() >= 0.9 and np.isfinite(nx[st == 1]).all(), f"{int(st.sum())} of {len(st)} (measured 221 of 221)"
