"""tbdk_find_homography on the GPU (libtbdk homography.hip) against the numpy
restatement of cv::findHomography (tests/_homography_oracle.py) and the recorded
reference (tests/golden/reference_homography.npz), under the numerics contract of
DESIGN.md §5 "findHomography":

A. bit for bit: valid, npoints, ninliers, iters, the whole mask, and the H that
   refine = 0 returns (the RANSAC model re-fitted on the inliers, or the method-0
   / 4-point fit);
B. iters rests on one margin, asserted in tests/test_homography_oracle.py: no
   niters update of a committed case is within 1e-6 of a rounding tie;
C. the refined H by what it does to the set's inlier points, within BAR_PX
   (tests/test_homography_oracle.py, where the bar is derived)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _homography_cases as HC
import _homography_oracle as HO
from test_homography_oracle import BAR_PX

pytestmark = pytest.mark.gpu


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(gpu, src, dst, st=None, offsets=None, **kw):
    from opencv_amd import klt

    r = klt.find_homography(d(src.reshape(-1, 2)), d(dst.reshape(-1, 2)), status=None if st is None else d(st),
                            offsets=None if offsets is None else d(np.asarray(offsets, np.int32)), ctx=gpu, **kw)
    torch.cuda.synchronize()
    return r


def fields(r, k=0):
    return tuple(int(t[k]) for t in (r.valid, r.npoints, r.ninliers, r.iters))


def case_kw(i):
    src, dst, st, method, thr, iters, conf = HC.fixture_inputs(HO.fixture(), i)
    return src, dst, st, dict(method=method, ransacReprojThreshold=thr, maxIters=iters, confidence=conf)


def full_mask(st, mask, n):
    """the restatement's mask over the compacted pairs, spread over all n pairs"""
    if st is None:
        return mask
    out = np.zeros(n, np.uint8)
    out[st != 0] = mask
    return out


@pytest.mark.parametrize("i", range(HC.NCASES))
def test_case_equals_restatement_and_recording(gpu, i):
    src, dst, st, kw = case_kw(i)
    want = HO.table_result(i)
    s, _ = HC.compact(src, dst, st)
    valid, nin, fmask, fh, _ = HC.fixture_outputs(HO.fixture(), i, len(s))
    for refine in (False, True):
        r = run(gpu, src, dst, st, refine=refine, **kw)
        assert fields(r) == (want.valid, len(s), want.ninliers, want.iters), (HC.label(i), refine)
        assert fields(r)[::2] == (valid, nin)
        got_mask = r.mask.cpu().numpy()
        assert np.array_equal(got_mask, full_mask(st, want.mask, len(src))), (HC.label(i), refine)
        assert np.array_equal(got_mask, full_mask(st, fmask, len(src)))
        H = r.H[0].cpu().numpy()
        if not refine:  # contract A
            assert H.tobytes() == np.array(want.H0, np.float64).tobytes(), HC.label(i)
        elif want.valid:  # contract C
            inl = s[want.mask != 0]
            dr, df = HO.distance(H, want.H, inl), HO.distance(H, fh, inl)
            print(f"{HC.label(i)}: d(device, restatement) = {dr:.3g} px, d(device, noavx2) = {df:.3g} px")
            assert dr <= BAR_PX and df <= BAR_PX
            if len(s) == 4:  # the reference exposes the un-refined H here: its bits
                assert H.tobytes() == fh.tobytes()
        else:
            assert np.array_equal(H, np.eye(3))


def test_one_launch_of_six_sets_equals_six_launches(gpu):
    idx = [HC.label(i) for i in range(HC.NCASES)]
    ids = [idx.index(f"size {n}") for n in (0, 3, 4, 65, 200, 1000)]
    sets = [case_kw(i)[:2] for i in ids]
    offs = np.cumsum([0] + [len(s) for s, _ in sets])
    src, dst = np.concatenate([s for s, _ in sets]), np.concatenate([q for _, q in sets])
    r = run(gpu, src, dst, offsets=offs)
    raw, mask = r.raw.cpu().numpy().reshape(6, -1), r.mask.cpu().numpy()
    for k, (s, q) in enumerate(sets):
        one = run(gpu, s, q)
        assert np.array_equal(one.raw.cpu().numpy(), raw[k]), ids[k]
        assert np.array_equal(one.mask.cpu().numpy(), mask[offs[k]:offs[k + 1]]), ids[k]
        assert fields(r, k) == fields(one)


def test_64_copies_of_one_set_are_equal(gpu):
    i = [HC.label(k) for k in range(HC.NCASES)].index("size 200")
    src, dst, _, kw = case_kw(i)
    r = run(gpu, np.tile(src, (64, 1)), np.tile(dst, (64, 1)), offsets=np.arange(65) * len(src), **kw)
    raw, mask = r.raw.cpu().numpy().reshape(64, -1), r.mask.cpu().numpy().reshape(64, -1)
    assert (raw == raw[0]).all() and (mask == mask[0]).all()
    want = HO.table_result(i)
    assert fields(r, 63) == (1, len(src), want.ninliers, want.iters) and np.array_equal(mask[63], want.mask)


def test_the_cap_is_reported_never_truncated(gpu):
    from opencv_amd import _lib

    cap = 4096
    src, dst = HC.points("plane", cap + 1, 30, "mild", 31)
    st = np.ones(cap + 1, np.uint8)
    r = run(gpu, src, dst, st, maxIters=50)
    assert fields(r) == (0, -1, 0, 0) and not r.mask.any() and np.array_equal(r.H[0].cpu().numpy(), np.eye(3))
    st[7] = 0  # exactly the cap, through the compaction
    r = run(gpu, src, dst, st, maxIters=50, refine=False)
    k = st != 0
    want = HO.find_homography(src[k], dst[k], HC.RANSAC, 3.0, 50, 0.995, refine=False)
    assert fields(r) == (1, cap, want.ninliers, want.iters)
    assert np.array_equal(r.mask.cpu().numpy(), full_mask(st, want.mask, cap + 1))
    assert r.H[0].cpu().numpy().tobytes() == np.array(want.H0).tobytes()
    assert C.sizeof(_lib.Homography) == 88


def test_parameters_out_of_range(gpu):
    from opencv_amd import _lib, klt

    src, dst = HC.points("plane", 20, 0, "mild", 5)
    for kw in (dict(method=4), dict(method=16), dict(maxIters=0), dict(maxIters=10001), dict(confidence=0.0),
               dict(confidence=1.0), dict(confidence=float("nan")), dict(ransacReprojThreshold=float("nan"))):
        with pytest.raises(_lib.TbdkError):
            klt.find_homography(d(src), d(dst), ctx=gpu, **kw)
    r = run(gpu, src[:0], dst[:0], offsets=[0])  # nsets == 0: a no-op
    assert r.H.shape == (0, 3, 3) and r.mask.numel() == 0
    r = run(gpu, src[:3], dst[:3], method=klt.LSQ)  # method 0 below four pairs: no result
    assert fields(r) == (0, 3, 0, 0)


def test_hostile_points_leave_the_kernel_bounded(gpu):
    # the sets tests/test_homography_core_host.py walks under the sanitizers; what H they give is unspecified
    src, dst = (a.copy() for a in case_kw([HC.label(k) for k in range(HC.NCASES)].index("size 200"))[:2])
    src[::7, 0], dst[3::11, 1], src[5::13, 1] = np.nan, np.inf, -np.inf
    for method in (HC.RANSAC, HC.LSQ):
        r = run(gpu, src, dst, method=method, maxIters=40)
        assert 0 <= fields(r)[3] <= 40 and fields(r)[1] == 200 and int(r.mask.max()) <= 1
