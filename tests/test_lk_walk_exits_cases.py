"""CPU companion of tests/test_gpu_lk_walk_exits.py: the oracle alone shows that
the inputs of tests/_lk_walk_cases.py send points through every way out of the
PyrLK level walk, for each pixel type and each flag setting, so the GPU
comparison holds the shared walk (opencv_amd/csrc/lk_walk.hpp) to all of them:
status 0 with no Newton step, status 0 after steps, status 1 after every step
of every level, status 1 after fewer."""
import numpy as np
import pytest

import _fb_oracle as F
import _lk_walk_cases as WC
import _oracle as O


def _status_iters(kind, flags):
    if kind == "fb":
        r = WC.ref_fb(flags)
        return r.fwd_status, r.iters
    r = {"gray": WC.ref_gray, "cn3": WC.ref_cn3, "u16_cn3": WC.ref_u16_cn3}[kind](flags)
    return r[1], r[3]


@pytest.mark.parametrize("flags", WC.FLAGS)
@pytest.mark.parametrize("kind", ["gray", "fb", "cn3", "u16_cn3"])
def test_every_exit_is_taken(kind, flags):
    st, it = _status_iters(kind, flags)
    e = WC.exits(st, it)
    print(kind, flags, e)
    assert all(v > 0 for v in e.values()), e
    assert it.max() == WC.FULL


@pytest.mark.parametrize("flags", WC.FLAGS)
def test_backward_pass_takes_its_exits(flags):
    """the backward kernel: points it skips (lost forward), loses itself, tracks
    back too far, and keeps"""
    fwd_lost, back_lost, too_far, kept = F.kinds(WC.ref_fb(flags))
    print(flags, fwd_lost, back_lost, too_far, kept)
    assert min(fwd_lost, back_lost, too_far, kept) > 0


def test_point_list():
    p = WC.points()
    assert 36 <= len(p) <= 64
    x, y = p[:, 0], p[:, 1]
    half = (WC.WIN - 1) / 2
    inside = (x >= 0) & (x < WC.W) & (y >= 0) & (y < WC.H)
    assert (~inside).sum() >= 4
    assert (inside & (x < half)).any() and (inside & (x >= WC.W - half)).any()
    assert (inside & (y < half)).any() and (inside & (y >= WC.H - half)).any()
    a, b = WC.gray_pair()
    assert a.shape == b.shape == (WC.H, WC.W) and np.ptp(a[WC.FLAT]) == 0 and np.ptp(b[WC.FLAT]) == 0
    for f in WC.cn3_pair() + WC.u16_cn3_pair():  # flat in every channel, away from the shifted copies' seam
        assert np.ptp(f[WC.FLAT][:, 2:].reshape(-1, 3), 0).max() == 0
    # the minimum-eigenvalue output differs from the error output where a point is kept
    assert not np.array_equal(WC.ref_gray(0)[2], WC.ref_gray(O.OPTFLOW_LK_GET_MIN_EIGENVALS)[2])
