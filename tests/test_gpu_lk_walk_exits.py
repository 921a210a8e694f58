"""Every one-point-per-wave PyrLK kernel takes every way out of the level walk
(opencv_amd/csrc/lk_walk.hpp), bit for bit with the oracle in exact-sum mode.

The inputs are tests/_lk_walk_cases.py: a 160x120 pair, window 9x9, 3 levels, 2
Newton steps per level, and a point list that tests/test_lk_walk_exits_cases.py
shows (on the CPU, from the oracle alone) to contain, for each pixel type and
each flag setting, points lost with no step taken, lost after steps, kept after
every step and kept after fewer.  The kernels: lk_strip_kernel (impl 1),
lk_sparse_kernel (impl 2), lk_sparse_kernel + lk_sparse_back_kernel (the
forward-backward call at window 8), lk_cn_kernel (3 u8 channels) and
lk_cn_f32_kernel (3 channels of a 16U frame); each with flags 0,
GET_MIN_EIGENVALS and USE_INITIAL_FLOW."""
import numpy as np
import pytest
import torch

import _lk_walk_cases as WC
import _oracle as O
from test_gpu_f32 import _cn_pyr
from test_gpu_klt import assert_exact, to_dev
from test_gpu_lk_fb import back_equal, bits, host

pytestmark = pytest.mark.gpu


def _flow(flags, win=WC.WIN, impl=0):
    from opencv_amd import klt

    return klt.SparsePyrLKOpticalFlow((win, win), WC.MAX_LEVEL, WC.MAX_COUNT, bool(flags & O.OPTFLOW_USE_INITIAL_FLOW),
                                      epsilon=WC.EPS, minEigThreshold=WC.MIN_EIG,
                                      getMinEigenVals=bool(flags & O.OPTFLOW_LK_GET_MIN_EIGENVALS), impl=impl)


def _init(flags):
    return to_dev(WC.initial_flow()) if flags & O.OPTFLOW_USE_INITIAL_FLOW else None


def _calc(lk, Pa, Pb, flags):
    r = lk.calc(Pa, Pb, to_dev(WC.points()), _init(flags), want_iters=True)
    torch.cuda.synchronize()
    return r.next_pts.cpu().numpy(), r.status.cpu().numpy(), r.err.cpu().numpy(), r.iters.cpu().numpy()


@pytest.mark.parametrize("flags", WC.FLAGS)
@pytest.mark.parametrize("impl", [pytest.param(1, id="strip"), pytest.param(2, id="generic")])
def test_gray(gpu, impl, flags):
    from opencv_amd import klt

    a, b = WC.gray_pair()
    win = (WC.WIN, WC.WIN)
    Pa, Pb = (klt.build_pyramid(to_dev(f), win, WC.MAX_LEVEL, ctx=gpu) for f in (a, b))
    assert_exact(_calc(_flow(flags, impl=impl), Pa, Pb, flags), WC.ref_gray(flags))


@pytest.mark.parametrize("flags", WC.FLAGS)
def test_forward_backward_window_8(gpu, flags):
    from opencv_amd import klt

    a, b = WC.gray_pair()
    win = (WC.FB_WIN, WC.FB_WIN)
    Pa, Pb = (klt.build_pyramid(to_dev(f), win, WC.MAX_LEVEL, ctx=gpu) for f in (a, b))
    ref = WC.ref_fb(flags)
    g = host(_flow(flags, win=WC.FB_WIN).calc_checked(Pa, Pb, to_dev(WC.points()), _init(flags),
                                                      back_threshold=WC.FB_THR, want_iters=True))
    assert np.array_equal(g["status"], ref.status)
    ok = ref.fwd_status == 1
    assert np.array_equal(bits(g["next_pts"][ok]), bits(ref.next_pts[ok]))
    assert np.array_equal(bits(g["err"][ok]), bits(ref.err[ok])) and np.array_equal(g["iters"], ref.iters)
    back_equal(g, ref)


@pytest.mark.parametrize("flags", WC.FLAGS)
def test_u8_cn3(gpu, flags):
    from opencv_amd import klt

    a, b = WC.cn3_pair()
    win = (WC.WIN, WC.WIN)
    Pa, Pb = (klt.build_pyramid(to_dev(f), win, WC.MAX_LEVEL, ctx=gpu) for f in (a, b))
    assert Pa.channels == 3
    assert_exact(_calc(_flow(flags), Pa, Pb, flags), WC.ref_cn3(flags))


@pytest.mark.parametrize("flags", WC.FLAGS)
def test_u16_cn3(gpu, flags):
    a, b = WC.u16_cn3_pair()
    win = (WC.WIN, WC.WIN)
    Pa, Pb = _cn_pyr(gpu, a, win, WC.MAX_LEVEL), _cn_pyr(gpu, b, win, WC.MAX_LEVEL)
    assert_exact(_calc(_flow(flags), Pa, Pb, flags), WC.ref_u16_cn3(flags))
