"""tbdk_warp_perspective_dev on the GPU: warpPerspective with its matrix in device
memory is byte-identical to tbdk_warp_perspective given the same matrix from the
host, for the 130x121 source of tests/_remap_cases.py into 130x33 and 67x15, 8U and
32F, one and three channels, NEAREST / LINEAR / CUBIC (8U), with and without
WARP_INVERSE_MAP.  The matrices are three of persp_cases' and one that
tbdk_find_homography produced in the same stream with no synchronisation between
the two calls.  A zero `valid` flag, or a matrix that is not finite, leaves a
pre-filled destination untouched."""
import numpy as np
import pytest
import torch

import _homography_cases as HC
import _remap_cases as PC
import _remap_oracle as R

pytestmark = pytest.mark.gpu

SW, SH = 130, 121
DESTS = ((130, 33), (67, 15))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def variants():
    for depth in ("8u", "32f"):
        for cn in (1, 3):
            for inter in ((0, 1, 2) if depth == "8u" else (0, 1)):
                for inv in (0, R.WARP_INVERSE_MAP):
                    yield depth, cn, inter | inv


def compare(gpu, Md, valid=None):
    """every variant with the device matrix Md against the host call with the downloaded matrix"""
    from opencv_amd import klt

    k = 0
    for depth, cn, flags in variants():
        for dw, dh in DESTS:
            src = dev(PC.image(SW, SH, cn, depth, 7100 + k))
            fill = PC.image(dw, dh, cn, depth, 9100 + k)
            border = k % 6
            got = klt.warp_perspective(src, Md, (dw, dh), flags, border, PC.BORDER_VALUE, dst=dev(fill), ctx=gpu,
                                       valid=valid)
            # the download synchronises; it comes after the device-matrix call
            want = klt.warp_perspective(src, Md.cpu().numpy(), (dw, dh), flags, border, PC.BORDER_VALUE, dst=dev(fill),
                                        ctx=gpu)
            assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (depth, cn, flags, dw, dh, border)
            k += 1
    return k


@pytest.mark.parametrize("name", ("mild", "wcross", "large"))
def test_equals_the_host_matrix_call(gpu, name):
    M = PC.matrix(name, SW, SH, 130, 33)
    assert compare(gpu, dev(M.reshape(9))) == 40


def test_a_matrix_from_find_homography_in_the_same_stream(gpu):
    from opencv_amd import klt

    src, dst = HC.points("plane", 200, 30, "mild", 12)
    r = klt.find_homography(dev(src), dev(dst), ctx=gpu)  # no synchronisation: the warps below queue behind it
    assert compare(gpu, r.H[0].reshape(9), valid=r.valid[0:1]) == 40
    assert int(r.valid[0]) == 1


def test_invalid_or_non_finite_leaves_the_destination_untouched(gpu):
    from opencv_amd import klt

    src = dev(PC.image(SW, SH, 3, "8u", 7200))
    fill = PC.image(67, 15, 3, "8u", 9200)
    M = dev(PC.matrix("mild", SW, SH, 67, 15).reshape(9))
    zero, one = dev(np.zeros(1, np.int32)), dev(np.ones(1, np.int32))
    out = klt.warp_perspective(src, M, (67, 15), R.INTER_LINEAR, 0, PC.BORDER_VALUE, dst=dev(fill), ctx=gpu, valid=zero)
    assert np.array_equal(out.cpu().numpy(), fill)
    out = klt.warp_perspective(src, M, (67, 15), R.INTER_LINEAR, 0, PC.BORDER_VALUE, dst=dev(fill), ctx=gpu, valid=one)
    assert not np.array_equal(out.cpu().numpy(), fill)
    bad = M.clone()
    bad[7] = float("nan")
    out = klt.warp_perspective(src, bad, (67, 15), R.INTER_LINEAR, 0, PC.BORDER_VALUE, dst=dev(fill), ctx=gpu)
    assert np.array_equal(out.cpu().numpy(), fill)
    # a set without a result: find_homography's valid flag gates the warp
    s, d = HC.points("collinear", 20, 0, "mild", 700)
    r = klt.find_homography(dev(s), dev(d), ctx=gpu)
    out = klt.warp_perspective(src, r.H[0].reshape(9), (67, 15), R.INTER_LINEAR, 0, PC.BORDER_VALUE, dst=dev(fill),
                               ctx=gpu, valid=r.valid[0:1])
    assert np.array_equal(out.cpu().numpy(), fill) and int(r.valid[0]) == 0
