"""The image front end on the GPU (cvt_color, resize_linear, the fused
colour -> gray -> resize pass) vs tests/_frontend_oracle.py, which
tests/test_frontend_oracle.py pins to the real cv::cvtColor / cv::resize:
bit-exact (integer fixed-point paths)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _frontend_oracle as F

pytestmark = pytest.mark.gpu

CVT_SIZES = [(97, 61), (6, 5)]
# the recorded shapes, two with an odd width halved (x scale exactly 2 or not, never the
# exact-2 path), a destination width that is no multiple of 4, one row, one column
RESIZE_SHAPES = [(97, 61, 31, 20), (50, 40, 123, 77), (400, 300, 320, 240), (64, 48, 32, 24), (33, 7, 32, 7),
                 (5, 5, 9, 3), (640, 480, 610, 457), (1242, 375, 621, 188), (40, 30, 40, 30), (31, 1, 13, 4),
                 (1, 9, 7, 3)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("size", CVT_SIZES)
@pytest.mark.parametrize("code", sorted(F.SRC_CN))
def test_cvt_color_matches_oracle(gpu, size, code):
    from opencv_amd import klt

    w, h = size
    src = F.pattern(w, h, F.SRC_CN[code], 300 + code)
    assert np.array_equal(host(klt.cvt_color(dev(src), code, ctx=gpu)), F.cvt_color(src, code))


@pytest.mark.parametrize("shape", RESIZE_SHAPES)
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_resize_linear_matches_oracle(gpu, shape, cn):
    from opencv_amd import klt

    sw, sh, dw, dh = shape
    src = F.pattern(sw, sh, cn, 400 + cn)
    assert np.array_equal(host(klt.resize_linear(dev(src), (dw, dh), ctx=gpu)), F.resize_linear(src, (dw, dh)))


def test_pitch_larger_than_the_row_and_unaligned_rows(gpu):
    """Source and destination are windows of wider tensors (pitch > row, rows
    and first pixels at odd addresses); the bytes around the destination stay."""
    from opencv_amd import klt

    for cn in (1, 3, 4):
        sw, sh, dw, dh = 53, 21, 37, 17
        src = F.pattern(sw, sh, cn, 500 + cn)
        big = torch.zeros((sh, sw + 5) + ((cn,) if cn > 1 else ()), dtype=torch.uint8, device="cuda")
        big[:, 3:3 + sw] = dev(src)
        out = torch.full((dh, dw + 6) + ((cn,) if cn > 1 else ()), 77, dtype=torch.uint8, device="cuda")
        klt.resize_linear(big[:, 3:3 + sw], (dw, dh), dst=out[:, 1:1 + dw], ctx=gpu)
        o = host(out)
        assert np.array_equal(o[:, 1:1 + dw], F.resize_linear(src, (dw, dh)))
        assert (o[:, :1] == 77).all() and (o[:, 1 + dw:] == 77).all()
    for code in sorted(F.SRC_CN):
        scn = F.SRC_CN[code]
        src = F.pattern(53, 9, scn, 520 + code)
        big = torch.zeros((9, 58) + ((scn,) if scn > 1 else ()), dtype=torch.uint8, device="cuda")
        big[:, 3:56] = dev(src)
        ref = F.cvt_color(src, code)
        out = torch.full((9, 59) + ref.shape[2:], 77, dtype=torch.uint8, device="cuda")
        klt.cvt_color(big[:, 3:56], code, dst=out[:, 1:54], ctx=gpu)
        o = host(out)
        assert np.array_equal(o[:, 1:54], ref), code
        assert (o[:, :1] == 77).all() and (o[:, 54:] == 77).all()


@pytest.mark.parametrize("shape", [(400, 300, 320, 240), (640, 480, 320, 240), (50, 40, 123, 77), (97, 61, 31, 20),
                                   (40, 30, 40, 30)])
@pytest.mark.parametrize("code", [F.COLOR_BGR2GRAY, F.COLOR_RGB2GRAY, F.COLOR_BGRA2GRAY, F.COLOR_RGBA2GRAY])
def test_fused_equals_the_two_calls(gpu, shape, code):
    from opencv_amd import klt

    sw, sh, dw, dh = shape
    src = F.pattern(sw, sh, F.SRC_CN[code], 600 + code)
    d = dev(src)
    fused = host(klt.cvt_resize_gray(d, code, (dw, dh), ctx=gpu))
    two = host(klt.resize_linear(klt.cvt_color(d, code, ctx=gpu), (dw, dh), ctx=gpu))
    assert np.array_equal(fused, two)
    assert np.array_equal(fused, F.cvt_resize_gray(src, code, (dw, dh)))


def test_repeated_size_reuses_the_tables(gpu):
    """Sizes alternate over more pairs than one and come back: the cached tables
    still give the same bits."""
    from opencv_amd import klt

    src = dev(F.pattern(90, 70, 1, 700))
    shapes = [(31, 20), (123, 77), (64, 33), (31, 20), (123, 77), (64, 33)]
    outs = [host(klt.resize_linear(src, s, ctx=gpu)) for s in shapes]
    for s, o in zip(shapes, outs):
        assert np.array_equal(o, F.resize_linear(F.pattern(90, 70, 1, 700), s))


def test_bad_arguments(gpu):
    from opencv_amd import _lib, klt

    lib, P = gpu.lib, C.c_void_p
    src = dev(F.pattern(16, 8, 3, 1))
    gray = torch.empty((8, 16), dtype=torch.uint8, device="cuda")
    two = torch.zeros((8, 16, 2), dtype=torch.uint8, device="cuda")
    out = torch.empty((4, 8, 3), dtype=torch.uint8, device="cuda")
    # unknown code (5 is COLOR_RGBA2BGRA in the reference: not built)
    assert lib.tbdk_cvt_color_u8(gpu.handle, P(src.data_ptr()), 16, 8, 48, P(gray.data_ptr()), 16, 5,
                                 None) == _lib.TBDK_EINVAL
    assert lib.tbdk_cvt_resize_gray_u8(gpu.handle, P(src.data_ptr()), 16, 8, 48, _lib.COLOR_BGR2BGRA,
                                       P(gray.data_ptr()), 8, 4, 16, None) == _lib.TBDK_EINVAL
    # cn = 2
    assert lib.tbdk_resize_linear_u8(gpu.handle, P(two.data_ptr()), 16, 8, 32, 2, P(out.data_ptr()), 8, 4, 24,
                                     None) == _lib.TBDK_EINVAL
    # aliasing destination
    assert lib.tbdk_resize_linear_u8(gpu.handle, P(src.data_ptr()), 16, 8, 48, 3, P(src.data_ptr()), 8, 4, 24,
                                     None) == _lib.TBDK_EINVAL
    assert lib.tbdk_cvt_color_u8(gpu.handle, P(src.data_ptr()), 16, 8, 48, P(src.data_ptr() + 16), 16,
                                 _lib.COLOR_BGR2GRAY, None) == _lib.TBDK_EINVAL
    # pitch smaller than the row, empty sizes, null pointers
    assert lib.tbdk_cvt_color_u8(gpu.handle, P(src.data_ptr()), 16, 8, 47, P(gray.data_ptr()), 16,
                                 _lib.COLOR_BGR2GRAY, None) == _lib.TBDK_EINVAL
    assert lib.tbdk_resize_linear_u8(gpu.handle, P(src.data_ptr()), 16, 8, 48, 3, P(out.data_ptr()), 0, 4, 24,
                                     None) == _lib.TBDK_EINVAL
    assert lib.tbdk_resize_linear_u8(gpu.handle, None, 16, 8, 48, 3, P(out.data_ptr()), 8, 4, 24,
                                     None) == _lib.TBDK_EINVAL
    # the wrappers raise before the call
    with pytest.raises(_lib.TbdkError):
        klt.cvt_color(src, 5, ctx=gpu)
    with pytest.raises(_lib.TbdkError):
        klt.cvt_color(gray, klt.COLOR_BGR2GRAY, ctx=gpu)
    with pytest.raises(_lib.TbdkError):
        klt.resize_linear(two, (8, 4), ctx=gpu)
    with pytest.raises(_lib.TbdkError):
        klt.resize_linear(src.cpu(), (8, 4), ctx=gpu)
