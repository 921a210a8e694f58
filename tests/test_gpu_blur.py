"""GPU: tbdk_gaussian_blur_u8 (opencv_amd.imgproc.gaussian_blur, opencv_amd.bgsegm.smooth_mask) against the outputs
recorded from the real reference (tests/golden/reference_blur.npz), byte for byte or row CRC for row CRC, and
against the numpy restatement (tests/_blur_oracle.py) on shapes chosen for the kernel's own seams: its tile is 128
bytes x 32 rows, so widths around 128 and 256 bytes for one, three and four channels, heights around 32 and 64,
pitched odd-aligned views with guarded padding, in-place calls, every compile-time instance against the run-time
one; the fused threshold against blur then threshold; poisoned scratch and a context born dirty."""
import ctypes as C

import numpy as np
import pytest
import torch

import _blur_cases as UC
import _blur_oracle as BO
import _reference_cases as RC
import _views as V
from test_gpu_dirty_state import byte_param, dirty_twice, fresh_context

pytestmark = pytest.mark.gpu

CASES = UC.cases()
KERNELS = UC.kernels()
TILE_W, TILE_H = 128, 32


def IP():
    from opencv_amd import imgproc

    return imgproc


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("blur")


def blur(gpu, img, kernel, border, dst=None, threshold=None, stream=None):
    kw, kh, sx, sy = KERNELS[kernel] if isinstance(kernel, str) else kernel
    src = img if isinstance(img, torch.Tensor) else torch.from_numpy(img).cuda()
    return IP().gaussian_blur(src, (kw, kh), sx, dst, sy, border, stream, threshold, ctx=gpu)


def ref(img, kernel, border, threshold=None):
    kw, kh, sx, sy = KERNELS[kernel] if isinstance(kernel, str) else kernel
    return BO.gaussian_blur(img, (kw, kh), sx, sy, border, threshold=threshold)


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: UC.label(i).replace(" ", "_"))
def test_equals_the_recorded_reference_and_fuses(gpu, fx, i):
    c = CASES[i]
    img = UC.case_image(c)
    src = torch.from_numpy(img).cuda()
    out = blur(gpu, src, c["kernel"], c["border"], src if c["inplace"] else None)
    assert (out is src) == c["inplace"]
    got = out.cpu().numpy()
    RC.assert_pinned(got, fx[f"{i}_d"], UC.label(i))
    # the fused call equals blur followed by threshold, here and through tbdk_threshold
    t = (UC.THRESHOLDS[1 + i % 4], UC.MAXVALS[i % 3], UC.TYPES[i % 5])
    fused = blur(gpu, torch.from_numpy(img).cuda(), c["kernel"], c["border"], threshold=t)
    _, two = IP().threshold(torch.from_numpy(got).cuda(), *t, ctx=gpu)
    assert torch.equal(fused, two), (UC.label(i), t)
    assert np.array_equal(two.cpu().numpy(), BO.threshold_u8(got, *t)[1]), (UC.label(i), t)


def test_smooth_mask_equals_the_recorded_11x11_row(gpu, fx):
    from opencv_amd import bgsegm

    name, thresh, maxval, type_ = UC.SMOOTH_MASK
    rows = [i for i, c in enumerate(CASES) if c["kernel"] == name and c["content"] in ("mog2", "runs")
            and c["border"] == UC.REFLECT_101]
    assert len(rows) == 2
    for i in rows:
        img = UC.case_image(CASES[i])
        blurred = ref(img, name, UC.REFLECT_101)
        RC.assert_pinned(blurred, fx[f"{i}_d"], UC.label(i))  # the restatement is the recording here
        want = BO.threshold_u8(blurred, thresh, maxval, type_)[1]
        assert 0 < (want == 255).mean() < 1
        mask = torch.from_numpy(img).cuda()
        assert np.array_equal(bgsegm.smooth_mask(mask, ctx=gpu).cpu().numpy(), want), UC.label(i)
        assert bgsegm.smooth_mask(mask, dst=mask, ctx=gpu) is mask and np.array_equal(mask.cpu().numpy(), want)


SEAM_SHAPES = [(2 * TILE_W + 1, 2 * TILE_H + 1, 1), (TILE_W - 1, TILE_H - 1, 1), (TILE_W + 1, TILE_H + 1, 1),
               (TILE_W, TILE_H, 1), (43, 70, 3), (85, 33, 3), (32, 31, 4), (65, 66, 4), (31, 5, 4), (2, 3, 3)]


@pytest.mark.parametrize("w,h,cn", SEAM_SHAPES, ids=lambda v: str(v))
def test_tile_seams_and_every_instance_against_the_generic_one(gpu, w, h, cn):
    img = np.ascontiguousarray(UC.pattern(w, h, cn, 6000 + w + 3 * h + cn))
    for j, name in enumerate(("3@0", "5@0.8", "7@1.5", "11@3.5", "25@max", "31@5", "5x11", "7x1")):
        for border in (UC.BORDERS[j % 5], UC.REFLECT_101):
            want = ref(img, name, border)
            got = blur(gpu, img, name, border).cpu().numpy()
            assert np.array_equal(got, want), (name, border, np.argwhere(got != want)[:4].tolist())
            gpu.set_option("blur_generic", 1)
            try:
                generic = blur(gpu, img, name, border).cpu().numpy()
            finally:
                gpu.set_option("blur_generic", 0)
            assert np.array_equal(generic, want), ("generic", name, border)


@pytest.mark.parametrize("layout", ["odd_both", "odd_pitch", "odd_base", "a16_pitched"])
@pytest.mark.parametrize("cn", [1, 3])
def test_pitched_odd_aligned_source_and_destination(gpu, layout, cn):
    img = np.ascontiguousarray(UC.pattern(2 * TILE_W // cn + 7, 2 * TILE_H + 3, cn, 6100 + cn))
    for name, border, t in (("11@3.5", UC.REFLECT_101, None), ("5@0", UC.WRAP, (10.0, 255.0, BO.BINARY)),
                            ("31@5", UC.REPLICATE, None), ("5x11", UC.CONSTANT, None)):
        sp, sv = V.window(img, layout, seed=1, device="cuda")
        dp, dv = V.window(np.full_like(img, 0x33), "odd_both" if layout != "odd_both" else "odd_pitch", seed=2,
                          device="cuda")
        s0, d0 = V.snapshot(sp), V.snapshot(dp)
        out = blur(gpu, sv, name, border, dv, t)
        assert out is dv
        assert np.array_equal(V.host(dv), ref(img, name, border, t)), (name, border)
        assert torch.equal(sp, s0) and V.guards_intact(dp, d0, dv), (name, border)
        # in place on the view: the guards of the source's parent stay as they were
        same = blur(gpu, sv, name, border, sv, t)
        assert same is sv and np.array_equal(V.host(sv), ref(img, name, border, t)), (name, border, "in place")
        assert V.guards_intact(sp, s0, sv), (name, border, "in place")


def test_in_place_equals_out_of_place(gpu):
    for cn in (1, 4):
        img = np.ascontiguousarray(UC.pattern(300, 70, cn, 6200 + cn))
        for name, border in (("3@0", UC.REFLECT), ("11@3.5", UC.REFLECT_101), ("31@0", UC.WRAP), ("1x7", UC.REPLICATE)):
            a = torch.from_numpy(img).cuda()
            out = blur(gpu, a, name, border)
            same = blur(gpu, a, name, border, a)
            assert same is a and torch.equal(a, out), (cn, name)
            assert np.array_equal(out.cpu().numpy(), ref(img, name, border)), (cn, name)


def _raw(gpu, src, dst, w=None, h=None, cn=1, kw=3, kh=3, sx=0.0, sy=0.0, border=4, fused=None, spitch=None):
    from opencv_amd import _lib

    f = None if fused is None else C.byref(_lib.ThreshParams(fused[0], fused[1], fused[2], 0))
    return gpu.lib.tbdk_gaussian_blur_u8(gpu.handle, C.c_void_p(src.data_ptr()), src.shape[1] if w is None else w,
                                         src.shape[0] if h is None else h, cn, src.stride(0) if spitch is None else spitch,
                                         C.c_void_p(dst.data_ptr()), dst.stride(0), kw, kh, sx, sy, border, f, None)


def test_invalid_arguments_return_einval_and_leave_dst_untouched(gpu):
    from opencv_amd import _lib

    src = torch.from_numpy(UC.image(37, 23, "noise")).cuda()
    dst = torch.full_like(src, 0x5A)
    bad = [dict(kw=4), dict(kh=2), dict(kw=33), dict(kh=33), dict(kw=0, kh=0), dict(kw=0, kh=0, sx=5.2),  # automatic 33
           dict(kw=0, sx=-1.0), dict(sx=float("nan")), dict(sy=float("nan")), dict(border=5), dict(border=16),
           dict(border=-1), dict(cn=2), dict(cn=0), dict(cn=5), dict(w=0), dict(h=0), dict(w=65536), dict(w=38),
           dict(cn=3, w=13), dict(fused=(10.0, 255.0, 8)), dict(fused=(10.0, 255.0, 16)), dict(fused=(10.0, 255.0, 5)),
           dict(fused=(float("nan"), 255.0, 0))]
    for kw in bad:
        assert _raw(gpu, src, dst, **kw) == _lib.TBDK_EINVAL, kw
    assert gpu.lib.tbdk_gaussian_blur_u8(gpu.handle, None, 37, 23, 1, 37, C.c_void_p(dst.data_ptr()), 37, 3, 3, 0.0,
                                         0.0, 4, None, None) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())
    with pytest.raises(_lib.TbdkError):
        IP().gaussian_blur(src, (4, 4), 1.0, ctx=gpu)
    # the limits themselves are fine: 31 taps given, and the automatic 31 of sigma 5
    assert _raw(gpu, src, dst, kw=0, kh=0, sx=5.0) == _lib.TBDK_OK
    assert np.array_equal(dst.cpu().numpy(), BO.gaussian_blur(src.cpu().numpy(), (31, 31), 5.0))


STATE = {"11@3.5": UC.REFLECT_101, "31@5": UC.REPLICATE, "5@0": UC.WRAP}


def _state_image():
    return UC.image(130, 121, "runs")


@byte_param
@pytest.mark.parametrize("name", list(STATE))
def test_scratch_poisoned(gpu, name, byte):
    img = _state_image()
    want = ref(img, name, STATE[name])

    def call():  # in place: the one form that goes through the context's intermediate plane
        a = torch.from_numpy(img).cuda()
        return np.stack([blur(gpu, a, name, STATE[name]).cpu().numpy(), blur(gpu, a, name, STATE[name], a).cpu().numpy()])

    dirty_twice(gpu, byte, call, lambda g, what: np.testing.assert_array_equal(g, np.stack([want, want]), what),
                img.size, f"blur {name}")


@byte_param
def test_fresh_context(byte):
    img = _state_image()
    with fresh_context(byte) as ctx:
        for name, border in STATE.items():
            a = torch.from_numpy(img).cuda()
            np.testing.assert_array_equal(blur(ctx, a, name, border).cpu().numpy(), ref(img, name, border), name)
            np.testing.assert_array_equal(blur(ctx, a, name, border, a).cpu().numpy(), ref(img, name, border), name)
