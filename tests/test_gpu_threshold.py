"""GPU: tbdk_threshold (opencv_amd.imgproc.threshold) against the outputs recorded from the real reference
(tests/golden/reference_threshold.npz): every 8U case with its constant-fill and copy thresholds, the 32F cases with
NaN and infinities, THRESH_OTSU with the chosen threshold read back from its device word; then the numpy restatement
on shapes around the kernels' 4-byte groups and 1024-byte blocks, pitched odd-aligned views with guarded padding,
in-place calls, poisoned scratch and a context born dirty."""
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

CASES = UC.thresh_cases()


def IP():
    from opencv_amd import imgproc

    return imgproc


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("threshold")


def _group(kind):
    return [i for i, c in enumerate(CASES) if c["kind"] == kind]


@pytest.mark.parametrize("type_", UC.TYPES, ids=[BO.TYPE_NAMES[t] for t in UC.TYPES])
def test_8u_equals_the_recorded_reference(gpu, fx, type_):
    rows = [i for i in _group("u8") if CASES[i]["type"] == type_]
    assert len(rows) == 2 * len(UC.THRESHOLDS) * len(UC.MAXVALS)
    for i in rows:
        c = CASES[i]
        src = torch.from_numpy(UC.thresh_image(c)).cuda()
        used, out = IP().threshold(src, c["thresh"], c["maxval"], c["type"], ctx=gpu)
        RC.assert_pinned(out.cpu().numpy(), fx[f"{i}_d"], UC.thresh_label(i))
        assert np.float64(used).view(np.int64) == fx[f"{i}_t"][0], UC.thresh_label(i)


def test_32f_equals_the_recorded_reference(gpu, fx):
    rows = _group("f32")
    assert len(rows) == 30
    for i in rows:
        c = CASES[i]
        img = UC.thresh_image(c)
        assert np.isnan(img).any() and np.isinf(img).any()
        used, out = IP().threshold(torch.from_numpy(img).cuda(), c["thresh"], c["maxval"], c["type"], ctx=gpu)
        RC.assert_pinned(out.cpu().numpy().view(np.int32), fx[f"{i}_d"], UC.thresh_label(i))
        assert np.float64(used).view(np.int64) == fx[f"{i}_t"][0], UC.thresh_label(i)


def test_otsu_equals_the_recorded_reference(gpu, fx):
    rows = _group("otsu")
    assert len(rows) == 2 * len(UC.OTSU_IMAGES)
    for i in rows:
        c = CASES[i]
        word, out = IP().threshold(torch.from_numpy(UC.thresh_image(c)).cuda(), c["thresh"], c["maxval"], c["type"],
                                   ctx=gpu)
        assert isinstance(word, torch.Tensor) and word.dtype == torch.int32 and word.is_cuda
        assert float(word.item()) == float(fx[f"{i}_t"].view(np.float64)[0]), UC.thresh_label(i)
        RC.assert_pinned(out.cpu().numpy(), fx[f"{i}_d"], UC.thresh_label(i))


@pytest.mark.parametrize("w,h,cn", [(1, 1, 1), (3, 2, 1), (1023, 3, 1), (1025, 2, 1), (1024, 1, 1), (343, 5, 3),
                                    (257, 4, 4), (4099, 2, 1)], ids=lambda v: str(v))
def test_block_seams(gpu, w, h, cn):
    img = np.ascontiguousarray(UC.pattern(w, h, cn, 6300 + w + h + cn))
    f32 = ((img.astype(np.float32) - np.float32(90.0)) * np.float32(0.7)).reshape(h, w * cn)
    for t in UC.TYPES:
        for th, mv in ((99.5, 200.0), (-3.0, 77.0), (255.0, 255.0)):
            used, out = IP().threshold(torch.from_numpy(img).cuda(), th, mv, t, ctx=gpu)
            ru, ro = BO.threshold_u8(img, th, mv, t)
            assert used == ru and np.array_equal(out.cpu().numpy(), ro), (t, th, mv)
        used, out = IP().threshold(torch.from_numpy(f32).cuda(), 11.25, 3.5, t, ctx=gpu)
        ru, ro = BO.threshold_f32(f32, 11.25, 3.5, t)
        assert used == ru and np.array_equal(out.cpu().numpy(), ro), ("f32", t)
    if cn == 1:
        for t in (BO.BINARY, BO.TRUNC, BO.TOZERO):
            word, out = IP().threshold(torch.from_numpy(img).cuda(), 0, 255, t | BO.OTSU, ctx=gpu)
            ru, ro = BO.threshold_u8(img, 0, 255, t | BO.OTSU)
            assert float(word.item()) == ru and np.array_equal(out.cpu().numpy(), ro), ("otsu", t)


@pytest.mark.parametrize("layout", ["odd_both", "odd_pitch", "odd_base", "vec4"])
def test_pitched_odd_aligned_views_and_in_place(gpu, layout):
    img = UC.image(130, 121, "noise")
    for t, th in ((BO.BINARY, 100.0), (BO.TOZERO_INV, 30.5), (BO.TRUNC | BO.OTSU, 0.0)):
        sp, sv = V.window(img, layout, seed=3, device="cuda")
        dp, dv = V.window(np.full_like(img, 0x33), "odd_both" if layout != "odd_both" else "odd_pitch", seed=4,
                          device="cuda")
        s0, d0 = V.snapshot(sp), V.snapshot(dp)
        want = BO.threshold_u8(img, th, 250.0, t)[1]
        _, out = IP().threshold(sv, th, 250.0, t, dv, ctx=gpu)
        assert out is dv and np.array_equal(V.host(dv), want), (t, th)
        assert torch.equal(sp, s0) and V.guards_intact(dp, d0, dv), (t, th)
        _, same = IP().threshold(sv, th, 250.0, t, sv, ctx=gpu)
        assert same is sv and np.array_equal(V.host(sv), want) and V.guards_intact(sp, s0, sv), (t, th, "in place")
    f = UC.f32_image()
    fp, fv = V.window(f, "a16_pitched", seed=5, device="cuda")
    f0 = V.snapshot(fp)
    _, same = IP().threshold(fv, 0.5, 9.0, BO.TOZERO, fv, ctx=gpu)
    assert np.array_equal(V.host(fv).view(np.int32), BO.threshold_f32(f, 0.5, 9.0, BO.TOZERO)[1].view(np.int32))
    assert V.guards_intact(fp, f0, fv)


def _raw(gpu, src, dst, pix=0, w=None, h=None, cn=1, thresh=10.0, maxval=255.0, type_=0, word=None):
    return gpu.lib.tbdk_threshold(gpu.handle, C.c_void_p(src.data_ptr()), pix, src.shape[1] if w is None else w,
                                  src.shape[0] if h is None else h, cn, src.stride(0) * src.element_size(),
                                  C.c_void_p(dst.data_ptr()), dst.stride(0) * dst.element_size(), thresh, maxval, type_,
                                  None, None if word is None else C.c_void_p(word.data_ptr()), None)


def test_invalid_arguments_return_einval_and_leave_dst_untouched(gpu):
    from opencv_amd import _lib

    src = torch.from_numpy(UC.image(37, 23, "noise")).cuda()
    dst = torch.full_like(src, 0x5A)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = [dict(type_=5), dict(type_=7), dict(type_=16), dict(type_=16 | 8), dict(type_=32), dict(type_=-1),
           dict(type_=8),                                   # OTSU without its device word
           dict(type_=8, word=word, cn=3, w=12), dict(pix=1), dict(pix=3), dict(w=0), dict(h=0), dict(w=38), dict(cn=0),
           dict(thresh=float("nan")), dict(maxval=float("nan")), dict(pix=2, w=10)]  # 32F rows of 40 bytes in 37
    for kw in bad:
        assert _raw(gpu, src, dst, **kw) == _lib.TBDK_EINVAL, kw
    f = torch.zeros((4, 9), dtype=torch.float32, device="cuda")
    assert _raw(gpu, f, f, pix=2, type_=8, word=word) == _lib.TBDK_EINVAL  # OTSU on 32F
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all()) and int(word.item()) == 0
    with pytest.raises(_lib.TbdkError):
        IP().threshold(src, 10, 255, 16, ctx=gpu)
    with pytest.raises(_lib.TbdkError):
        IP().threshold(src.to(torch.float32), 10, 255, 8, ctx=gpu)


@byte_param
def test_scratch_poisoned_and_fresh_context(gpu, byte):
    img = UC.otsu_image("bimodal")
    ru, ro = BO.threshold_u8(img, 0, 255, BO.BINARY | BO.OTSU)

    def call(ctx=gpu):
        word, out = IP().threshold(torch.from_numpy(img).cuda(), 0, 255, BO.BINARY | BO.OTSU, ctx=ctx)
        return int(word.item()), out.cpu().numpy()

    def check(g, what):
        assert g[0] == ru and np.array_equal(g[1], ro), what

    dirty_twice(gpu, byte, call, check, 1024, "otsu")  # the histogram lives in the context's intermediate plane
    with fresh_context(byte) as ctx:
        check(call(ctx), "otsu on a fresh context")
        check(call(ctx), "otsu on a fresh context, again")
