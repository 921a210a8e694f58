"""GPU: tbdk_morph_u8 (opencv_amd.imgproc.erode / dilate / morphology_ex) against the outputs recorded from the
real reference (tests/golden/reference_morph.npz), byte for byte or row CRC for row CRC; its argument checks; in
place against out of place; pitched, odd-aligned source and destination."""
import ctypes as C

import numpy as np
import pytest
import torch

import _morph_cases as BC
import _morph_oracle as MO
import _reference_cases as RC
import _views as V

pytestmark = pytest.mark.gpu

CASES = BC.cases()
ELEMENTS = BC.elements()


def IP():
    from opencv_amd import imgproc

    return imgproc


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("morph")


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: BC.label(i).replace(" ", "_"))
def test_equals_the_recorded_reference(gpu, fx, i):
    c = CASES[i]
    src = torch.from_numpy(BC.image(c["w"], c["h"], c["content"])).cuda()
    dst = src if c["inplace"] else None
    out = IP().morphology_ex(src, c["op"], ELEMENTS[c["elem"]], dst, c["anchor"], c["it"], c["border"], c["bval"],
                             ctx=gpu)
    assert (out is src) == c["inplace"]
    RC.assert_pinned(out.cpu().numpy(), fx[f"{i}_d"], BC.label(i))


def test_in_place_equals_out_of_place(gpu):
    img = BC.image(130, 121, "noise")
    for op, name, it in ((BC.ERODE, "arb5x4", 1), (BC.DILATE, "arb5x4", 3), (BC.OPEN, "rect5x5", 1),
                         (BC.CLOSE, "ellipse7x7", 2), (BC.ERODE, "rect7x1", 1), (BC.DILATE, "rect3x3", 0)):
        a = torch.from_numpy(img).cuda()
        out = IP().morphology_ex(a, op, ELEMENTS[name], iterations=it, ctx=gpu)
        same = IP().morphology_ex(a, op, ELEMENTS[name], a, iterations=it, ctx=gpu)
        assert same is a and torch.equal(a, out), (op, name, it)
        assert np.array_equal(out.cpu().numpy(), MO.morphology_ex(img, op, ELEMENTS[name], iterations=it)), (op, name)


def _raw(gpu, src, dst, op=BC.ERODE, elem=None, kw=3, kh=3, anchor=(-1, -1), it=1, border=BC.CONSTANT, bval=-1,
         w=None, h=None):
    e = None if elem is None else np.ascontiguousarray(elem, np.uint8)
    return gpu.lib.tbdk_morph_u8(gpu.handle, op, C.c_void_p(src.data_ptr()), src.shape[1] if w is None else w,
                                 src.shape[0] if h is None else h, src.stride(0), C.c_void_p(dst.data_ptr()),
                                 dst.stride(0), None if e is None else e.ctypes.data_as(C.c_void_p), kw, kh, anchor[0],
                                 anchor[1], it, border, bval, None)


def test_invalid_arguments_return_einval_and_leave_dst_untouched(gpu):
    from opencv_amd import _lib

    src = torch.from_numpy(BC.image(37, 23, "noise")).cuda()
    dst = torch.full_like(src, 0x5A)
    ones = np.ones((3, 3), np.uint8)
    bad = [
        dict(op=4), dict(op=5), dict(op=6), dict(op=7), dict(op=-1),          # GRADIENT, TOPHAT, BLACKHAT, HITMISS
        dict(it=16),                                                          # the 3x3 rectangle at 16: 33 x 33
        dict(elem=ones, it=16),
        dict(elem=np.ones((32, 1), np.uint8), kw=1, kh=32), dict(elem=np.ones((1, 32), np.uint8), kw=32, kh=1),
        dict(elem=np.ones((17, 17), np.uint8), kw=17, kh=17, it=2),           # merges to 33 x 33
        dict(elem=np.zeros((3, 3), np.uint8)),                                # no non-zero entry
        dict(elem=ones, anchor=(3, 1)), dict(elem=ones, anchor=(1, -2)), dict(elem=ones, anchor=(-1, 3)),
        dict(border=3), dict(border=5), dict(border=16), dict(border=-1),     # WRAP, TRANSPARENT, ISOLATED
        dict(bval=256), dict(bval=-2), dict(it=-1),
        dict(w=0), dict(h=0), dict(w=65536), dict(w=38),                      # a pitch below the row
    ]
    for kw in bad:
        assert _raw(gpu, src, dst, **kw) == _lib.TBDK_EINVAL, kw
    assert gpu.lib.tbdk_morph_u8(gpu.handle, 0, None, 37, 23, 37, C.c_void_p(dst.data_ptr()), 37, None, 3, 3, -1, -1,
                                 1, 0, -1, None) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())
    with pytest.raises(_lib.TbdkError):
        IP().morphology_ex(src, 4, None, ctx=gpu)
    # the limit itself is fine
    assert _raw(gpu, src, dst, it=15) == _lib.TBDK_OK
    assert np.array_equal(dst.cpu().numpy(), MO.morphology_ex(src.cpu().numpy(), MO.ERODE, None, iterations=15))


@pytest.mark.parametrize("layout", ["odd_both", "odd_pitch", "odd_base"])
def test_pitched_odd_aligned_source_and_destination(gpu, layout):
    img = BC.image(130, 121, "noise")
    for op, name, border in ((BC.OPEN, "rect3x3", BC.CONSTANT), (BC.DILATE, "arb6x5z", BC.REFLECT_101),
                             (BC.ERODE, "ellipse15x15", BC.REPLICATE)):
        sp, sv = V.window(img, layout, seed=1, device="cuda")
        dp, dv = V.window(np.full_like(img, 0x33), "odd_both" if layout != "odd_both" else "odd_pitch", seed=2,
                          device="cuda")
        s0, d0 = V.snapshot(sp), V.snapshot(dp)
        out = IP().morphology_ex(sv, op, ELEMENTS[name], dv, borderType=border, ctx=gpu)
        assert out is dv
        assert np.array_equal(V.host(dv), MO.morphology_ex(img, op, ELEMENTS[name], border=border)), (op, name)
        assert torch.equal(sp, s0) and V.guards_intact(dp, d0, dv), (op, name)


def test_structuring_element_facade():
    for shape, kw, kh, anchor in BC.strel_cases():
        assert np.array_equal(IP().get_structuring_element(shape, (kw, kh), anchor),
                              MO.structuring_element(shape, (kw, kh), anchor))
