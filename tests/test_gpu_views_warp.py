"""warp_affine on pitched, unaligned views (tests/_views.py): source (61, 93)
and destination (50, 70) both interior windows of noise-filled allocations.
warp.hip stores four pixels at once where the destination address is
dword-aligned, so the destination runs through every layout; the result is
bit-exact with O.warp_affine (test_gpu_warp.py's criterion), the prior content
survives where BORDER_TRANSPARENT leaves it, and no guard byte changes."""
import ctypes as C

import numpy as np
import pytest
import torch

import _oracle as O
import _views as V
from test_warp_oracle import rotation_matrix

pytestmark = pytest.mark.gpu

LAYOUTS = list(V.LAYOUTS)
BORDERS = [O.BORDER_CONSTANT, O.BORDER_REPLICATE, O.BORDER_REFLECT, O.BORDER_WRAP, O.BORDER_REFLECT_101,
           O.BORDER_TRANSPARENT]
SW, SH, DW, DH, BVAL = 93, 61, 70, 50, 201


def dwin(arr, layout, seed=0):
    return V.window(arr, layout, seed, device="cuda")


@pytest.fixture(scope="module")
def case():
    """source, prior destination, matrix and the oracle's result for every mode,
    computed once.  The matrix sends part of the destination outside the
    source, so every border mode acts, in the forward and the inverse sense."""
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (SH, SW), dtype=np.uint8)
    init = rng.integers(0, 256, (DH, DW), dtype=np.uint8)
    M = rotation_matrix(SW / 2.0, SH / 2.0, 40.0, 0.9)
    M[:, 2] += (-15.5, -6.25)
    refs = {}
    for inter in (O.INTER_NEAREST, O.INTER_LINEAR, O.INTER_CUBIC):
        for border in BORDERS:
            for inverse in (False, True):
                flags = inter | (O.WARP_INVERSE_MAP if inverse else 0)
                refs[inter, border, inverse] = O.warp_affine(src, M, (DW, DH), flags, border, BVAL, dst=init.copy())
    for inter in (O.INTER_NEAREST, O.INTER_LINEAR, O.INTER_CUBIC):
        for inverse in (False, True):
            kept = refs[inter, O.BORDER_TRANSPARENT, inverse] == init
            moved = refs[inter, O.BORDER_CONSTANT, inverse] != init
            assert (kept & moved).sum() > 100  # the transparent border does keep prior pixels here
    return src, init, M, refs


@pytest.mark.parametrize("dlayout", LAYOUTS)
@pytest.mark.parametrize("inter", [O.INTER_NEAREST, O.INTER_LINEAR, O.INTER_CUBIC])
def test_warp_affine_on_views(gpu, case, dlayout, inter):
    from opencv_amd import klt

    src, init, M, refs = case
    slayout = LAYOUTS[(LAYOUTS.index(dlayout) + 2 + inter) % len(LAYOUTS)]  # every source layout meets every filter
    ps, vs = dwin(src, slayout, seed=1)
    s0 = V.snapshot(ps)
    for border in BORDERS:
        for inverse in (False, True):
            pd, vd = dwin(init, dlayout, seed=2)
            d0 = V.snapshot(pd)
            flags = inter | (O.WARP_INVERSE_MAP if inverse else 0)
            out = klt.warp_affine(vs, M, (DW, DH), flags, border, BVAL, dst=vd, ctx=gpu)
            torch.cuda.synchronize()
            assert out is vd
            tag = f"border {border} inverse {inverse} src {slayout}"
            assert np.array_equal(vd.cpu().numpy(), refs[inter, border, inverse]), tag
            assert V.guards_intact(pd, d0, vd), tag
    assert torch.equal(ps, s0)


def test_pitch_below_the_row_is_refused(gpu, case):
    from opencv_amd import _lib

    src, init, M, _ = case
    ps, vs = dwin(src, "odd_both")
    pd, vd = dwin(init, "odd_both", seed=1)
    d0 = V.snapshot(pd)
    m = (C.c_double * 6)(*M.reshape(6))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for sp, dp in ((SW - 1, vd.stride(0)), (vs.stride(0), DW - 1)):
        assert gpu.lib.tbdk_warp_affine_u8(gpu.handle, vs.data_ptr(), SW, SH, sp, vd.data_ptr(), DW, DH, dp, m,
                                           O.INTER_LINEAR, O.BORDER_CONSTANT, 0, s) == _lib.TBDK_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(pd, d0)
