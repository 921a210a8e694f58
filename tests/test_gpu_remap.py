"""remap, remap_flow and warp_perspective on the GPU (libtbdk remap.hip): equal,
bit for bit, to the recordings of the real reference
(tests/golden/reference_remap.npz, reference_warpperspective.npz) and to the numpy
restatement tests/_remap_oracle.py, which tests/test_remap_oracle.py holds to the
same recordings."""
import os

import numpy as np
import pytest
import torch

import _frontend_oracle as F
import _oracle as O
import _reference_cases as RC
import _remap_cases as PC
import _remap_oracle as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(a, pad=0):
    """a device copy; with pad > 0 a view of a wider tensor, so the pitch is larger than the row"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    if not pad:
        return t.cuda()
    shape = list(t.shape)
    shape[1] += pad
    wide = torch.full(shape, 77, dtype=t.dtype).cuda()
    wide[:, :t.shape[1]] = t.cuda()
    return wide[:, :t.shape[1]]


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.fixture(scope="module")
def fx_remap():
    return RC.fixture("remap")


@pytest.fixture(scope="module")
def fx_persp():
    return RC.fixture("warpperspective")


def test_remap_equals_the_recorded_reference(gpu, fx_remap):
    from opencv_amd import klt

    for i, (depth, cn, s, d, gen, kind, inter, border) in enumerate(PC.remap_cases()):
        src, dst, m1, m2, k, bv = PC.remap_inputs(i)
        out = dev(dst, pad=3 if i % 2 else 0)
        got = klt.remap(dev(src, PC.SOURCES[s][2]), dev(m1), None if m2 is None else dev(m2), inter, border, bv, dst=out,
                        ctx=gpu)
        assert got is out
        RC.assert_pinned(got.cpu().numpy(), fx_remap[f"{i}_w"], PC.remap_label(i))


def test_warp_perspective_equals_the_recorded_reference(gpu, fx_persp):
    from opencv_amd import klt

    for i, (depth, cn, s, d, name, flags, border) in enumerate(PC.persp_cases()):
        src, dst, M, bv = PC.persp_inputs(i)
        got = klt.warp_perspective(dev(src, PC.SOURCES[s][2]), M, (dst.shape[1], dst.shape[0]), flags, border, bv,
                                   dst=dev(dst, pad=5 if i % 2 else 0), ctx=gpu)
        RC.assert_pinned(got.cpu().numpy(), fx_persp[f"{i}_w"], PC.persp_label(i))


def test_remap_flow_equals_the_recorded_reference(gpu, fx_remap):
    """every recorded CV_32FC2 case again through remap_flow: flow = map - grid is exact in float32 only where
    grid + flow gives the map back, so the flow is searched per value and the few that miss are skipped per case"""
    from opencv_amd import klt

    done = 0
    for i, (depth, cn, s, d, gen, kind, inter, border) in enumerate(PC.remap_cases()):
        if kind != "32fc2" or gen == "hostile":
            continue
        src, dst, m1, m2, k, bv = PC.remap_inputs(i)
        h, w = m1.shape[:2]
        grid = np.stack(np.broadcast_arrays(np.arange(w, dtype=np.float32)[None, :],
                                            np.arange(h, dtype=np.float32)[:, None]), -1)
        for sign in (1, -1):
            flow = (np.float32(sign) * (m1 - grid)).astype(np.float32)
            if not np.array_equal(R.flow_map(flow, sign), m1):
                continue
            got = klt.remap_flow(dev(src), dev(flow), sign, inter, border, bv, dst=dev(dst), ctx=gpu)
            RC.assert_pinned(got.cpu().numpy(), fx_remap[f"{i}_w"], PC.remap_label(i))
            done += 1
    assert done >= 10, done


def _hashed_flow(w, h, seed):
    """hashed noise of +-6 px, 16 bits per value"""
    return ((PC._unit(w, h, seed) - 0.5) * 12).astype(np.float32)


@pytest.mark.parametrize("w,h", [(130, 33), (640, 480)])
def test_remap_flow_is_remap_with_the_map_formed_on_the_host(gpu, w, h):
    from opencv_amd import klt

    flow = _hashed_flow(w, h, 40 + w)
    for depth, cn in (("8u", 3), ("32f", 1)):
        src = dev(PC.image(w, h, cn, depth, 41))
        for sign in (1, -1):
            m = dev(R.flow_map(flow, sign))
            for inter in (R.INTER_LINEAR, R.INTER_NEAREST):
                a = klt.remap_flow(src, dev(flow), sign, inter, R.BORDER_REFLECT_101, ctx=gpu)
                b = klt.remap(src, m, None, inter, R.BORDER_REFLECT_101, ctx=gpu)
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (depth, sign, inter)
                if (w, sign, inter) == (130, 1, R.INTER_LINEAR):  # and both are the restatement
                    want = R.remap_flow(src.cpu().numpy(), np.zeros_like(src.cpu().numpy()), flow, sign, inter,
                                        R.BORDER_REFLECT_101)
                    assert same(a, want)


def test_randomised_sweep_against_the_restatement(gpu):
    """seeded: sizes up to 320x220, all map kinds, borders and interpolations, cn 1 to 4, both depths,
    the three entry points"""
    from opencv_amd import klt

    rng = np.random.default_rng(20261020)
    gens = ("smooth", "noise", "ties", "hostile")
    for it in range(48):
        depth = ("8u", "32f")[it % 2]
        cn = 1 + (it // 2) % 4
        inter = int(rng.integers(0, 4))
        if depth == "32f" and inter == R.INTER_CUBIC:
            inter = R.INTER_LINEAR
        border = it % 6
        sw, sh = int(rng.integers(1, 321)), int(rng.integers(1, 221))
        dw, dh = int(rng.integers(1, 321)), int(rng.integers(1, 221))
        src, dst = PC.image(sw, sh, cn, depth, 100 + it), PC.image(dw, dh, cn, depth, 200 + it)
        bv = tuple(rng.uniform(-50, 300, 4))
        what = it % 5
        label = (it, depth, cn, inter, border, sw, sh, dw, dh, what)
        if what < 3:
            kind = ("32fc2", "32fc1", "16sc2f")[what]
            gen = gens[int(rng.integers(0, 4))]
            if kind == "32fc2":
                m1, m2, k = PC.float_map(gen, sw, sh, dw, dh, it), None, R.MAP_32FC2
            elif kind == "32fc1":
                m = PC.float_map(gen, sw, sh, dw, dh, it)
                m1, m2, k = np.ascontiguousarray(m[..., 0]), np.ascontiguousarray(m[..., 1]), R.MAP_32FC1
            else:
                m1, m2 = PC.fixed_map(gen, sw, sh, dw, dh, it)
                k = R.MAP_16SC2
            got = klt.remap(dev(src, it % 3), dev(m1), None if m2 is None else dev(m2), inter, border, bv,
                            dst=dev(dst, it % 4), ctx=gpu)
            want = R.remap(src, dst, m1, m2, k, inter, border, bv)
        elif what == 3:
            flow = _hashed_flow(dw, dh, 300 + it) * np.float32(3)
            sign = 1 if it % 2 else -1
            got = klt.remap_flow(dev(src, it % 3), dev(flow), sign, inter, border, bv, dst=dev(dst), ctx=gpu)
            want = R.remap_flow(src, dst, flow, sign, inter, border, bv)
        else:
            ang = rng.uniform(-0.5, 0.5)
            M = np.array([[np.cos(ang) * 1.1, -np.sin(ang), rng.uniform(-9, 9)],
                          [np.sin(ang), np.cos(ang) * 0.9, rng.uniform(-9, 9)],
                          [rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3), 1.0]])
            flags = inter | (R.WARP_INVERSE_MAP if it % 2 else 0)
            got = klt.warp_perspective(dev(src, it % 3), M, (dw, dh), flags, border, bv, dst=dev(dst), ctx=gpu)
            want = R.warp_perspective(src, dst, M, flags, border, bv)
        assert same(got, want), label


def test_end_to_end_flow_warp_on_the_basketball_pair(gpu):
    """Farneback flow A -> B on the device, then remap_flow(B, flow, +1): equal to the oracle pipeline
    (the Farneback oracle, exact-order box sums, then the numpy restatement) bit for bit, and closer to A
    than B itself is.  The oracle pipeline satisfies the inequality on this pair (checked first)."""
    from opencv_amd import farneback as FB
    from opencv_amd import klt

    d = np.load(os.path.join(GOLDEN, "basketball_pair.npz"))
    a, b = np.ascontiguousarray(d["a"]), np.ascontiguousarray(d["b"])
    ref_flow = O.farneback(a, b, box_direct=True)
    ref = R.remap_flow(b, np.zeros_like(b), ref_flow, 1, R.INTER_LINEAR, R.BORDER_REPLICATE)
    inner = (slice(16, -16), slice(16, -16))
    mad = lambda x: float(np.abs(x[inner].astype(np.int32) - a[inner].astype(np.int32)).mean())  # noqa: E731
    assert mad(ref) < mad(b), (mad(ref), mad(b))
    tb = torch.from_numpy(b).cuda()
    flow = FB.FarnebackOpticalFlow.create(ctx=gpu).calc(torch.from_numpy(a).cuda(), tb)
    got = klt.remap_flow(tb, flow, 1, klt.INTER_LINEAR, klt.BORDER_REPLICATE, ctx=gpu)
    torch.cuda.synchronize()
    assert np.array_equal(flow.cpu().numpy(), ref_flow)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert mad(got.cpu().numpy()) < mad(b)


def test_warp_perspective_with_an_affine_matrix_is_the_restatement_not_warp_affine(gpu):
    """cv::warpPerspective and cv::warpAffine round differently by design (a double division per pixel
    against a 10-bit fixed-point map), so the two kernels are not asserted equal; the count of differing
    pixels is printed for DESIGN.md"""
    from opencv_amd import klt

    src = F.pattern(130, 121, 1, 77)
    ang = np.deg2rad(7.0)
    A = np.array([[1.03 * np.cos(ang), -1.03 * np.sin(ang), 3.25], [1.03 * np.sin(ang), 1.03 * np.cos(ang), -2.5]])
    M = np.vstack([A, [0.0, 0.0, 1.0]])
    for inter in (R.INTER_NEAREST, R.INTER_LINEAR, R.INTER_CUBIC):
        got = klt.warp_perspective(dev(src), M, (130, 121), inter, R.BORDER_REFLECT_101, ctx=gpu)
        want = R.warp_perspective(src, np.zeros_like(src), M, inter, R.BORDER_REFLECT_101)
        assert same(got, want), inter
        aff = klt.warp_affine(dev(src), A, (130, 121), inter, klt.BORDER_REFLECT_101, ctx=gpu).cpu().numpy()
        print(f"warp_perspective vs warp_affine, 130x121, inter {inter}: "
              f"{int((aff != got.cpu().numpy()).sum())} of {aff.size} pixels differ")


def test_bad_arguments_and_the_empty_destination(gpu):
    from opencv_amd import _lib, klt

    src = dev(F.pattern(16, 12, 1, 1))
    m = dev(np.zeros((4, 5, 2), np.float32))
    with pytest.raises(_lib.TbdkError):  # CUBIC on 32F
        klt.remap(src.float(), m, None, klt.INTER_CUBIC, ctx=gpu)
    with pytest.raises(_lib.TbdkError):  # 16SC2 alone under LINEAR
        klt.remap(src, dev(np.zeros((4, 5, 2), np.int16)), None, klt.INTER_LINEAR, ctx=gpu)
    with pytest.raises(_lib.TbdkError):  # a non-finite matrix
        klt.warp_perspective(src, [[1, 0, 0], [0, 1, 0], [0, np.nan, 1]], (5, 4), ctx=gpu)
    with pytest.raises(_lib.TbdkError):  # aliasing
        klt.remap_flow(src, dev(np.zeros((12, 16, 2), np.float32)), dst=src, ctx=gpu)
    with pytest.raises(_lib.TbdkError):  # sign
        klt.remap_flow(src, dev(np.zeros((12, 16, 2), np.float32)), 2, ctx=gpu)
    empty = klt.warp_perspective(src, np.eye(3), (0, 4), ctx=gpu)
    assert empty.shape == (4, 0)
    # the timing names
    gpu.timing_enable(True)
    klt.remap(src, m, ctx=gpu)
    klt.remap_flow(src, dev(np.zeros((12, 16, 2), np.float32)), ctx=gpu)
    klt.warp_perspective(src, np.eye(3), (5, 4), ctx=gpu)
    torch.cuda.synchronize()
    for name in ("remap", "remap_flow", "warp_perspective"):
        assert gpu.timing_query(name)[0] >= 1, name
    gpu.timing_enable(False)
