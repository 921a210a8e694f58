"""The C++ facade's tbdk::estimateAffine2D, tbdk::estimateAffinePartial2D and
tbdk::warpAffineDeviceMatrix (include/tbdk.hpp) compile against libtbdk.so, whose
new entry points exist with the reference's defaults; on a GPU box the facade
equals the C entry, the device-matrix warp equals the host-matrix one, and bad
parameters return TBDK_EINVAL."""
import ctypes as C
import os
import subprocess

import pytest

from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "facade_affine2d_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_affine2d_check.cpp"), "-L", libdir, "-ltbdk",
           f"-Wl,-rpath,{libdir}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def test_new_symbols_exist_in_the_library():
    lib = _lib.load()
    for name in ("tbdk_estimate_affine_2d", "tbdk_affine2d_default_params", "tbdk_warp_affine_u8_dev"):
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES
    assert lib.tbdk_abi_version() == _lib.TBDK_ABI_VERSION == 3  # no existing layout changed
    # the struct layouts of include/tbdk.h
    assert C.sizeof(_lib.Affine2D) == 64 and _lib.Affine2D.npoints.offset == 48 and _lib.Affine2D.valid.offset == 60
    assert C.sizeof(_lib.Affine2DParams) == 40
    assert (_lib.Affine2DParams.reproj_threshold.offset, _lib.Affine2DParams.confidence.offset,
            _lib.Affine2DParams.refine_iters.offset) == (8, 24, 32)
    assert (_lib.AFFINE2D_FULL, _lib.AFFINE2D_PARTIAL, _lib.AFFINE2D_RANSAC, _lib.AFFINE2D_LMEDS,
            _lib.AFFINE2D_MAX_PAIRS) == (0, 1, 8, 4, 4096)
    par = _lib.Affine2DParams()
    assert lib.tbdk_affine2d_default_params(C.byref(par)) == 0
    assert (par.model, par.method, par.reproj_threshold, par.max_iters, par.confidence, par.refine_iters) == \
        (0, 8, 3.0, 2000, 0.99, 10)  # estimateAffine2D's defaults (calib3d.hpp)
    # a call without a context is a bad argument, not a crash
    assert lib.tbdk_estimate_affine_2d(None, None, None, None, None, 1, C.byref(par), None, None, None) == -1
    assert lib.tbdk_warp_affine_u8_dev(None, None, 1, 1, 1, None, 1, 1, 1, None, None, 1, 0, 0, None) == -1


def test_affine2d_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_affine2d_facade_on_gpu(tmp_path, gpu):
    exe = build(tmp_path)
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
