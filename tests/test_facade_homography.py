"""The C++ facade's tbdk::findHomography and tbdk::warpPerspectiveDeviceMatrix
(include/tbdk.hpp) compile against libtbdk.so, whose new entry points exist; on a
GPU box the facade equals the C entry, the device-matrix warp equals the
host-matrix one, and bad parameters return TBDK_EINVAL."""
import ctypes as C
import os
import subprocess

import pytest

from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "facade_homography_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_homography_check.cpp"), "-L", libdir, "-ltbdk",
           f"-Wl,-rpath,{libdir}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def test_new_symbols_exist_in_the_library():
    lib = _lib.load()
    for name in ("tbdk_find_homography", "tbdk_homography_default_params", "tbdk_warp_perspective_dev"):
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), name
    assert lib.tbdk_abi_version() == _lib.TBDK_ABI_VERSION == 3
    # the struct layouts of include/tbdk.h
    assert C.sizeof(_lib.Homography) == 88 and _lib.Homography.npoints.offset == 72
    assert C.sizeof(_lib.HomographyParams) == 40 and _lib.HomographyParams.confidence.offset == 24
    par = _lib.HomographyParams()
    assert lib.tbdk_homography_default_params(C.byref(par)) == 0
    assert (par.method, par.reproj_threshold, par.max_iters, par.confidence, par.refine) == (8, 3.0, 2000, 0.995, 1)
    # a call without a context is a bad argument, not a crash
    assert lib.tbdk_find_homography(None, None, None, None, None, 1, C.byref(par), None, None, None) == -1


def test_homography_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_homography_facade_on_gpu(tmp_path, gpu):
    exe = build(tmp_path)
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
