"""The C++ facade's tbdk::remap, tbdk::remapFlow and tbdk::warpPerspective
(include/tbdk.hpp) compile against libtbdk.so, whose new entry points exist; on a
GPU box the facade equals the C entries and bad arguments return TBDK_EINVAL."""
import ctypes as C
import os
import subprocess

import pytest

from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "facade_remap_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_remap_check.cpp"), "-L", libdir, "-ltbdk",
           f"-Wl,-rpath,{libdir}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def test_new_symbols_exist_in_the_library():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("tbdk_remap", "tbdk_remap_flow", "tbdk_warp_perspective", "tbdk_warp_perspective_invert"):
        assert hasattr(lib, name), name
    # a call without a context is a bad argument, not a crash
    lib.tbdk_remap_flow.restype = C.c_int
    assert _lib.load().tbdk_remap_flow(None, None, 0, 1, 4, 4, 4, None, 4, 4, 4, None, 32, 1, 1, 0, None, None) == -1


def test_remap_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_remap_facade_on_gpu(tmp_path, gpu):
    exe = build(tmp_path)
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
