"""The C++ facade's getGaussianKernelU8, GaussianBlur and threshold (include/tbdk.hpp) compile against libtbdk.so,
whose new entry points exist; on a GPU box the facade blurs a mask, with and without the fused threshold, thresholds
in place and runs Otsu, and the results equal the numpy restatements (which tests/test_blur_oracle.py holds to the
recorded reference).  The Python facade's argument checks that need no GPU are here too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _blur_cases as UC
import _blur_oracle as BO
from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tbdk_gaussian_kernel_u8", "tbdk_gaussian_blur_u8", "tbdk_threshold")


def build(tmp_path):
    exe = str(tmp_path / "facade_blur_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_blur_check.cpp"), "-L", libdir, "-ltbdk",
           f"-Wl,-rpath,{libdir}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def test_new_symbols_exist_in_the_library():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES
    assert lib.tbdk_abi_version() == _lib.TBDK_ABI_VERSION == 3  # no existing layout changed
    # calls without a context are bad arguments, not crashes
    assert lib.tbdk_gaussian_blur_u8(None, None, 1, 1, 1, 1, None, 1, 3, 3, 0.0, 0.0, 4, None, None) == -1
    assert lib.tbdk_threshold(None, None, 0, 1, 1, 1, 1, None, 1, 0.0, 0.0, 0, None, None, None) == -1
    assert lib.tbdk_gaussian_kernel_u8(3, 0.0, None) == -1
    assert C.sizeof(_lib.ThreshParams) == 24


def test_python_facade_without_gpu():
    import torch

    from opencv_amd import bgsegm, imgproc

    assert imgproc.get_gaussian_kernel_u8(7, 0).tolist() == [8, 28, 56, 72, 56, 28, 8]
    assert (imgproc.THRESH_BINARY, imgproc.THRESH_TOZERO_INV, imgproc.THRESH_OTSU, imgproc.BORDER_WRAP) == (0, 4, 8, 3)
    host = torch.zeros((4, 5), dtype=torch.uint8)
    for bad in (torch.zeros((4, 5), dtype=torch.int16), torch.zeros((0, 5), dtype=torch.uint8), host.t(),
                torch.zeros((2, 3, 4, 5), dtype=torch.uint8), torch.zeros((4, 5, 3), dtype=torch.uint8)[:, :, :2]):
        with pytest.raises(_lib.TbdkError):
            imgproc.gaussian_blur(bad, (3, 3), 0)
        with pytest.raises(_lib.TbdkError):
            imgproc.threshold(bad, 1, 2, 0)
    with pytest.raises(_lib.TbdkError):
        imgproc.gaussian_blur(host, (3, 3), 0, dst=torch.zeros((4, 6), dtype=torch.uint8))
    assert callable(bgsegm.smooth_mask)


def test_blur_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_blur_facade_on_gpu(tmp_path, gpu):
    exe = build(tmp_path)
    w, h = 130, 121
    mask = UC.image(w, h, "runs")
    src, out = str(tmp_path / "mask.bin"), str(tmp_path / "out.bin")
    mask.tofile(src)
    r = subprocess.run([exe, "gpu", src, out, str(w), str(h)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(out, "rb").read()
    blurred, fused, thresholded = (np.frombuffer(data, np.uint8, w * h, k * w * h).reshape(h, w) for k in range(3))
    word = int(np.frombuffer(data, np.int32, 1, 3 * w * h)[0])
    want = BO.gaussian_blur(mask, (11, 11), 3.5, 3.5)
    assert np.array_equal(blurred, want)
    assert np.array_equal(fused, BO.threshold_u8(want, 10, 255, BO.BINARY)[1]) and 0 < (fused == 255).mean() < 1
    assert np.array_equal(thresholded, BO.threshold_u8(want, 10.7, 255, BO.BINARY)[1])
    assert word == BO.otsu(want) and 0 < word < 255
