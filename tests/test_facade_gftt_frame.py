"""The C++ facade's whole-frame corner detection (include/tbdk.hpp:
CornersDetector::detect) compiles against libtbdk.so; on a GPU box it detects on
the 1242 x 375 frame of tests/_gftt_frame_cases.py, which has more candidates than
the LDS selection holds, and returns the list the Python binding returns."""
import os
import subprocess

import numpy as np
import pytest

from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "facade_gftt_frame_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_gftt_frame_check.cpp"), "-L", libdir, "-ltbdk",
           f"-Wl,-rpath,{libdir}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def test_frame_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_frame_facade_detects_what_python_detects(tmp_path, gpu):
    import torch

    import _gftt_frame_cases as WC
    from opencv_amd import klt

    img = np.array(WC.frame("kitti"))
    maxc, q, md = 4000, 0.01, 1.5
    c = klt.GoodFeaturesToTrackDetector(maxc, q, md).detect(torch.from_numpy(img).cuda())
    torch.cuda.synchronize()
    c = c.cpu().numpy()
    assert len(c) == maxc
    assert np.array_equal(c, WC.corners(WC.fixture(), WC.index("kitti", "none", maxc, q, md)))
    img.tofile(tmp_path / "frame.u8")
    c.tofile(tmp_path / "corners.f32")
    exe = build(tmp_path)
    r = subprocess.run([exe, "gpu", str(tmp_path / "frame.u8"), str(img.shape[1]), str(img.shape[0]), str(maxc),
                        repr(q), repr(md), str(tmp_path / "corners.f32")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
