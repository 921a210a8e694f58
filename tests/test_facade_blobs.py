"""The C++ facade's getStructuringElement, erode, dilate, morphologyEx, connectedComponents and
connectedComponentsWithStats (include/tbdk.hpp) compile against libtbdk.so, whose new entry points exist; on a GPU
box the facade opens a mask in place and labels it, and the results equal the numpy restatements (which
tests/test_morph_oracle.py and tests/test_cc_oracle.py hold to the recorded reference)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _cc_cases as LC
import _cc_oracle as CO
import _morph_oracle as MO
from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tbdk_structuring_element", "tbdk_morph_u8", "tbdk_connected_components")


def build(tmp_path):
    exe = str(tmp_path / "facade_blobs_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_blobs_check.cpp"), "-L", libdir, "-ltbdk",
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
    assert lib.tbdk_morph_u8(None, 0, None, 1, 1, 1, None, 1, None, 3, 3, -1, -1, 1, 0, -1, None) == -1
    assert lib.tbdk_connected_components(None, None, 1, 1, 1, None, 4, 8, -1, None, None, 0, None, None) == -1
    assert lib.tbdk_structuring_element(0, 3, 3, -1, -1, None) == -1


def test_python_facade_elements_without_gpu():
    from opencv_amd import imgproc

    for shape in (imgproc.MORPH_RECT, imgproc.MORPH_CROSS, imgproc.MORPH_ELLIPSE):
        for ksize in ((1, 1), (3, 3), (9, 5), (4, 6), (31, 31)):
            assert np.array_equal(imgproc.get_structuring_element(shape, ksize), MO.structuring_element(shape, ksize))
    with pytest.raises(_lib.TbdkError):
        imgproc.get_structuring_element(3, (3, 3))
    with pytest.raises(_lib.TbdkError):
        imgproc.get_structuring_element(imgproc.MORPH_CROSS, (3, 3), (3, 0))


def test_detections_from_stats_without_gpu():
    import torch

    from opencv_amd import bgsegm, tbd

    stats = torch.tensor([[0, 0, 64, 48, 3000], [3, 4, 5, 6, 20], [10, 11, 2, 2, 4], [20, 21, 9, 9, 70],
                          [-1, -1, -1, -1, -1]], dtype=torch.int32)
    d = bgsegm.detections_from_stats(stats, torch.tensor([4], dtype=torch.int32), min_area=6)
    assert d.dtype == tbd.DET_DTYPE and d["id"].tolist() == [1, 3]
    assert [tuple(r) for r in d[["x", "y", "width", "height"]].tolist()] == [(3, 4, 5, 6), (20, 21, 9, 9)]
    assert d["confidence"].tolist() == [1.0, 1.0]
    assert bgsegm.detections_from_stats(stats, 4, min_area=1, max_area=20)["id"].tolist() == [1, 2]
    assert len(bgsegm.detections_from_stats(stats, 1)) == 0 and len(bgsegm.detections_from_stats(stats[:2], 4)) == 1


def test_blobs_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_blobs_facade_on_gpu(tmp_path, gpu):
    exe = build(tmp_path)
    w, h, cap = 130, 121, 128
    mask = LC.image("noise0.6", w, h)
    src, out = str(tmp_path / "mask.bin"), str(tmp_path / "out.bin")
    mask.tofile(src)
    r = subprocess.run([exe, "gpu", src, out, str(w), str(h), str(cap)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(out, "rb").read()
    opened = np.frombuffer(data, np.uint8, w * h).reshape(h, w)
    n = int(np.frombuffer(data, np.int32, 1, w * h)[0])
    labels = np.frombuffer(data, np.int32, w * h, w * h + 4).reshape(h, w)
    stats = np.frombuffer(data, np.int32, cap * 5, w * h * 5 + 4).reshape(cap, 5)
    cent = np.frombuffer(data, np.float64, cap * 2, w * h * 5 + 4 + cap * 20).reshape(cap, 2)
    want = MO.morphology_ex(mask, MO.OPEN, np.ones((3, 3), np.uint8))
    assert np.array_equal(opened, want)
    rn, rlabels, rstats, rcent = CO.connected_components_with_stats(want, 8, CO.CCL_DEFAULT)
    assert n == rn and 2 < n <= cap and np.array_equal(labels, rlabels)
    assert np.array_equal(stats[:n], rstats) and CO.same_centroids(cent[:n], rcent)
    assert (stats[n:] == 0x11111111).all() and (cent[n:].view(np.uint64) == 0x1111111111111111).all()
