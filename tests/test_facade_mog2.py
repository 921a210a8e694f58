"""The C++ facade's tbdk::BackgroundSubtractorMOG2 (include/tbdk.hpp) compiles against libtbdk.so, whose new
entry points exist with the reference's defaults; on a GPU box the class, fed the gray base sequence, returns
the masks and the final background image the real reference returned (tests/golden/reference_mog2.npz)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mog2_cases as GC
import _reference_cases as RC
from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tbdk_mog2_config_default", "tbdk_mog2_create", "tbdk_mog2_destroy", "tbdk_mog2_reset",
           "tbdk_mog2_set_params", "tbdk_mog2_apply", "tbdk_mog2_get_background", "tbdk_mog2_get_model",
           "tbdk_mog2_frames")


def build(tmp_path):
    exe = str(tmp_path / "facade_mog2_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_mog2_check.cpp"), "-L", libdir, "-ltbdk",
           f"-Wl,-rpath,{libdir}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def test_new_symbols_exist_in_the_library():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES
    assert lib.tbdk_abi_version() == _lib.TBDK_ABI_VERSION == 3  # no existing layout changed
    assert C.sizeof(_lib.Mog2Config) == 72
    assert (_lib.Mog2Config.var_threshold.offset, _lib.Mog2Config.var_threshold_gen.offset,
            _lib.Mog2Config.shadow_threshold.offset) == (32, 40, 64)
    cfg = _lib.Mog2Config()
    assert lib.tbdk_mog2_config_default(64, 48, 5, 3, C.byref(cfg)) == 0
    got = {k: getattr(cfg, k) for k in GC.PARAM_KEYS}
    want = {k: (np.float32(v) if isinstance(v, float) and k != "var_threshold" else v) for k, v in GC.DEFAULTS.items()}
    assert got == want  # bgfg_gaussmix2.cpp:106-118
    assert (cfg.width, cfg.height, cfg.depth, cfg.channels) == (64, 48, 5, 3)
    # calls without an object are bad arguments, not crashes
    assert lib.tbdk_mog2_create(None, C.byref(cfg), None) == -1
    assert lib.tbdk_mog2_apply(None, None, 0, None, 0, -1.0, None) == -1
    assert lib.tbdk_mog2_get_background(None, None, 0, None) == -1
    assert lib.tbdk_mog2_get_model(None, None, None, None, None, None) == -1
    assert lib.tbdk_mog2_reset(None) == lib.tbdk_mog2_destroy(None) == lib.tbdk_mog2_frames(None, None) == -1


def test_mog2_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_mog2_facade_on_gpu(tmp_path, gpu):
    exe = build(tmp_path)
    i = 0  # 8UC1 history 12
    case = GC.cases()[i]
    assert case["name"] == "8UC1 history 12" and case["whole"]
    w, h, n = case["w"], case["h"], case["n"]
    frames, out = str(tmp_path / "frames.bin"), str(tmp_path / "out.bin")
    GC.case_frames(case).tofile(frames)
    r = subprocess.run([exe, "gpu", frames, out, str(w), str(h), str(n), "12"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = np.fromfile(out, np.uint8)
    masks, bg = data[:n * h * w].reshape(n, h, w), data[n * h * w:].reshape(h, w)
    fx = RC.fixture("mog2")
    want = GC.unpack_masks(fx[f"{i}_masks"], n, h, w, 127)
    bad = [t for t in range(n) if not np.array_equal(masks[t], want[t])]
    assert not bad, bad[:8]
    assert np.array_equal(bg, fx[f"{i}_bg{n}"])
