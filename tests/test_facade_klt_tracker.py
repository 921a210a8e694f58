"""The C++ facade's KLT point tracker (include/tbdk.hpp: tbdk::KltTracker) compiles
against libtbdk.so; on a GPU box it steps over the `small` case of
tests/_klt_tracker_oracle.py and reads what the Python binding reads."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "facade_klt_tracker_check")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_klt_tracker_check.cpp"), "-L", libdir, "-ltbdk",
           f"-Wl,-rpath,{libdir}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return exe


def test_klt_tracker_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TBDK_ENODEV" in r.stdout


@pytest.mark.gpu
def test_klt_tracker_facade_reads_what_python_reads(tmp_path, gpu):
    import torch

    import _klt_tracker_oracle as KO
    from opencv_amd import klt

    case = KO.CASES["small"]
    fr = KO.frames(case.seq)[:case.nframes]
    t = klt.KltTracker(ctx=gpu, width=fr.shape[2], height=fr.shape[1], **case.cfg)
    d = torch.from_numpy(fr).cuda()
    for f in range(case.nframes):
        t.step(d[f])
    s = t.read()
    ref = KO.run_case(case)
    assert np.array_equal(s.ids, ref.states[-1][0]) and np.array_equal(s.hist, ref.states[-1][3])
    (tmp_path / "cfg.bin").write_bytes(bytes(memoryview(t.cfg)))
    assert os.path.getsize(tmp_path / "cfg.bin") == C.sizeof(_lib.KltTrackerConfig)
    fr.tofile(tmp_path / "frames.u8")
    for name, a in (("ids", s.ids), ("lens", s.lens), ("last", s.last_pts), ("hist", s.hist)):
        a.tofile(tmp_path / f"state.{name}")
    np.array([s.stats[f[0]] for f in _lib.KltTrackerStats._fields_], np.int32).tofile(tmp_path / "state.stats")
    exe = build(tmp_path)
    r = subprocess.run([exe, "gpu", str(tmp_path / "cfg.bin"), str(tmp_path / "frames.u8"), str(case.nframes),
                        str(tmp_path / "state")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
