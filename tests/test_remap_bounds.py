"""CPU: the address computation of the remap kernels (opencv_amd/csrc/remap_core.hpp,
the __host__ __device__ functions remap.hip calls) never indexes outside the source,
whatever a map holds.  A stand-alone host program (tests/cpp/remap_bounds_check.cpp)
built with AddressSanitizer and UndefinedBehaviorSanitizer walks every case of
tests/_remap_cases.py, the hostile maps included, through those functions; it also
holds border_interp's closed form to the reference's loop.  Host code only: nothing
here touches a GPU or is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _remap_cases as PC
import _remap_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT_FLOW, FRONT_PERSPECTIVE = 3, 4


def _record(f, front, inter, border, sw, sh, dw, dh, m, map1=None, map2=None, sign=1):
    b1 = b"" if map1 is None else np.ascontiguousarray(map1).tobytes()
    b2 = b"" if map2 is None else np.ascontiguousarray(map2).tobytes()
    f.write(struct.pack("<12i", front, inter, border, sw, sh, dw, dh, int(map2 is not None), sign, len(b1), len(b2), 0))
    f.write(np.asarray(m, np.float64).reshape(9).tobytes())
    f.write(b1)
    f.write(b2)


def write_cases(path):
    n = 0
    with open(path, "wb") as f:
        for i, (depth, cn, s, d, gen, kind, inter, border) in enumerate(PC.remap_cases()):
            src, dst, m1, m2, k, _ = PC.remap_inputs(i)
            _record(f, k, inter, border, src.shape[1], src.shape[0], dst.shape[1], dst.shape[0], np.zeros(9), m1, m2)
            n += 1
            if k == R.MAP_32FC2:  # the same values as a flow, both signs
                for sign in (1, -1):
                    _record(f, FRONT_FLOW, inter, border, src.shape[1], src.shape[0], dst.shape[1], dst.shape[0],
                            np.zeros(9), m1, None, sign)
                    n += 1
        for i, (depth, cn, s, d, name, flags, border) in enumerate(PC.persp_cases()):
            src, dst, M, _ = PC.persp_inputs(i)
            m = M if flags & R.WARP_INVERSE_MAP else R.invert3x3(M)
            _record(f, FRONT_PERSPECTIVE, flags & 7, border, src.shape[1], src.shape[0], dst.shape[1], dst.shape[0], m)
            n += 1
    return n


def test_address_functions_stay_inside_the_source_under_sanitizers(tmp_path):
    exe = str(tmp_path / "remap_bounds_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "opencv_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "remap_bounds_check.cpp"),
           "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    cases = str(tmp_path / "cases.bin")
    n = write_cases(cases)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"cases {n} " in r.stdout and "outside 0" in r.stdout, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
