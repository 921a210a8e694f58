"""CPU: opencv_amd/csrc/homography_core.hpp, the __host__ __device__ arithmetic
homography.hip's kernels call, compiled for the host into a stand-alone program
(tests/cpp/homography_core_check.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer.  It runs the full sequential algorithm over the case
table; its output is held to the numpy restatement (tests/_homography_oracle.py)
bit for bit where the numerics contract is exact (DESIGN.md §5 "findHomography":
the subset sequence, every hypothesis, iters, ninliers, the mask, the H before the
LM step) and to the recorded reference.  Host code only: nothing here touches a
GPU or is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _homography_cases as HC
import _homography_oracle as HO
from test_homography_oracle import BAR_PX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# two hostile sets after the table: NaN and infinite points must leave every loop bounded and every index inside
HOSTILE = 2


def write_cases(path, fx):
    sets = []
    for i in range(HC.NCASES):
        src, dst, st, method, thr, iters, conf = HC.fixture_inputs(fx, i)
        s, d = HC.compact(src, dst, st)
        sets.append((s, d, method, thr, iters, conf))
    s, d = (a.copy() for a in sets[8][:2])  # size 200
    s[::7, 0], d[3::11, 1], s[5::13, 1] = np.nan, np.inf, -np.inf
    sets.append((s, d, HC.RANSAC, 3.0, 40, 0.995))
    sets.append((s, d, HC.LSQ, 3.0, 40, 0.995))
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(sets)))
        for s, d, method, thr, iters, conf in sets:
            f.write(struct.pack("<3i2d", len(s), method, iters, thr, conf))
            f.write(np.ascontiguousarray(s, np.float32).tobytes())
            f.write(np.ascontiguousarray(d, np.float32).tobytes())
    return len(sets)


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("homography_core")
    exe = str(tmp / "homography_core_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cpp", "homography_core_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    cases = str(tmp / "cases.bin")
    n = write_cases(cases, HO.fixture())
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out, cur = [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = {k: v for k, v in zip(w[2::2], w[3::2])}
            out.append(cur)
        elif w[0] in ("H", "H0"):
            cur[w[0]] = np.array([int(v, 16) for v in w[1:]], np.uint64).view(np.float64)
        elif w[0] == "mask":
            cur["mask"] = np.array([int(c) for c in (w[1] if len(w) > 1 else "")], np.uint8)
        elif w[0] == "subsets":
            cur["subsets"] = [int(v) for v in w[1:]]
        elif w[0] == "hyps":
            cur["hyps"] = int(w[1], 16)
    assert len(out) == n == HC.NCASES + HOSTILE
    return out


def test_the_host_build_equals_the_restatement_bit_for_bit(host_output):
    for i in range(HC.NCASES):
        got, want = host_output[i], HO.table_result(i)
        lab = HC.label(i)
        assert int(got["valid"]) == want.valid, lab
        assert int(got["ninliers"]) == want.ninliers and int(got["iters"]) == want.iters, (lab, got["ninliers"], got["iters"])
        assert np.array_equal(got["mask"], want.mask), lab
        assert got["subsets"] == [v for s in want.subsets for v in s], lab
        assert got["hyps"] == HO.hyps_hash(want.hyps), lab
        assert got["H0"].tobytes() == np.array(want.H0, np.float64).tobytes(), lab
        if want.margins:
            assert abs(float(got["margin"]) - min(want.margins)) < 1e-9, lab
        inl = HC.compact(*HC.fixture_inputs(HO.fixture(), i)[:3])[0][want.mask != 0]
        assert HO.distance(got["H"], want.H, inl) <= BAR_PX, lab


def test_the_host_build_meets_the_recorded_reference(host_output):
    fx = HO.fixture()
    for i in range(HC.NCASES):
        got = host_output[i]
        s = HC.compact(*HC.fixture_inputs(fx, i)[:3])[0]
        valid, nin, mask, h, _ = HC.fixture_outputs(fx, i, len(s))
        assert (int(got["valid"]), int(got["ninliers"])) == (valid, nin), HC.label(i)
        assert np.array_equal(got["mask"], mask), HC.label(i)
        if valid:
            assert HO.distance(got["H"], h, s[mask != 0]) <= BAR_PX, HC.label(i)
            if len(s) == 4:  # the reference exposes the un-refined H only here: the bits
                assert got["H"].tobytes() == h.tobytes(), HC.label(i)


def test_hostile_points_end_inside_the_bounds(host_output):
    # the sanitizers and the exit code are the check; what H such points give is unspecified
    for got in host_output[HC.NCASES:]:
        assert int(got["iters"]) <= 40 and len(got["mask"]) == 200
