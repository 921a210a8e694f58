"""CPU: opencv_amd/csrc/knn_core.hpp, the __host__ __device__ arithmetic knn.hip's kernels call, compiled for the
host into a stand-alone program (tests/cpp/knn_core_check.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer.  Over every recorded case its masks, background images, the full model, the counters,
the RNG state after the last frame, the periods and the branch counts equal the restatement
(tests/_knn_oracle.py) bit for bit; every fill is made block by block from jump-ahead starts, as the kernel makes
it, and must equal the sequential one.  The jump-ahead is held against sequential stepping for 10^5 random
(state, n), at the two fixed points and at a constructed ambiguous start.  Host code only: nothing here touches a
GPU or is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _knn_cases as KC
import _knn_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 100000


def write_cases(path, rows):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(rows)))
        for case in rows:
            p = KC.params(case)
            f.write(struct.pack("<9i", case["w"], case["h"], case["cn"], case["n"], p["history"], p["nsamples"],
                                p["knn_samples"], p["detect_shadows"], p["shadow_value"]))
            f.write(struct.pack("<2f", p["dist2_threshold"], p["shadow_threshold"]))
            f.write(struct.pack("<Q", p["rng_state"]))
            f.write(np.asarray(case["rates"], np.float64).tobytes())
            f.write(bytes(int(t + 1 in case["bg"]) for t in range(case["n"])))
            f.write(np.ascontiguousarray(KC.case_frames(case)).tobytes())


def read_results(path, rows):
    data = open(path, "rb").read()
    pos, out = 0, []

    def take(count, dt):
        nonlocal pos
        a = np.frombuffer(data, dt, count, pos)
        pos += a.nbytes
        return a

    for case in rows:
        w, h, cn, n, k = case["w"], case["h"], case["cn"], case["n"], KC.params(case)["nsamples"]
        masks = take(n * h * w, np.uint8).reshape(n, h, w)
        shape = (h, w) if cn == 1 else (h, w, 3)
        bgs = {t: take(h * w * cn, np.uint8).reshape(shape) for t in case["bg"]}
        model = (take(h * w * 3 * k * (cn + 1), np.uint8).reshape(h, w, 3 * k, cn + 1),
                 take(3 * h * w, np.uint8).reshape(3, h, w), take(3 * h * w, np.uint8).reshape(3, h, w),
                 take(3, np.int32), int(take(1, np.uint64)[0]))
        counts = dict(zip(KO.COUNT_KEYS, take(11, np.int64).tolist()))
        periods = take(3 * n, np.int32).reshape(n, 3)
        out.append((masks, bgs, model, counts, periods))
    assert pos == len(data)
    return out


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("knn_core")
    exe = str(tmp / "knn_core_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cpp", "knn_core_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return tmp, exe


def run_clean(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout.split()


@pytest.fixture(scope="module")
def host_output(host_program):
    tmp, exe = host_program
    rows = KC.cases()
    cases, res = str(tmp / "cases.bin"), str(tmp / "out.bin")
    write_cases(cases, rows)
    assert run_clean([exe, "cases", cases, res]) == ["cases", str(len(rows))]
    return rows, read_results(res, rows)


@pytest.mark.parametrize("i", range(KC.NCASES))
def test_the_host_build_equals_the_restatement_bit_for_bit(host_output, i):
    rows, res = host_output
    masks, bgs, model, counts, periods = res[i]
    wm, wb, wmodel, wcounts, wperiods, _ = KO.expected(i)
    lab = rows[i]["name"]
    assert np.array_equal(masks, wm), lab
    for t in rows[i]["bg"]:
        assert bgs[t].shape == wb[t].shape and np.array_equal(bgs[t], wb[t]), (lab, t)
    for name, got, want in zip(("samples", "index", "next", "counters"), model, wmodel):
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (lab, name)
    assert model[4] == wmodel[4], (lab, "rng state", hex(model[4]), hex(wmodel[4]))
    assert counts == wcounts, lab
    assert np.array_equal(periods, wperiods), lab


def test_the_jump_ahead_equals_stepping(host_program):
    """10^5 random (state, n) with n up to 4096, states above m and with small residues among them; the block form
    and the shift-and-subtract reduction; 0 and m stay; the successor of 0xf83f630effffffff is m + 5, a residue
    that is also a state, and the fallback returns m + 5"""
    _, exe = host_program
    assert run_clean([exe, "jump", str(PAIRS)]) == ["jump", "ok", str(PAIRS)]
