"""CPU: opencv_amd/csrc/mog2_core.hpp, the __host__ __device__ arithmetic mog2.hip's kernels call, compiled for
the host into a stand-alone program (tests/cpp/mog2_core_check.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer.  Over every recorded case its masks, background images and the full model after the
last frame equal the restatement (tests/_mog2_oracle.py) bit for bit, and so do its branch counts.  Hostile 32F
frames must end cleanly with modes_used inside 0..nmixtures.  Host code only: nothing here touches a GPU or is
loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _mog2_cases as GC
import _mog2_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = ("var_threshold", "var_threshold_gen", "var_init", "var_min", "var_max", "background_ratio",
       "complexity_reduction", "shadow_threshold")


def hostile_cases():
    """32F frames of NaN, +-inf, +-1e30 and subnormals among ordinary values, one and three channels, and one of
    nothing but NaN; the learning rates include 0 and a re-initialisation"""
    out = []
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40, -1e-42, 0.0, 100.0, 3.5], np.float32)
    for cn, k in ((1, 5), (3, 8), (3, 1)):
        n, h, w = 12, 9, 13
        idx = GC.pattern(w * cn, h * n, 1, 4100 + cn).astype(np.int64).reshape(n, h, w, cn) % len(vals)
        fr = vals[idx] if cn == 3 else vals[idx][..., 0]
        rates = np.full(n, -1.0)
        rates[5], rates[8] = 0.0, 1.0
        out.append(dict(name=f"hostile cn {cn} K {k}", w=w, h=h, n=n, cn=cn, rates=rates, bg=(3, n),
                        params=dict(nmixtures=k, history=7)), )
        out[-1]["frames"] = np.ascontiguousarray(fr, np.float32)
    nan = dict(name="all NaN", w=5, h=3, n=6, cn=1, rates=np.full(6, -1.0), bg=(6,), params=dict(history=3))
    nan["frames"] = np.full((6, 3, 5), np.nan, np.float32)
    out.append(nan)
    return out


def write_cases(path, rows):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(rows)))
        for case in rows:
            p = dict(GC.DEFAULTS)
            p.update(case["params"])
            fr = case["frames"] if "frames" in case else GC.case_frames(case)
            f.write(struct.pack("<9i", case["w"], case["h"], case["cn"], int(fr.dtype == np.float32), case["n"],
                                p["history"], p["nmixtures"], p["detect_shadows"], p["shadow_value"]))
            f.write(struct.pack("<8d", *[float(p[k]) for k in PAR]))
            f.write(np.asarray(case["rates"], np.float64).tobytes())
            f.write(bytes(int(t + 1 in case["bg"]) for t in range(case["n"])))
            f.write(np.ascontiguousarray(fr).tobytes())


def read_results(path, rows):
    data = open(path, "rb").read()
    pos, out = 0, []

    def take(count, dt):
        nonlocal pos
        a = np.frombuffer(data, dt, count, pos)
        pos += a.nbytes
        return a

    for case in rows:
        p = dict(GC.DEFAULTS)
        p.update(case["params"])
        w, h, cn, n, k = case["w"], case["h"], case["cn"], case["n"], p["nmixtures"]
        f32 = "frames" in case or case["content"] != "u8"
        masks = take(n * h * w, np.uint8).reshape(n, h, w)
        shape = (h, w) if cn == 1 else (h, w, 3)
        bgs = {t: take(h * w * cn, np.float32 if f32 else np.uint8).reshape(shape) for t in case["bg"]}
        model = (take(h * w * k, np.float32).reshape(h, w, k), take(h * w * k, np.float32).reshape(h, w, k),
                 take(h * w * k * cn, np.float32).reshape(h, w, k, cn), take(h * w, np.uint8).reshape(h, w))
        counts = dict(zip(MO.EVENTS, take(11, np.int64).tolist()))
        out.append((masks, bgs, model, counts))
    assert pos == len(data)
    return out


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mog2_core")
    exe = str(tmp / "mog2_core_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cpp", "mog2_core_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    rows = GC.cases() + hostile_cases()
    cases, res = str(tmp / "cases.bin"), str(tmp / "out.bin")
    write_cases(cases, rows)
    r = subprocess.run([exe, cases, res], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.split() == ["cases", str(len(rows))]
    return rows, read_results(res, rows)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("i", range(GC.NCASES))
def test_the_host_build_equals_the_restatement_bit_for_bit(host_output, i):
    rows, res = host_output
    masks, bgs, model, counts = res[i]
    wm, wb, wmodel, wcounts = MO.expected(i)
    lab = rows[i]["name"]
    assert np.array_equal(masks, wm), lab
    for t in rows[i]["bg"]:
        assert bgs[t].dtype == wb[t].dtype and np.array_equal(bits(bgs[t]), bits(wb[t])), (lab, t)
    for name, got, want in zip(("weight", "variance", "mean", "modes_used"), model, wmodel):
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (lab, name)
    assert counts == wcounts, lab


def test_hostile_frames_end_inside_the_bounds(host_output):
    # the sanitizers and the exit code are the check; what such pixels classify as is unspecified
    rows, res = host_output
    assert len(rows) == GC.NCASES + 4
    for case, (masks, _, model, _) in zip(rows[GC.NCASES:], res[GC.NCASES:]):
        k = dict(GC.DEFAULTS, **case["params"])["nmixtures"]
        assert model[3].max() <= k, case["name"]
        assert np.isin(masks, (0, 127, 255)).all(), case["name"]
