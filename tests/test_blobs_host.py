"""CPU: opencv_amd/csrc/morph_host.hpp, the host side of tbdk_morph_u8 and tbdk_structuring_element
(getStructuringElement, anchor normalisation, morphOp's iteration-merge rule), compiled into a stand-alone program
(tests/cpp/blobs_host_check.cpp) with AddressSanitizer and UndefinedBehaviorSanitizer.  Its elements equal the
recordings of the real getStructuringElement (tests/golden/reference_morph.npz), its plans the rules as
tests/_morph_oracle.py restates them.  Host code only: nothing here touches a GPU or is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _morph_cases as BC
import _morph_oracle as MO
import _reference_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAD_ELEMENTS = [(3, 3, 3, -1, -1), (-1, 3, 3, -1, -1), (0, 0, 3, -1, -1), (0, 3, -2, -1, -1), (1, 3, 3, 3, 0),
                (1, 3, 3, 0, -2), (2, 5, 5, 5, 5)]


def element_cases():
    rows = [(shape, kw, kh, a[0], a[1]) for shape, kw, kh, a in BC.strel_cases()]
    rows += [(shape, kw, kh, -1, -1) for shape in (0, 1, 2) for kw, kh in ((1, 1), (2, 1), (1, 2), (64, 3), (3, 64), (33, 33))]
    return rows + BAD_ELEMENTS


def plan_cases():
    """(element or None, anchor, iterations)"""
    el = BC.elements()
    rows = []
    for c in BC.cases():
        rows.append((el[c["elem"]], c["anchor"], c["it"]))
    ones = np.ones((3, 3), np.uint8)
    rows += [(None, (-1, -1), 16), (ones, (-1, -1), 16), (ones, (-1, -1), 15), (None, (-1, -1), 15),
             (np.ones((1, 32), np.uint8), (-1, -1), 1), (np.ones((32, 1), np.uint8), (-1, -1), 1),
             (np.ones((17, 17), np.uint8), (-1, -1), 2), (np.ones((16, 16), np.uint8), (15, 0), 2),
             (np.zeros((3, 3), np.uint8), (-1, -1), 1), (np.zeros((1, 1), np.uint8), (-1, -1), 1),
             (np.zeros((3, 3), np.uint8), (-1, -1), 0), (ones, (3, 0), 1), (ones, (0, -2), 1), (ones, (-1, 2), 1),
             (ones, (-1, -1), -1), (el["arb5x4"], (4, 3), 64), (np.ones((31, 31), np.uint8), (30, 30), 1),
             (np.ones((1, 1), np.uint8), (-1, -1), 100), (np.ones((1, 3), np.uint8), (-1, -1), 16)]
    return rows


def expected_plan(elem, anchor, it):
    """the rules of morphOp (morph.dispatch.cpp:952-972) as tests/_morph_oracle.py has them, as the plan's fields;
    None where the entry point refuses"""
    kh, kw = (3, 3) if elem is None else elem.shape
    if it < 0:
        return None
    ax = kw // 2 if anchor[0] == -1 else anchor[0]
    ay = kh // 2 if anchor[1] == -1 else anchor[1]
    if not (0 <= ax < kw and 0 <= ay < kh):
        return None
    if it == 0 or (elem is not None and kw * kh == 1):
        return dict(copy=1, rect=0, kw=1, kh=1, ax=0, ay=0, passes=0, rows=[1])
    if elem is not None and not elem.any():
        return None
    rect = elem is None or bool(elem.all())
    passes = it
    if elem is None:
        kw = kh = 1 + 2 * it
        ax = ay = it
        passes = 1
    elif it > 1 and rect:
        kw, kh, ax, ay, passes = kw + (it - 1) * (kw - 1), kh + (it - 1) * (kh - 1), ax * it, ay * it, 1
    if kw > 31 or kh > 31:
        return None
    e = np.ones((kh, kw), np.uint8) if rect else elem
    return dict(copy=0, rect=int(rect), kw=kw, kh=kh, ax=ax, ay=ay, passes=passes,
                rows=[int(sum(1 << j for j in range(kw) if e[i, j])) for i in range(kh)])


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("blobs_host")
    exe = str(tmp / "blobs_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cpp", "blobs_host_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    elems, plans = element_cases(), plan_cases()
    cases, res = str(tmp / "cases.bin"), str(tmp / "out.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<i", len(elems) + len(plans)))
        for row in elems:
            f.write(struct.pack("<6i", 0, *row))
        for elem, anchor, it in plans:
            kh, kw = (3, 3) if elem is None else elem.shape
            f.write(struct.pack("<7i", 1, int(elem is not None), kw, kh, anchor[0], anchor[1], it))
            if elem is not None:
                f.write(np.ascontiguousarray(elem, np.uint8).tobytes())
    r = subprocess.run([exe, cases, res], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.split() == ["cases", str(len(elems) + len(plans))]
    data, pos = open(res, "rb").read(), 0
    got_e, got_p = [], []
    for shape, kw, kh, ax, ay in elems:
        ok = struct.unpack_from("<i", data, pos)[0]
        pos += 4
        got_e.append(np.frombuffer(data, np.uint8, kw * kh, pos).reshape(kh, kw) if ok else None)
        pos += kw * kh if ok else 0
    for _ in plans:
        head = struct.unpack_from("<8i", data, pos)
        rows = struct.unpack_from("<31I", data, pos + 32)
        pos += 32 + 124
        got_p.append((head, rows))
    assert pos == len(data)
    return elems, got_e, plans, got_p


def test_structuring_elements_equal_the_recorded_reference(host_output):
    elems, got, _, _ = host_output
    fx = RC.fixture("morph")
    nrec = len(BC.strel_cases())
    for k, ((shape, kw, kh, ax, ay), e) in enumerate(zip(elems, got)):
        if (shape, kw, kh, ax, ay) in BAD_ELEMENTS:
            assert e is None, (shape, kw, kh, ax, ay)
            continue
        assert e is not None and np.isin(e, (0, 1)).all(), (shape, kw, kh)
        if k < nrec:
            assert np.array_equal(np.packbits(e), fx[f"strel_{k}"]), (shape, kw, kh, ax, ay)
        assert np.array_equal(e, MO.structuring_element(shape, (kw, kh), (ax, ay))), (shape, kw, kh, ax, ay)


def test_anchor_and_iteration_rules(host_output):
    _, _, plans, got = host_output
    refused = 0
    for (elem, anchor, it), (head, rows) in zip(plans, got):
        want = expected_plan(elem, anchor, it)
        what = (None if elem is None else elem.shape, anchor, it)
        if want is None:
            assert head[0] == 0, what
            refused += 1
            continue
        assert head[0] == 1, what
        assert dict(zip(("copy", "rect", "kw", "kh", "ax", "ay", "passes"), head[1:])) == \
            {k: v for k, v in want.items() if k != "rows"} or (want["copy"] and head[1] == 1), what
        if not want["copy"]:
            assert list(rows[:want["kh"]]) == want["rows"] and not any(rows[want["kh"]:]), what
    assert refused == 10
    # the limit: the 3x3 rectangle at 15 iterations is one 31 x 31 pass, at 16 it is refused
    assert expected_plan(None, (-1, -1), 15)["kw"] == 31 and expected_plan(None, (-1, -1), 16) is None
