#!/usr/bin/env python3
"""Generates the point sets of tests/golden/rigid_transform_cases.npz and
records the real cv::estimateRigidTransform on them through
tools/rigid_transform_driver.cpp (how to build it: tools/record_rigid_cases.md).

    python tools/record_rigid_cases.py /path/to/rigid_transform_driver [out.npz]

Nothing in the test suite runs this; the fixture is committed."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def similarity_set(rng, n, outlier_frac, noise=0.3):
    x, y = rng.uniform(0, 1700), rng.uniform(0, 900)
    w, h = int(rng.integers(20, 220)), int(rng.integers(20, 220))
    a = np.stack([rng.uniform(x, x + w, n), rng.uniform(y, y + h, n)], 1)
    ang, s = rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.1)
    R = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    b = a @ R.T + rng.uniform(-8, 8, 2) + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outlier_frac
    b[out] += rng.uniform(-40, 40, (int(out.sum()), 2))
    return a.astype(np.float32), b.astype(np.float32)


def make_cases():
    rng = np.random.default_rng(20261019)
    cases = []  # (a, b, max_iters, good_ratio)
    fr = [0.0, 0.2, 0.4, 0.6, 0.9]
    for i in range(48):  # random similarity sets, every outlier fraction
        n = int(rng.integers(3, 65))
        cases.append((*similarity_set(rng, n, fr[i % 5]), 500, 0.5))
    for n in (0, 1, 2, 3, 4, 5):  # tiny sets (0: the reference throws)
        cases.append((*similarity_set(rng, n, 0.0), 500, 0.5))
    for mi, gr in ((20, 0.8), (500, 0.3), (3, 0.5), (1, 0.0)):  # the 6-argument overload
        cases.append((*similarity_set(rng, 40, 0.4), mi, gr))
    p = rng.uniform(100, 200, (1, 2)).astype(np.float32)
    cases.append((np.repeat(p, 12, 0), np.repeat(p + 2, 12, 0), 500, 0.5))  # coincident
    cases.append((np.repeat(p, 5, 0), np.repeat(p + 2, 5, 0), 50, 0.5))
    t = np.arange(20, dtype=np.float32)[:, None]
    line = np.concatenate([100 + 4 * t, 50 + 2 * t], 1).astype(np.float32)  # exactly collinear (integers)
    cases.append((line, line + np.float32(3), 50, 0.5))
    two = np.array([[10, 10], [90, 40]], np.float32)[np.arange(16) % 2]  # two distinct points repeated
    cases.append((two, two + np.float32(1), 50, 0.5))
    a, b = similarity_set(rng, 30, 0.0)
    b[:] = b[0]  # one point set coincident, the other spread
    cases.append((a, b, 50, 0.5))
    a, b = similarity_set(rng, 64, 0.0)
    b += rng.uniform(-40, 40, b.shape).astype(np.float32)  # no consensus: every pair an outlier
    cases.append((a, b, 60, 0.5))
    for f in (0.0, 0.4, 0.6, 0.9):  # the loop's slot size
        cases.append((*similarity_set(rng, 256, f), 500, 0.5))
    return cases


def main():
    driver = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "rigid_transform_cases.npz")
    cases = make_cases()
    lines = [str(len(cases))]
    for a, b, mi, gr in cases:
        lines.append(f"{len(a)} {mi} {gr!r}")
        lines += [f"{p[0]:.9g} {p[1]:.9g} {q[0]:.9g} {q[1]:.9g}" for p, q in zip(a, b)]
    txt = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in txt.strip().splitlines()]
    assert len(rows) == len(cases)
    found = np.array([int(r[0]) for r in rows], np.uint8)
    M = np.array([[float(v) for v in r[1:]] for r in rows], np.float64)
    offs = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int32)
    cat = lambda k: np.concatenate([c[k].reshape(-1, 2) for c in cases]).astype(np.float32)  # noqa: E731
    np.savez_compressed(out, a=cat(0), b=cat(1), offsets=offs, max_iters=np.array([c[2] for c in cases], np.int32),
                        good_ratio=np.array([c[3] for c in cases], np.float64), found=found, M=M)
    print(f"{out}: {len(cases)} cases, {offs[-1]} points, {int(found.sum())} with a transform, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
