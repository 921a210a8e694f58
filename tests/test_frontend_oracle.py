"""tests/_frontend_oracle.py (numpy cvtColor / resize INTER_LINEAR) equals the
real cv::cvtColor and cv::resize on every recorded case
(tests/golden/frontend_cases.npz, recorded by tools/record_frontend_cases.py)."""
import os
import zlib

import numpy as np
import pytest

import _frontend_oracle as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_cases.npz")


@pytest.fixture(scope="module")
def cases():
    return np.load(GOLDEN)


def test_fixture_covers_the_required_cases(cases):
    cvt = {tuple(int(v) for v in r[:3]) for r in cases["cvt_meta"]}
    for size in ((97, 61), (6, 5)):
        for code in F.SRC_CN:
            assert size + (code,) in cvt
    rs = {tuple(int(v) for v in r[:5]) for r in cases["rs_meta"]}
    for sw, sh, dw, dh in ((97, 61, 31, 20), (50, 40, 123, 77), (400, 300, 320, 240), (64, 48, 32, 24),
                           (33, 7, 32, 7), (5, 5, 9, 3)):
        for cn in (1, 3, 4):
            assert (sw, sh, cn, dw, dh) in rs
    assert os.path.getsize(GOLDEN) <= 256 * 1024


def test_cvt_color_equals_recorded(cases):
    for i, (w, h, code, seed) in enumerate(cases["cvt_meta"].tolist()):
        got = F.cvt_color(F.pattern(w, h, F.SRC_CN[code], seed), code)
        assert np.array_equal(got, cases[f"cvt_{i}"]), (w, h, code)


def test_resize_linear_equals_recorded(cases):
    for i, (sw, sh, cn, dw, dh, seed, whole) in enumerate(cases["rs_meta"].tolist()):
        got = F.resize_linear(F.pattern(sw, sh, cn, seed), (dw, dh)).reshape(dh, dw * cn)
        want = cases[f"rs_{i}"]
        if whole:
            assert np.array_equal(got, want), (sw, sh, cn, dw, dh)
        else:
            crc = np.array([zlib.crc32(r.tobytes()) for r in got], np.uint32)
            bad = np.nonzero(crc != want)[0]
            assert bad.size == 0, ((sw, sh, cn, dw, dh), "rows", bad[:8])


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        F.cvt_color(np.zeros((4, 4, 3), np.uint8), 5)
    with pytest.raises(ValueError):
        F.cvt_color(np.zeros((4, 4), np.uint8), F.COLOR_BGR2GRAY)
