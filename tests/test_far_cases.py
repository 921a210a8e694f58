"""The conditions of tests/test_gpu_far_views.py's case table, from the tables and
include/tbdk.h alone (no GPU): every pitch parameter of the header has a case
that puts its image far (or an exclusion that cites the header: host memory
only); the layouts' arithmetic is as tests/_far.py claims; the rectangles of a
case keep apart, also from each other's rows shifted by 2^31 and 2^32, and fit
the arena; every cited header line exists and names a bound; no case expects a
rejection under `under_2g`."""
import os
import re

import numpy as np
import pytest

import _far as F
import _far_table as FT

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tbdk.h")


def pitch_parameters():
    """(symbol, parameter) for every parameter of a tbdk_* function whose name ends in `pitch`"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = []
    for m in re.finditer(r"\bint\s+(tbdk_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        for p in re.findall(r"\bint\s+(\w*pitch)\b", m.group(2)):
            out.append((m.group(1), p))
    return out


def header_text():
    return re.sub(r"\s+", " ", " ".join(re.sub(r"^\s*/?\*+/?", "", ln).strip() for ln in open(HEADER).read().splitlines()))


def test_every_pitch_parameter_has_a_case():
    params = pitch_parameters()
    assert len(params) >= 75 and ("tbdk_pyr_build", "pitch") in params and ("tbdk_remap", "map2_pitch") in params
    cased = {p for c in FT.CASES for p in c.covers}
    named = cased | set(FT.EXCLUDED)
    assert not set(params) - named, f"pitch parameters with neither a case nor an exclusion: {sorted(set(params) - named)}"
    assert not named - set(params), f"the table names parameters the header does not have: {sorted(named - set(params))}"
    assert not cased & set(FT.EXCLUDED)
    text = header_text()
    for key, why in FT.EXCLUDED.items():  # host memory only, and the header says so
        assert "host" in why and key[0] in why
        for quote in re.findall(r"\"(.*?)\"", why):
            assert re.sub(r"\s+", " ", quote) in text, (key, quote)
    # an image alone in its role: a case whose far images are exactly those under that one parameter
    for c in FT.CASES:
        assert c.far and c.covers and len(set(c.share.values())) <= 1, c.name
        assert len(c.covers) == 1 or c.share or c.name == "morph_in_place", c.name


def geometry(fc, i):
    return [(n, s[0], int(np.prod(s[1:])) * dt.itemsize, u) for n, s, dt, u in fc.images(i)]


@pytest.mark.parametrize("layout", F.LAYOUTS)
def test_layout_arithmetic(layout):
    seen = 0
    for fc in FT.CASES:
        for i in range(fc.ncalls()):
            for name, h, row, unit in geometry(fc, i):
                p = F.pitch_of(layout, h, row, unit)
                what = (fc.name, name, layout)
                assert h >= F.MIN_ROWS and row <= p < 1 << 31 and p % unit == 0, what
                starts = np.arange(h, dtype=np.int64) * p
                if layout == "under_2g":
                    assert F.extent(h, p, row) <= (1 << 31) - 1 and h * p > 1 << 31, what
                else:
                    b = F.BOUNDARY[layout]
                    assert (starts >= b).sum() == F.EDGE_ROWS and (starts + row <= b).sum() >= F.EDGE_ROWS, what
                    assert F.extent(h, p, row) <= 1.3 * b, what
                seen += 1
    assert seen >= len(FT.CASES)


@pytest.mark.parametrize("layout", F.LAYOUTS)
def test_rectangles_keep_apart_and_fit(layout):
    for fc in FT.CASES:
        taken = []
        for i in range(fc.ncalls()):
            rects = F.place(geometry(fc, i), layout, pitches=fc.share, taken=taken)
            assert len(rects) == len(fc.images(i)), fc.name
            assert F.separated(taken + rects), (fc.name, i)
            for r in rects:
                assert 0 <= r.col and r.extent <= F.SPAN and (F.LOW_GUARD + r.col) % r.unit == 0, (fc.name, r)
                # whatever 32 bits make of one of its offsets stays inside the arena: at most 2^32 below the base
                assert F.LOW_GUARD + r.col - (1 << 32) >= 0 and F.LOW_GUARD + r.extent + F.HIGH_GUARD <= F.ARENA_BYTES
            if fc.base.keep:  # an input kept for the next call shares the arena with that call's images
                taken = [r for r in rects if r.name in fc.base.keep]
        assert any(fc.images(i) for i in range(fc.ncalls())), fc.name
    assert F.ARENA_BYTES <= 10 * F.GIB and F.LOW_GUARD == 4 * F.GIB and F.HIGH_GUARD == 1 << 20
    assert F.gap(F.Rect("a", 0, 32, 100, 1 << 20, 1), F.Rect("b", 100 + 4095, 32, 100, 1 << 20, 1)) == 4095
    assert not F.separated([F.Rect("a", 0, 32, 100, 1 << 27, 1), F.Rect("b", 4196 - 1, 32, 100, 1 << 27, 1)])
    p = (1 << 27) + 8192  # a's row 32 starts at 2^32 + 262144: moved 2^32 down it lands 900 bytes from b's row 0
    assert F.separated([F.Rect("a", 0, 32, 100, p, 1), F.Rect("b", 263144, 32, 100, p, 1)])
    assert not F.separated([F.Rect("a", 0, 33, 100, p, 1), F.Rect("b", 263144, 32, 100, p, 1)])


def test_bounds_cite_the_header_and_spare_under_2g():
    text = header_text()
    bounded = [c for c in FT.CASES if c.bound is not None]
    assert len(bounded) >= 12
    for c in bounded:
        quotes = re.findall(r"\"(.*?)\"", c.bound.cite)
        assert c.bound.cite.startswith("tbdk.h") and quotes, c.name
        for q in quotes:
            assert re.sub(r"\s+", " ", q) in text and "4294967295" in q, (c.name, q)
        for i in range(c.ncalls()):
            for name, h, row, unit in geometry(c, i):
                assert c.bound.accepts(h, F.pitch_of("under_2g", h, row, unit), row), (c.name, "under_2g")
                assert c.bound.accepts(h, F.pitch_of("over_2g", h, row, unit), row), (c.name, "over_2g")
                last = c.bound.last_accepted(h, row, unit)
                assert c.bound.accepts(h, last, row) and not c.bound.accepts(h, last + unit, row)
                assert last + unit <= F.pitch_of("over_4g", h, row, unit) and F.extent(h, last + unit, row) <= F.SPAN - 64 * F.SLOT
    # the rejections are the buffer-descriptor kernels only: GFTT's walk (also as the minimum-eigenvalue map), PyrLK
    # on a borrowed level 0, and the loop where its run reaches them
    assert {s for c in bounded for s, _ in c.covers} == {
        "tbdk_gftt_rois", "tbdk_gftt_rois_masked", "tbdk_gftt_rois_px", "tbdk_corner_min_eig_val", "tbdk_corner_response",
        "tbdk_corner_response_px", "tbdk_pyr_build_borrowed", "tbdk_tbd_run", "tbdk_tbd_set_corner_mask"}


def test_the_far_masks_are_aperiodic():
    """a mask row read whole pitches too low must not pass for the right one"""
    for m in (FT.gftt_mask(), FT.loop_mask()):
        h = m.shape[0]
        assert 0.2 < (m != 0).mean() < 0.8
        for y in range(h - F.EDGE_ROWS, h):  # the rows beyond a boundary against the rows they would wrap to
            for lower in range(0, F.EDGE_ROWS):
                assert not np.array_equal(m[y], m[lower]), (y, lower)


def test_cases_reuse_an_active_oracle_case():
    """every case stands on a case of the streams table's kind whose oracle finds something (checked for the table's own
    cases by tests/test_streams_cases.py; here for the cases built in _far_table.py)"""
    for c in FT.CASES:
        if c.base.name in FT.T.BY_NAME or c.base.sync is not None:
            continue  # the streams table's own, or a loop (its oracle runs for seconds: the GPU test computes it)
        want = FT.T.refs(c.base, "real")
        assert (c.base.active or FT.T.nonempty)(want), f"{c.name}: the oracle finds nothing"
