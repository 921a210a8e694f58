"""Every row path and strip edge of the GFTT eigenvalue walk (klt_gftt.hip,
eig_segment) against the oracle: identical corner lists per ROI, same order,
same count.

The walk splits a ROI's rows into four segments of ceil(h / 4) own rows; a
segment runs its steady rows four at a time (eight in the eigenvalue-plane
kernel), what is left of them one at a time, and the rows at its ends (the
first rows, the capture row before the next segment, the last row, the halo
rows) through the run-time-flag row.  The ROI heights give segments that are
not live (h < 4), segments with fewer steady rows than one block, every
remainder 0..3 after the blocks, and a capture row next to a remainder row;
the widths straddle the 56-column strip on both sides.  Each shape lies on a
textured patch, a flat patch (all eigenvalues equal: the >= ties of the
local-maximum test), a saturated patch and a patch of isolated dots and a
two-pixel checkerboard (equal positive eigenvalues next to each other: ties
that reach the corner list); a few ROIs cross from one patch into the next."""
import numpy as np
import pytest
import torch

import _gftt_f32_oracle as O32
import _gftt_mask_cases as MC
import _gftt_mask_oracle as MO
import _oracle as O

pytestmark = pytest.mark.gpu

HEIGHTS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 19, 20, 21, 23, 33]
WIDTHS = [1, 2, 3, 55, 56, 57, 58, 112, 113]
PATCHES = ["textured", "flat", "saturated", "plateau"]
PW, PH = 480, 240  # one patch; the frame is the four stacked
PARAMS = [(100, 0.01, 0.0), (64, 0.05, 3.0)]  # (maxCorners, quality, minDistance)
BATCH = 100  # ROIs per call: within the 128 whose table travels in the kernel arguments
DEFAULTS = {"gftt_compact": 1, "gftt_eig_redo": 0}

_cache = {}


def cached(key, make):
    """a reference computed once and shared (read only)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frame():
    def make():
        rng = np.random.default_rng(20261021)
        f = np.zeros((4 * PH, PW), np.uint8)
        n = rng.integers(0, 256, (PH + 1, PW + 1)).astype(np.int32)
        f[:PH] = ((n[:-1, :-1] + n[1:, :-1] + n[:-1, 1:] + n[1:, 1:]) // 4).astype(np.uint8)
        f[20:60, 30:200] //= 8  # a dark and a bright region: corners of very different strength
        f[100:180, 250:400] = 255 - f[100:180, 250:400] // 6
        f[PH:2 * PH] = 77
        f[2 * PH:3 * PH] = 255
        p = f[3 * PH:]
        p[:] = 100
        p[6::12, 5:PW // 2:12] = 200  # isolated dots: mirror-symmetric eigenvalues round each
        yy, xx = np.mgrid[0:PH, PW // 2:PW]
        p[:, PW // 2:] = np.where(((yy // 2) + (xx // 2)) % 2 == 0, 60, 180)
        f.setflags(write=False)
        return f
    return cached("frame", make)


def rois():
    def make():
        out = []
        for k in range(len(PATCHES)):
            y = k * PH + 1
            for h in HEIGHTS:
                x = 1
                for w in WIDTHS:
                    out.append((x, y, w, h))
                    x += w + 1
                y += h + 1
        # across the patch borders: flat and saturated rows inside a ROI whose threshold is positive
        out += [(10, PH - 10, 113, 21), (200, PH - 15, 57, 33), (5, 2 * PH - 9, 58, 20), (300, 3 * PH - 4, 112, 9),
                (100, 3 * PH - 10, 56, 23), (250, PH - 3, 3, 7)]
        return out
    return cached("rois", make)


def batches(rs):
    return [rs[i:i + BATCH] for i in range(0, len(rs), BATCH)]


def detect(img, rs, maxc, q, md, mask=None):
    from opencv_amd import klt

    det = klt.GoodFeaturesToTrackDetector(maxc, q, md)
    cs, ns = [], []
    for b in batches(rs):
        c, n = det.detect_rois(img, b, mask=mask)
        cs.append(c)
        ns.append(n)
    torch.cuda.synchronize()
    return [c.cpu().numpy() for c in cs], [n.cpu().numpy() for n in ns]


def check(ref, cs, ns, rs, what):
    i = 0
    for c, n in zip(cs, ns):
        for j in range(len(n)):
            r = ref[i]
            assert n[j] == len(r), f"{what} roi {rs[i]}: count {n[j]} vs {len(r)}"
            assert np.array_equal(c[j, :n[j]], r), f"{what} roi {rs[i]}: corners differ"
            i += 1
    assert i == len(ref)


class options:
    def __init__(self, gpu, **kw):
        self.gpu, self.kw = gpu, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.gpu.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.gpu.set_option(k, DEFAULTS[k])


def test_the_frame_has_what_the_cases_need():
    """(no GPU work) the plateau patch holds equal positive eigenvalues side by
    side, the flat and saturated ones equal eigenvalues only, and the reference
    lists are not empty where a patch has texture"""
    e = O.min_eig(frame()[3 * PH:])
    assert ((e[1:-1, 1:-2] == e[1:-1, 2:-1]) & (e[1:-1, 1:-2] > 0.01 * e.max())).sum() > 100
    for k in (1, 2):
        assert (O.min_eig(frame()[k * PH:(k + 1) * PH]) == 0).all()
    ref = cached(("ref", PARAMS[0]), lambda: O.gftt_rois(frame(), rois(), *PARAMS[0]))
    per = len(HEIGHTS) * len(WIDTHS)
    assert sum(len(r) for r in ref[:per]) > 1000 and sum(len(r) for r in ref[3 * per:4 * per]) > 1000
    assert sum(len(r) for r in ref[per:3 * per]) == 0
    assert all(len(ref[4 * per + i]) > 0 for i in (0, 1, 3, 4))  # (a straight edge between flat patches has no corner)


@pytest.mark.parametrize("maxc,q,md", PARAMS)
@pytest.mark.parametrize("compact,redo", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_row_paths_match_oracle(gpu, compact, redo, maxc, q, md):
    ref = cached(("ref", (maxc, q, md)), lambda: O.gftt_rois(frame(), rois(), maxc, q, md))
    img = cached("dev", lambda: torch.from_numpy(np.array(frame())).cuda())
    with options(gpu, gftt_compact=compact, gftt_eig_redo=redo):
        cs, ns = detect(img, rois(), maxc, q, md)
    check(ref, cs, ns, rois(), f"compact {compact} redo {redo} ({maxc}, {q}, {md})")


def test_row_paths_masked(gpu):
    maxc, q, md = PARAMS[0]
    m = MC.checker(PW, 4 * PH, 5)
    m[:, 300:] = 255  # strips with nothing masked out
    m[50:70] = 0      # and ROIs with nothing masked in
    ref = MO.gftt_rois_masked(frame(), m, rois(), maxc, q, md)
    img = cached("dev", lambda: torch.from_numpy(np.array(frame())).cuda())
    cs, ns = detect(img, rois(), maxc, q, md, mask=torch.from_numpy(m).cuda())
    check(ref, cs, ns, rois(), "masked")
    assert sum(int(n.sum()) for n in ns) > 1000


def test_row_paths_u16(gpu):
    maxc, q, md = PARAMS[0]
    f16 = frame().astype(np.uint16) * 257  # 0 .. 65535: the saturated patch is the type's maximum
    ref = O32.gftt_rois(f16, None, rois(), maxc, q, md)
    cs, ns = detect(torch.from_numpy(f16).cuda(), rois(), maxc, q, md)
    check(ref, cs, ns, rois(), "u16")
    assert sum(int(n.sum()) for n in ns) > 1000


def test_row_paths_f32_with_negative_zero_pixels(gpu):
    maxc, q, md = PARAMS[0]
    rng = np.random.default_rng(7)
    f = frame().astype(np.float32) / np.float32(255)
    f[rng.random(f.shape) < 0.05] = -0.0  # sprinkled
    f[PH:PH + PH // 2] = -0.0             # half of the flat patch
    f[30:50, 100:300] = -0.0
    assert np.signbit(f).sum() > 10000
    ref = O32.gftt_rois(f, None, rois(), maxc, q, md)
    cs, ns = detect(torch.from_numpy(f).cuda(), rois(), maxc, q, md)
    check(ref, cs, ns, rois(), "f32")
    assert sum(int(n.sum()) for n in ns) > 1000
