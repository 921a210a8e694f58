"""The recorded cases of cv::remap and cv::warpPerspective
(tests/golden/reference_remap.npz, reference_warpperspective.npz): inputs are
generated here from integer hashing and closed forms, never stored.  Shared by
tools/record_reference_cases.py, tests/test_remap_oracle.py,
tests/test_gpu_remap.py and the host bounds walk (tests/test_remap_bounds.py)."""
import numpy as np

import _frontend_oracle as F
import _remap_oracle as R

WHOLE_LIMIT = 2048  # bytes: larger outputs are stored as one CRC-32 per row

# (width, height, extra pitch in pixels)
SOURCES = [(1, 1, 0), (2, 2, 0), (3, 3, 0), (37, 23, 11), (130, 121, 0)]
# 67x7 and 300x5: warpPerspective's block is 67 and 204 columns wide there; 130x33 crosses a
# 64-column block and a thread's group of four pixels
DESTS = [(1, 1), (5, 3), (67, 7), (300, 5), (67, 15), (130, 33)]
BORDER_VALUE = (17.5, 300.0, -4.0, 99.25)  # saturates per channel: 8U (18, 255, 0, 99)
HOSTILE = [np.nan, np.inf, -np.inf, 1e30, -1e30, 40000.0, -40000.0]


def image(w, h, cn, depth, seed):
    """u8 hashed noise, or for 32F a float32 image in [-64, 192) with 16 significant bits"""
    a = np.ascontiguousarray(F.pattern(w, h, cn, seed))
    if depth == "8u":
        return a
    b = np.ascontiguousarray(F.pattern(w, h, cn, seed + 7919))
    return ((a.astype(np.float32) * 256 + b.astype(np.float32)) / np.float32(256) - np.float32(64)).astype(np.float32)


def _unit(w, h, seed):
    """hashed noise in [0, 1), 16 bits, two planes"""
    a, b = F.pattern(w, h, 2, seed).astype(np.float64), F.pattern(w, h, 2, seed + 104729).astype(np.float64)
    return (a * 256 + b) / 65536.0


def _smooth(sw, sh, dw, dh, seed):
    ang = np.deg2rad(7 + seed % 23)
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    u, v = (x - dw / 2) * (sw + 6) / max(dw, 1), (y - dh / 2) * (sh + 6) / max(dh, 1)
    mx = sw / 2 + u * np.cos(ang) - v * np.sin(ang) + 1.5 * np.sin(y / 3.0 + seed)
    my = sh / 2 + u * np.sin(ang) + v * np.cos(ang) + 1.25 * np.cos(x / 4.0)
    return mx, my


def float_map(gen, sw, sh, dw, dh, seed):
    """(dh, dw, 2) float32"""
    if gen == "smooth":
        mx, my = _smooth(sw, sh, dw, dh, seed)
    elif gen == "noise":  # -20 .. size + 20
        u = _unit(dw, dh, 900 + seed)
        mx, my = -20 + u[..., 0] * (sw + 40), -20 + u[..., 1] * (sh + 40)
    elif gen == "ties":  # k + 1/64 (a tie of cvRound(v * 32)) and k + 0.5 (a tie of cvRound(v))
        y, x = np.mgrid[0:dh, 0:dw]
        fr = np.where((x + y) % 2 == 0, 1.0 / 64, 0.5)
        mx = ((x * 7 + y * 3 + seed) % (sw + 4) - 2) + fr
        my = ((x * 5 + y * 11 + seed) % (sh + 4) - 2) + fr[:, ::-1]
    elif gen == "hostile":
        mx, my = _smooth(sw, sh, dw, dh, seed)
        hsh = F.pattern(dw, dh, 2, 1300 + seed).astype(np.int64)
        hv = np.array(HOSTILE)
        px, py = hsh[..., 0] % 5 == 0, hsh[..., 1] % 5 == 0
        mx = np.where(px, hv[(hsh[..., 0] // 5) % len(hv)], mx)
        my = np.where(py, hv[(hsh[..., 1] // 5) % len(hv)], my)
    else:
        raise ValueError(gen)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.stack([mx, my], -1).astype(np.float32))


def fixed_map(gen, sw, sh, dw, dh, seed):
    """CV_16SC2 coordinates and a CV_16UC1 fraction plane whose words go above 1023"""
    m = float_map("smooth" if gen == "hostile" else gen, sw, sh, dw, dh, seed)
    xy = np.clip(np.floor(m.astype(np.float64)), -32768, 32767).astype(np.int16)
    if gen == "hostile":  # the ends of the short range, where NEAREST's delta wraps
        hsh = F.pattern(dw, dh, 2, 1700 + seed).astype(np.int64)
        ends = np.array([-32768, 32767, -32767, 32766], np.int16)
        for c in (0, 1):
            xy[..., c] = np.where(hsh[..., c] % 4 == 0, ends[(hsh[..., c] // 4) % 4], xy[..., c])
    p = F.pattern(dw, dh, 2, 2100 + seed).astype(np.uint16)
    frac = (p[..., 0] << 8) | p[..., 1]
    return np.ascontiguousarray(xy), np.ascontiguousarray(frac)


KINDS = ("32fc2", "32fc1", "16sc2f", "16sc2")  # 16sc2f: with the fraction plane; 16sc2: alone (NEAREST only)


def remap_cases():
    """(depth, cn, source index, dest index, map generator, kind, interpolation, border)"""
    rows = []
    i = 0
    # every interpolation x every border, per depth, channel counts and map kinds in rotation
    for depth, inters, cns in (("8u", (0, 1, 2, 3), (1, 3, 4, 2)), ("32f", (0, 1, 3), (1, 2, 3, 4))):
        for inter in inters:
            for border in range(6):
                gen = ("smooth", "noise", "ties", "hostile")[i % 4]
                kind = ("32fc2", "32fc1", "16sc2f")[(i // 2) % 3]
                rows.append((depth, cns[i % 4], 3 + i % 2, 2 + i % 4, gen, kind, inter, border))
                i += 1
    # the small sources: every pixel on the border path (1x1), below the cubic inlier window (2x2, 3x3)
    for s in (0, 1, 2):
        for inter in (0, 1, 2):
            for border in (R.BORDER_CONSTANT, R.BORDER_REFLECT_101, R.BORDER_WRAP, R.BORDER_TRANSPARENT):
                depth = "32f" if inter < 2 and (s + border) % 2 else "8u"
                rows.append((depth, (1, 3, 4)[(s + inter + border) % 3], s, 1 + (s + border) % 2,
                             ("noise", "ties")[border % 2], "32fc2", inter, border))
    # the 1x1 destination and 16SC2 alone
    for k, kind in enumerate(KINDS):
        rows.append(("8u", 3, 3, 0, "smooth", kind, 0, R.BORDER_REFLECT))
        rows.append(("32f", 1, 4, 5, "noise", kind, 0, R.BORDER_REPLICATE))
    # hostile values through every decoder and interpolation
    for kind in ("32fc2", "32fc1", "16sc2f"):
        for inter in (0, 1, 2):
            rows.append(("8u", 3 if inter else 4, 4, 5, "hostile", kind, inter, (R.BORDER_WRAP, R.BORDER_REFLECT,
                                                                               R.BORDER_CONSTANT)[inter]))
        rows.append(("32f", 2, 3, 4, "hostile", kind, 1, R.BORDER_REFLECT_101))
    rows.append(("8u", 1, 4, 5, "hostile", "16sc2", 0, R.BORDER_REFLECT_101))
    return rows


def remap_inputs(i):
    """source, pre-filled destination, map1, map2 (or None), kind constant, border value"""
    depth, cn, s, d, gen, kind, inter, border = remap_cases()[i]
    (sw, sh, _), (dw, dh) = SOURCES[s], DESTS[d]
    src, dst = image(sw, sh, cn, depth, 3000 + i), image(dw, dh, cn, depth, 5000 + i)
    if kind == "32fc2":
        m1, m2, k = float_map(gen, sw, sh, dw, dh, i), None, R.MAP_32FC2
    elif kind == "32fc1":
        m = float_map(gen, sw, sh, dw, dh, i)
        m1, m2, k = np.ascontiguousarray(m[..., 0]), np.ascontiguousarray(m[..., 1]), R.MAP_32FC1
    else:
        m1, m2 = fixed_map(gen, sw, sh, dw, dh, i)
        k = R.MAP_16SC2
        if kind == "16sc2":
            m2 = None
    return src, dst, m1, m2, k, BORDER_VALUE


def remap_label(i):
    depth, cn, s, d, gen, kind, inter, border = remap_cases()[i]
    return f"{depth}c{cn} {SOURCES[s][0]}x{SOURCES[s][1]} -> {DESTS[d][0]}x{DESTS[d][1]} {gen} {kind} " \
           f"inter {inter} border {border}"


def matrix(name, sw, sh, dw, dh):
    if name == "identity":
        return np.eye(3)
    if name == "mild":
        return np.array([[1.02, 0.03, -2.5], [-0.02, 0.98, 1.75], [1e-4, -1.2e-4, 1.0]])
    if name == "wcross":  # W = 1 - x/64 + y/512: zero inside destinations wider than 64 columns
        return np.array([[0.9, 0.1, 1.0], [-0.1, 0.9, 2.0], [-1.0 / 64, 1.0 / 512, 1.0]])
    if name == "wzero":  # W exactly zero along column 64
        return np.array([[0.9, 0.1, 1.0], [-0.1, 0.9, 2.0], [-1.0 / 64, 0.0, 1.0]])
    if name == "singular":
        return np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    if name == "large":  # drives fX, fY into the INT_MIN / INT_MAX clamps
        return np.array([[3e8, 1e7, -5e9], [-2e8, 4e8, 1e9], [0.0, 0.0, 1.0]])
    if name == "tinyw":  # W subnormal: 32/W is inf, and 0 * inf a NaN in column 0 and row 0
        return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1e-310]])
    raise ValueError(name)


MATRICES = ("identity", "mild", "wcross", "wzero", "singular", "large", "tinyw")


def persp_cases():
    """(depth, cn, source index, dest index, matrix, flags, border)"""
    rows = []
    i = 0
    for name in MATRICES:
        for inv in (0, R.WARP_INVERSE_MAP):
            for inter in (0, 1, 2):
                depth = "32f" if inter < 2 and i % 3 == 1 else "8u"
                d = (5, 2, 3, 4, 1)[i % 5] if name not in ("wcross", "wzero", "tinyw") else (5, 2, 3)[i % 3]
                rows.append((depth, (1, 3, 4, 2)[i % 4] if depth == "32f" else (1, 3, 4)[i % 3], 3 + i % 2, d, name,
                             inter | inv, i % 6))
                i += 1
    rows.append(("8u", 1, 4, 0, "mild", R.INTER_LINEAR, R.BORDER_CONSTANT))
    rows.append(("8u", 3, 0, 1, "mild", R.INTER_AREA | R.WARP_INVERSE_MAP, R.BORDER_REPLICATE))
    rows.append(("8u", 4, 2, 4, "mild", R.INTER_CUBIC, R.BORDER_TRANSPARENT))
    rows.append(("32f", 3, 1, 2, "identity", R.INTER_LINEAR, R.BORDER_CONSTANT))
    return rows


def persp_inputs(i):
    depth, cn, s, d, name, flags, border = persp_cases()[i]
    (sw, sh, _), (dw, dh) = SOURCES[s], DESTS[d]
    return (image(sw, sh, cn, depth, 7000 + i), image(dw, dh, cn, depth, 9000 + i), matrix(name, sw, sh, dw, dh),
            BORDER_VALUE)


def persp_label(i):
    depth, cn, s, d, name, flags, border = persp_cases()[i]
    return f"{depth}c{cn} {SOURCES[s][0]}x{SOURCES[s][1]} -> {DESTS[d][0]}x{DESTS[d][1]} {name} flags {flags} " \
           f"border {border}"
