"""The recorded BackgroundSubtractorMOG2 cases (tests/golden/reference_mog2.npz): the frame generator, the case
table and the fixture's packing.  tools/record_reference_cases.py records them; the oracle, host-core and GPU
tests regenerate the frames from here."""
import numpy as np

import _reference_cases as RC
from _frontend_oracle import pattern

W, H, NFRAMES = 64, 48, 48
BG_FRAMES = (1, 12, 30, 48)  # backgrounds are recorded after these frames (1-based)

DEFAULTS = dict(history=500, nmixtures=5, detect_shadows=1, shadow_value=127, var_threshold=16.0,
                var_threshold_gen=9.0, var_init=15.0, var_min=4.0, var_max=75.0, background_ratio=0.9,
                complexity_reduction=0.05, shadow_threshold=0.5)
PARAM_KEYS = tuple(DEFAULTS)


def _noise(w, h, seed, span):
    """hashed integers in -span..span"""
    return pattern(w, h, 1, seed).astype(np.int32) % (2 * span + 1) - span


def gray_frame(t, w=W, h=H):
    """Frame t of the sequence (int32, 0..255): a blocky static texture 20..219 in 4x4 blocks with +-2 noise;
    rows 40.. with +-20 noise; +25 from frame 30; a bright 10x12 rectangle moving 3 px a frame; a 12x10 region
    moving 2 px a frame the other way at 0.6 of the background; columns 56.. cycling through nine levels 26
    apart; columns 0..7 exactly 0."""
    tex = 20 + pattern(w // 4 + 1, h // 4 + 1, 1, 901).astype(np.int32) % 200
    tex = np.repeat(np.repeat(tex, 4, 0), 4, 1)[:h, :w]
    if t >= 30:
        tex = tex + 25
    f = tex + _noise(w, h, 1000 + t, 2)
    f[40:] = (tex + _noise(w, h, 3000 + t, 20))[40:]
    x0, y0 = (8 + (3 * t) % 40, 6) if w >= 16 else ((3 * t) % w, (2 * t) % h)
    f[y0:y0 + 12, x0:x0 + 10] = 250
    x1, y1 = 44 - (2 * t) % 34, 24
    f[y1:y1 + 10, x1:x1 + 12] = (tex[y1:y1 + 10, x1:x1 + 12] * 3) // 5
    xs = np.arange(w)
    cyc = 12 + 26 * ((t + xs) % 9)
    f[:, 56:] = cyc[None, 56:]
    if w >= 16:
        f[:, :8] = 0
    return np.clip(f, 0, 255)


def frames(w=W, h=H, n=NFRAMES, cn=1, content="u8"):
    """(n, h, w[, 3]) frames: uint8 for "u8"; float32 for "frac" (the 8-bit values plus a hashed fraction) and
    "unit" (the same times 1/255).  Three channels: the gray plane with a hashed +-3 per channel, so that the
    shadow test's colour distortion decides some pixels."""
    out = []
    for t in range(n):
        g = gray_frame(t, w, h)
        if cn == 3:
            f = np.stack([np.clip(g + _noise(w, h, 5000 + 97 * c + t, 3) * (g > 0), 0, 255) for c in range(3)], -1)
        else:
            f = g
        if content == "u8":
            out.append(f.astype(np.uint8))
            continue
        frac = pattern(w, h, cn, 7000 + t).astype(np.float32) / np.float32(256)
        v = f.astype(np.float32) + frac * (f > 0)
        if content == "unit":
            v = v * np.float32(1 / 255.0)
        out.append(v.astype(np.float32))
    return np.stack(out)


def cases():
    """dicts: name, w, h, n, cn, content, params (overrides of DEFAULTS), rates (n learning rates), bg (1-based
    frames after which the background is recorded), whole (store the masks whole, 2 bits a pixel)"""
    rows = []

    def add(name, w=W, h=H, n=NFRAMES, cn=1, content="u8", rates=None, bg=None, whole=False, **params):
        r = np.full(n, -1.0)
        for k, v in (rates or {}).items():
            r[k] = v
        rows.append(dict(name=name, w=w, h=h, n=n, cn=cn, content=content, params=params, rates=r,
                         bg=tuple(bg if bg is not None else (n,)), whole=whole))

    for cn in (1, 3):
        for hist in (12, 500):
            add(f"8UC{cn} history {hist}", cn=cn, history=hist, bg=BG_FRAMES, whole=True)
    for rate in (0.05, 0.3, 0.0):
        add(f"rate {rate} over frames 20..29", history=12, rates={t: rate for t in range(20, 30)}, bg=(30, 48))
    add("rate 1 at frame 25", history=12, rates={25: 1.0}, bg=(26, 48))
    for k in (1, 3, 8):
        add(f"nmixtures {k}", history=12, nmixtures=k)
    add("shadows off", history=12, detect_shadows=0)
    add("shadow value 0 threshold 0.8", history=12, shadow_value=0, shadow_threshold=0.8)
    add("varThreshold 4 gen 25", history=12, var_threshold=4.0, var_threshold_gen=25.0)
    add("var_min above var_max", history=12, var_min=75.0, var_max=4.0)
    add("backgroundRatio 0.5", history=12, background_ratio=0.5)
    add("complexity reduction 0", history=12, complexity_reduction=0.0)
    s = 1.0 / (255.0 * 255.0)
    for cn in (1, 3):
        add(f"32FC{cn} frac", cn=cn, content="frac", history=12, bg=BG_FRAMES)
        add(f"32FC{cn} unit", cn=cn, content="unit", history=12, bg=BG_FRAMES, var_init=15.0 * s, var_min=4.0 * s,
            var_max=75.0 * s)
    for (w, h) in ((1, 1), (7, 1), (1, 9), (67, 23)):
        for cn in (1, 3):
            add(f"{w}x{h} 8UC{cn}", w=w, h=h, n=8, cn=cn, history=12, bg=(1, 8))
    return rows


NCASES = 29


def label(i):
    return cases()[i]["name"]


def params(case):
    p = dict(DEFAULTS)
    p.update(case["params"])
    return p


def case_frames(case):
    return frames(case["w"], case["h"], case["n"], case["cn"], case["content"])


# ---- the fixture's packing ------------------------------------------------------------------------------------

def crcs(a):
    """one CRC-32 per row of a (per frame for a stack of masks), as int32 words"""
    return RC.row_crcs(a).view(np.int32)


def pack_masks(masks, shadow_value):
    """(n, h, w) three-valued masks at 2 bits a pixel: 0 background, 1 shadow, 2 foreground"""
    m = np.asarray(masks)
    code = np.where(m == 255, 2, np.where(m == 0, 0, 1)).astype(np.uint8)
    assert np.isin(m, (0, 255, shadow_value)).all()
    if shadow_value in (0, 255):
        assert not (code == 1).any()
    flat = code.reshape(len(m), -1)
    pad = (-flat.shape[1]) % 4
    flat = np.pad(flat, ((0, 0), (0, pad))).reshape(len(m), -1, 4)
    return (flat[:, :, 0] | flat[:, :, 1] << 2 | flat[:, :, 2] << 4 | flat[:, :, 3] << 6).astype(np.uint8)


def unpack_masks(packed, n, h, w, shadow_value):
    q = np.stack([(packed >> s) & 3 for s in (0, 2, 4, 6)], -1).reshape(n, -1)[:, :h * w].reshape(n, h, w)
    return np.where(q == 2, 255, np.where(q == 1, shadow_value, 0)).astype(np.uint8)


def stored_masks(case, masks):
    """what the fixture holds for a case's masks: 2-bit packed, or one CRC per frame"""
    return pack_masks(masks, params(case)["shadow_value"]) if case["whole"] else crcs(masks)


def stored_background(img):
    """a background image as the fixture holds it: 8-bit whole, 32F as row CRCs"""
    return np.ascontiguousarray(img) if img.dtype == np.uint8 else crcs(img)
