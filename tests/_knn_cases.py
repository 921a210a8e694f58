"""The recorded BackgroundSubtractorKNN cases (tests/golden/reference_knn.npz): the case table and the fixture's
packing.  The frames are those of tests/_mog2_cases.py.  tools/record_reference_cases.py records the cases; the
oracle, host-core and GPU tests regenerate the frames from here."""
import numpy as np

import _mog2_cases as GC

W, H, NFRAMES = GC.W, GC.H, GC.NFRAMES
BG_FRAMES = GC.BG_FRAMES

DEFAULTS = dict(history=500, nsamples=7, knn_samples=2, detect_shadows=1, shadow_value=127, dist2_threshold=400.0,
                shadow_threshold=0.5, rng_state=0xffffffff)
PARAM_KEYS = tuple(DEFAULTS)
SECOND_SEED = 0x9e3779b97f4a7c15

# With one sample a list, this rate gives the periods 327, 512 and 1266 (tests/test_knn_oracle.py holds it): the
# short plane is redrawn after frame 327 with d = 327 (DivStruct, values above 255 saturate) and the mid plane after
# frame 512 with d = 512 (a power of two above 256: a step per value, saturated).  A fill with range d needs d
# frames since the plane's last one, so nothing shorter reaches those two paths.
LONG_RATE, LONG_FRAMES = 0.001095, 514


def cases():
    """dicts: name, w, h, n, cn, params (overrides of DEFAULTS), rates (n learning rates), bg (1-based frames
    after which the background is recorded), whole (store masks and backgrounds whole)"""
    rows = []

    def add(name, w=W, h=H, n=NFRAMES, cn=1, rates=None, bg=None, whole=False, **params):
        r = np.full(n, -1.0)
        for k, v in (rates or {}).items():
            r[k] = v
        rows.append(dict(name=name, w=w, h=h, n=n, cn=cn, content="u8", params=params, rates=r,
                         bg=tuple(bg if bg is not None else (n,)), whole=whole))

    for cn in (1, 3):
        for hist in (500, 12):
            add(f"8UC{cn} history {hist}", cn=cn, history=hist, bg=BG_FRAMES, whole=True)
    for rate in (0.05, 0.3):
        add(f"rate {rate} over frames 20..29", cn=3, rates={t: rate for t in range(20, 30)}, bg=(30, 48))
    add("rate 1 at frame 25", rates={25: 1.0}, bg=(26, 48))
    for k in (1, 3, 16):
        add(f"nsamples {k}", cn=3 if k == 3 else 1, nsamples=k)
    for k in (1, 5):
        add(f"knn_samples {k}", cn=3 if k == 5 else 1, knn_samples=k)
    add("shadows off", cn=3, detect_shadows=0)
    add("shadow value 0 threshold 0.8", cn=3, shadow_value=0, shadow_threshold=0.8)
    add("dist2_threshold 100", cn=3, dist2_threshold=100.0)
    add("history 20000 nsamples 1 rate 1/20000", n=12, history=20000, nsamples=1, rates={t: 1 / 20000 for t in range(12)})
    add("second seed", cn=3, rng_state=SECOND_SEED)
    for (w, h) in ((1, 1), (7, 1), (1, 9), (67, 23)):
        for cn in (1, 3):
            add(f"{w}x{h} 8UC{cn}", w=w, h=h, n=8, cn=cn, bg=(1, 8))
    add("301x211 8UC3", w=301, h=211, n=8, cn=3, bg=(8,))
    add("8x6 nsamples 1 periods 327 and 512", w=8, h=6, n=LONG_FRAMES, nsamples=1,
        rates={t: LONG_RATE for t in range(LONG_FRAMES)}, bg=(327, 328, 512, 513, LONG_FRAMES))
    return rows


NCASES = 27


def label(i):
    return cases()[i]["name"]


def params(case):
    p = dict(DEFAULTS)
    p.update(case["params"])
    return p


def case_frames(case):
    return GC.frames(case["w"], case["h"], case["n"], case["cn"], "u8")


# ---- the fixture's packing ------------------------------------------------------------------------------------

crcs = GC.crcs
unpack_masks = GC.unpack_masks


def stored_masks(case, masks):
    """what the fixture holds for a case's masks: 2-bit packed, or one CRC per frame"""
    return GC.pack_masks(masks, params(case)["shadow_value"]) if case["whole"] else crcs(masks)


def stored_background(case, img):
    """a background image as the fixture holds it: whole for the base cases, else row CRCs"""
    return np.ascontiguousarray(img) if case["whole"] else crcs(img)


def split_state(state):
    """a uint64 as two int32 words (low, high): the fixture holds no uint32 arrays but row CRCs"""
    return np.array([state & 0xffffffff, state >> 32], np.uint32).view(np.int32)


def join_state(words):
    lo, hi = (int(x) for x in np.asarray(words).view(np.uint32))
    return lo | hi << 32
