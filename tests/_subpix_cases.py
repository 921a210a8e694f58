"""The cornerSubPix cases recorded in tests/golden/reference_subpix.npz
(tools/record_reference_cases.py, fixture `subpix`): images, point sets, windows,
zero zones and criteria.  The recorder, tests/test_subpix_oracle.py (the numpy
restatement) and tests/test_gpu_subpix.py (the kernel) all take the inputs from
here; the fixture stores the point sets (each image's GFTT corners come from
the reference's goodFeaturesToTrack at recording time), the refined points of
every case and the table of expf values the window mask is made of.

Images, each as 8U and as 32F (the 8-bit values plus a hashed fraction, so that
the 32F cases hold values no 8-bit image has):
  bb    the 64 x 48 basketball crop at (250, 200) of basketball_pair.npz
  n37   hashed noise, 37 x 61
  n130  hashed noise, 130 x 121, with a constant square (det fails at the first
        iteration for points in it) and a two-level step pasted in
  n15   hashed noise, 15 x 15: the minimum for win 5, every patch on the border path
  n25   hashed noise, 25 x 35: the minimum for win (10, 15)
Points of an image: its GFTT corners (256, 0.01, 3.0), the same corners moved by
(+0.37, -0.21), then SPECIAL points: the four image corners, the points half a
pixel inside each edge, two points outside the image, and for n130 points in the
constant square and points one pixel off the step."""
import numpy as np

import _reference_cases as RC

GFTT = (256, 0.01, 3.0)
SHIFT = np.float32([0.37, -0.21])
# (name, width, height, noise seed)
IMAGES = [("bb", 64, 48, 0), ("n37", 37, 61, 611), ("n130", 130, 121, 612), ("n15", 15, 15, 613), ("n25", 25, 35, 614)]
SIZE = {name: (w, h) for name, w, h, _ in IMAGES}
CONST_BOX = (20, 60, 40, 40)   # x, y, w, h of n130's constant square (value 77)
STEP_BOX = (70, 20, 50, 14)    # n130's step: columns below x = 98 are 0, the others 255
STEP_X = 98

LKDEMO = ((10, 10), (-1, -1), (3, 20, 0.03))
# (win, zero zone, (criteria type, maxCount, epsilon))
FULL = [((5, 5), (-1, -1), (3, 20, 0.03)),
        LKDEMO,
        ((3, 7), (0, 0), (1, 1, 0.0)),
        ((1, 1), (-1, -1), (2, 0, 0.001)),     # EPS only: up to 100 iterations
        ((15, 15), (1, 1), (3, 0, -1.0)),      # clamps to one iteration and eps 0
        ((5, 5), (1, 1), (1, 1000, 0.0)),      # clamps to 100 iterations
        ((5, 5), (5, 2), (3, 20, 0.03))]       # a zero zone as wide as the window: ignored
CONFIGS = {"bb": FULL, "n37": FULL, "n130": FULL,
           "n15": [((5, 5), (-1, -1), (3, 20, 0.03)), ((5, 5), (1, 1), (2, 0, 0.001)), ((1, 1), (0, 0), (3, 20, 0.03))],
           "n25": [((10, 15), (-1, -1), (3, 20, 0.03)), ((10, 15), (0, 0), (1, 1000, 0.0))]}
DEPTHS = ("8u", "32f")


def image(name, depth="8u"):
    """the case image `name` as uint8 (depth "8u") or float32 ("32f")"""
    w, h = SIZE[name]
    seed = dict((n, s) for n, _, _, s in IMAGES)[name]
    if name == "bb":
        img = np.ascontiguousarray(RC.basketball()[0][200:200 + h, 250:250 + w])
    else:
        img = RC.noise(w, h, 1, seed)
    if name == "n130":
        x, y, bw, bh = CONST_BOX
        img[y:y + bh, x:x + bw] = 77
        x, y, bw, bh = STEP_BOX
        img[y:y + bh, x:STEP_X] = 0
        img[y:y + bh, STEP_X:x + bw] = 255
    if depth == "8u":
        return img
    frac = RC.noise(w, h, 1, seed + 1000).astype(np.float32) / np.float32(256)
    return np.ascontiguousarray(img.astype(np.float32) + frac)


def special_points(name):
    w, h = SIZE[name]
    p = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1),
         (0.5, h // 2), (w - 1.5, h // 2), (w // 2, 0.5), (w // 2, h - 1.5),
         (-3.25, h // 3), (w + 2.5, h + 1.0)]
    if name == "n130":
        cx, cy = CONST_BOX[0] + CONST_BOX[2] // 2, CONST_BOX[1] + CONST_BOX[3] // 2
        p += [(cx, cy), (cx - 0.5, cy - 0.75), (cx + 1, cy + 1)]
        sy = STEP_BOX[1] + STEP_BOX[3] // 2
        p += [(STEP_X - 2, sy), (STEP_X + 1, sy), (STEP_X - 2, sy - 3.5), (STEP_X + 1, STEP_BOX[1] + 1),
              (STEP_X - 1.5, STEP_BOX[1] + STEP_BOX[3] - 2)]
    return np.float32(p)


def points(name, gftt_corners):
    """the point set of image `name` from its GFTT corners (n, 2)"""
    c = np.float32(gftt_corners).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([c, c + SHIFT, special_points(name)]), dtype=np.float32)


def cases():
    """(image name, depth, win, zero zone, criteria), in the fixture's order"""
    return [(name, depth, *cfg) for name, _, _, _ in IMAGES for depth in DEPTHS for cfg in CONFIGS[name]]


def label(i):
    name, depth, win, zero, crit = cases()[i]
    return f"{name} {depth} win {win} zero {zero} criteria {crit}"


def fixture():
    return RC.fixture("subpix")


def exp_table(fx):
    """the recorded expf(-(k/w)^2): w -> float32 array of k = 0 .. w"""
    t = fx["expf"]
    return {w: t[w - 1, :w + 1] for w in range(1, 16)}
