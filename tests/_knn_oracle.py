"""A numpy restatement of cv::BackgroundSubtractorKNN's CPU class (modules/video/src/bgfg_KNN.cpp) and of the
cv::randu fills it makes (modules/core/src/rand.cpp), vectorised over the pixels, the samples in the reference's
order; the generator is stepped one state after the other in Python.

  _cvCheckPixelBackgroundNP :394-506, _cvUpdatePixelBackgroundNP :343-392, apply :749-812,
  getBackgroundImage :815-870; RNG_NEXT rand.cpp:75, randBits_ :87-143, randi_ :153-200, RNG::fill :571-623, :702-760

All float arithmetic is float32, one operation at a time.  The class keeps branch counts (KNN.counts) so that the
tests can say which paths a case took."""
import functools
import math

import numpy as np

F = np.float32
A = 4164903690          # CV_RNG_COEFF
M = (A << 32) - 1       # one step is x -> x * A (mod M)
MASK32 = 0xffffffff
BLOCK = 1024            # RNG::fill's BLOCK_SIZE

COUNT_KEYS = ("early_backgrounds", "include_by_pbf", "shadows", "zero_denominators", "foreground", "short_updates",
              "mid_updates", "long_updates", "fills_small", "fills_bits", "fills_div")


def rng_next(x):
    return (x & MASK32) * A + (x >> 32)


def randu_mode(d):
    """"small": a power of two up to 256, a step per four values; "bits": a larger power of two; "div": DivStruct"""
    if d & (d - 1) == 0:
        return "small" if d - 1 <= 255 else "bits"
    return "div"


def div_struct(d):
    l = 0
    while (1 << l) < d:
        l += 1
    return ((1 << 32) * ((1 << l) - d) // d + 1) & MASK32, min(l, 1), max(l - 1, 0)


def randu(state, d, total):
    """cv::randu(plane, 0, d) on a continuous 1 x total CV_8U plane: (values, the state after it)"""
    mode = randu_mode(d)
    out = np.empty(total, np.int64)
    x = state
    for j in range(0, total, BLOCK):
        n = min(BLOCK, total - j)
        if mode == "small":
            words = []
            for _ in range(n // 4):
                x = rng_next(x)
                words.append(x & MASK32)
            w = np.array(words, np.int64)
            out[j:j + 4 * len(words)] = np.stack([(w >> s) & (d - 1) for s in (0, 8, 16, 24)], -1).reshape(-1)
            for i in range(4 * len(words), n):
                x = rng_next(x)
                out[j + i] = (x & MASK32) & (d - 1)
        else:
            words = []
            for _ in range(n):
                x = rng_next(x)
                words.append(x & MASK32)
            if mode == "bits":
                out[j:j + n] = np.array(words, np.int64) & (d - 1)
            else:  # randi_: every line in 32-bit unsigned arithmetic
                Mv, sh1, sh2 = div_struct(d)
                vals = []
                for t0 in words:
                    v0 = (t0 * Mv) >> 32
                    v0 = ((v0 + (((t0 - v0) & MASK32) >> sh1)) & MASK32) >> sh2
                    vals.append((t0 - v0 * d) & MASK32)
                out[j:j + n] = vals
    return np.minimum(out, 255).astype(np.uint8), x


def periods_of(rate, nN):
    """(nShortUpdate, nMidUpdate, nLongUpdate) of apply :764-773; ValueError where the reference's casts are undefined"""
    l1 = math.log(1 - rate) if rate < 1 else -math.inf
    q = []
    for v in (0.7, 0.4, 0.1):
        if l1 == 0:
            raise ValueError("rate 0")
        x = math.log(v) / l1
        if not (0 <= x <= 2147483645.0):
            raise ValueError("a K quotient does not fit an int")
        q.append(int(x))
    Kshort = q[0] + 1
    Kmid = q[1] - Kshort + 1
    Klong = q[2] - Kshort - Kmid + 1
    return Kshort // nN + 1, Kmid // nN + 1, Klong // nN + 1


class KNN:
    def __init__(self, history=500, nsamples=7, knn_samples=2, detect_shadows=1, shadow_value=127,
                 dist2_threshold=400.0, shadow_threshold=0.5, rng_state=0xffffffff):
        self.history, self.nN, self.nkNN = int(history), int(nsamples), int(knn_samples)
        self.detect_shadows, self.shadow_value = bool(detect_shadows), int(shadow_value) & 255
        self.Tb, self.tau = F(dist2_threshold), F(shadow_threshold)
        self.rng = int(rng_state)
        self.nframes = 0
        self.shape = None
        self.counters = [0, 0, 0]   # short, mid, long
        self.periods = []           # per frame
        self.fills = []             # (frame, plane, d, mode)
        self.counts = dict.fromkeys(COUNT_KEYS, 0)

    def _initialize(self, shape):
        self.shape = shape
        self.cn = 1 if len(shape) == 2 else shape[2]
        n = shape[0] * shape[1]
        self.samples = np.zeros((n, 3 * self.nN, self.cn + 1), np.uint8)
        self.index = np.zeros((3, n), np.uint8)
        self.next = np.zeros((3, n), np.uint8)
        self.counters = [0, 0, 0]
        self.nframes = 0

    def reset(self):
        self.nframes = 0

    def apply(self, frame, learning_rate=-1.0):
        frame = np.asarray(frame)
        assert frame.dtype == np.uint8
        if math.isnan(learning_rate) or learning_rate == 0 or learning_rate > 1:
            raise ValueError("a learning rate the reference has no defined result for")
        if self.nframes == 0 or learning_rate >= 1 or frame.shape != self.shape:
            self._initialize(frame.shape)
        self.nframes += 1
        rate = learning_rate if learning_rate >= 0 and self.nframes > 1 else 1.0 / min(2 * self.nframes, self.history)
        per = periods_of(rate, self.nN)
        self.periods.append(per)
        mask = self._pixels(frame.reshape(-1, self.cn))
        for k, name in enumerate(("short", "mid", "long")):
            self.counters[k] += 1
            if self.counters[k] >= per[k]:
                self.counters[k] = 0
                self.next[k], self.rng = randu(self.rng, per[k], self.next.shape[1])
                mode = randu_mode(per[k])
                self.counts["fills_" + mode] += 1
                self.fills.append((len(self.periods), name, per[k], mode))
        return mask.reshape(self.shape[:2])

    def _pixels(self, data):
        n, cn, nN, total = data.shape[0], self.cn, self.nN, 3 * self.nN
        S, cnt = self.samples, self.counts
        d = data.astype(F)
        Pbf, Pb = np.zeros(n, np.int64), np.zeros(n, np.int64)
        bg = np.zeros(n, bool)
        for k in range(total):
            live = ~bg
            if not live.any():
                break
            dist2 = np.zeros(n, F)
            for c in range(cn):
                dd = S[:, k, c].astype(F) - d[:, c]
                dist2 = dist2 + dd * dd
            near = live & (dist2 < self.Tb)
            Pbf += near
            flagged = near & (S[:, k, cn] != 0)
            Pb += flagged
            bg |= flagged & (Pb >= self.nkNN)
        include = bg | (Pbf >= self.nkNN)
        cnt["early_backgrounds"] += int(bg.sum())
        cnt["include_by_pbf"] += int((~bg & include).sum())

        verdict = np.where(bg, 1, 0)
        if self.detect_shadows:
            open_ = ~bg
            Ps = np.zeros(n, np.int64)
            with np.errstate(all="ignore"):
                for k in range(total):
                    live = open_ & (S[:, k, cn] != 0)
                    if not open_.any():
                        break
                    num, den = np.zeros(n, F), np.zeros(n, F)
                    for c in range(cn):
                        m = S[:, k, c].astype(F)
                        num = num + d[:, c] * m
                        den = den + m * m
                    zero = live & (den == 0)
                    cnt["zero_denominators"] += int(zero.sum())
                    open_ &= ~zero
                    live &= ~zero
                    inr = live & (num <= den) & (num >= self.tau * den)
                    a = (num / den).astype(F)
                    dist2a = np.zeros(n, F)
                    for c in range(cn):
                        dD = a * S[:, k, c].astype(F) - d[:, c]
                        dist2a = dist2a + dD * dD
                    yes = inr & (dist2a < self.Tb * a * a)
                    Ps += yes
                    sh = yes & (Ps >= self.nkNN)
                    verdict[sh] = 2
                    open_ &= ~sh
        cnt["shadows"] += int((verdict == 2).sum())
        cnt["foreground"] += int((verdict == 0).sum())

        # the update: offsets from the indices as they are before it; long, then mid, then short
        P = np.arange(n)
        oS = self.index[0].astype(np.int64)
        oM = self.index[1].astype(np.int64) + nN
        oL = self.index[2].astype(np.int64) + 2 * nN
        uS = self.next[0] == self.counters[0]
        uM = self.next[1] == self.counters[1]
        uL = self.next[2] == self.counters[2]
        S[P[uL], oL[uL]] = S[P[uL], oM[uL]]
        S[P[uM], oM[uM]] = S[P[uM], oS[uM]]
        S[P[uS], oS[uS], :cn] = data[uS]
        S[P[uS], oS[uS], cn] = include[uS]
        for k, u in enumerate((uS, uM, uL)):
            i = self.index[k]
            self.index[k] = np.where(u, np.where(i >= nN - 1, 0, i + 1), i).astype(np.uint8)
        cnt["short_updates"] += int(uS.sum())
        cnt["mid_updates"] += int(uM.sum())
        cnt["long_updates"] += int(uL.sum())
        return np.where(verdict == 1, 0, np.where(verdict == 2, self.shadow_value, 255)).astype(np.uint8)

    def background_image(self):
        S, cn = self.samples, self.cn
        flag = S[:, :, cn] != 0
        first = flag.argmax(1)
        v = S[np.arange(S.shape[0]), first, :cn] * flag.any(1)[:, None]
        return v.astype(np.uint8).reshape(self.shape)

    def model(self):
        """(samples (h, w, 3 nN, cn + 1), index (3, h, w), next (3, h, w), counters (3,) int32, rng state)"""
        h, w = self.shape[:2]
        return (self.samples.reshape(h, w, 3 * self.nN, self.cn + 1).copy(), self.index.reshape(3, h, w).copy(),
                self.next.reshape(3, h, w).copy(), np.array(self.counters, np.int32), self.rng)


def run_case(case, params, frames):
    """(masks (n, h, w), {frame: background}, KNN) of a case of tests/_knn_cases.py"""
    m = KNN(**params)
    masks, bgs = [], {}
    for t in range(case["n"]):
        masks.append(m.apply(frames[t], float(case["rates"][t])))
        if t + 1 in case["bg"]:
            bgs[t + 1] = m.background_image()
    return np.stack(masks), bgs, m


@functools.lru_cache(maxsize=None)
def expected(i):
    """(masks, {frame: background}, model, counts, periods, fills) of recorded case i, computed once and shared:
    do not modify"""
    import _knn_cases as KC

    case = KC.cases()[i]
    masks, bgs, m = run_case(case, KC.params(case), KC.case_frames(case))
    return masks, bgs, m.model(), dict(m.counts), np.array(m.periods, np.int32), tuple(m.fills)
