"""numpy restatement of cv::BackgroundSubtractorMOG2 (video/src/bgfg_gaussmix2.cpp: apply :845-882,
MOG2Invoker::operator() :568-753, detectShadowGMM :476-521, getBackgroundImage_intern :884-925), vectorised over
pixels with a loop over modes.  Every operation is float32, once, in the reference's order.  The model is kept in
the reference's layout: weight[h][w][K], variance[h][w][K], mean[h][w][K][cn], modes_used[h][w]."""
import functools

import numpy as np

F = np.float32
EVENTS = ("fits", "new_modes", "replacements", "prunes", "fit_sorts", "new_sorts", "shadows", "foreground",
          "var_max_clamps", "var_min_clamps", "zero_denominators")
FLT_EPSILON = np.finfo(np.float32).eps


def saturate_u8(x):
    """saturate_cast<uchar>(float): round half to even, clamped; NaN gives 0"""
    with np.errstate(invalid="ignore"):
        r = np.rint(x)
        return np.where(r > 0, np.minimum(r, 255), 0).astype(np.uint8)


class MOG2:
    def __init__(self, history=500, nmixtures=5, detect_shadows=1, shadow_value=127, var_threshold=16.0,
                 var_threshold_gen=9.0, var_init=15.0, var_min=4.0, var_max=75.0, background_ratio=0.9,
                 complexity_reduction=0.05, shadow_threshold=0.5):
        self.history, self.K = int(history), int(nmixtures)
        self.detect_shadows, self.shadow_value = int(detect_shadows), int(shadow_value) & 255
        self.var_threshold = float(var_threshold)  # a double in the reference; the others are floats
        self.Tg, self.var_init, self.var_min, self.var_max = F(var_threshold_gen), F(var_init), F(var_min), F(var_max)
        self.TB, self.fCT, self.tau = F(background_ratio), F(complexity_reduction), F(shadow_threshold)
        self.nframes = 0
        self.shape = None
        self.counts = dict.fromkeys(EVENTS, 0)
        self.rate = None

    def _init(self, shape, dtype):
        self.shape, self.dtype = shape, dtype
        h, w = shape[:2]
        cn = 1 if len(shape) == 2 else shape[2]
        n = h * w
        self.cn = cn
        self.weight = np.zeros((n, self.K), F)
        self.variance = np.zeros((n, self.K), F)
        self.mean = np.zeros((n, self.K, cn), F)
        self.modes_used = np.zeros(n, np.int32)
        self.nframes = 0

    def reset(self):
        self.nframes = 0

    def model(self):
        h, w = self.shape[:2]
        return (self.weight.reshape(h, w, self.K).copy(), self.variance.reshape(h, w, self.K).copy(),
                self.mean.reshape(h, w, self.K, self.cn).copy(), self.modes_used.reshape(h, w).astype(np.uint8))

    def _swap(self, idx, i, j):
        for a in (self.weight, self.variance, self.mean):
            t = a[idx, i].copy()
            a[idx, i] = a[idx, j]
            a[idx, j] = t

    def apply(self, frame, learning_rate=-1.0):
        frame = np.asarray(frame)
        assert frame.dtype in (np.uint8, np.float32)
        if self.nframes == 0 or learning_rate >= 1 or frame.shape != self.shape or frame.dtype != self.dtype:
            self._init(frame.shape, frame.dtype)
        self.nframes += 1
        rate = learning_rate if learning_rate >= 0 and self.nframes > 1 else 1.0 / min(2 * self.nframes, self.history)
        self.rate = rate
        alphaT = F(rate)
        alpha1 = F(1) - alphaT
        prune = F(-rate * float(self.fCT))
        Tb, TB, Tg = F(self.var_threshold), self.TB, self.Tg
        var_min, var_max = min(self.var_min, self.var_max), max(self.var_min, self.var_max)
        K, cn, cnt = self.K, self.cn, self.counts
        Wt, V, M = self.weight, self.variance, self.mean
        n = Wt.shape[0]
        d = frame.reshape(n, cn).astype(F)
        nm = self.modes_used.copy()
        rows = np.arange(n)
        background, fits = np.zeros(n, bool), np.zeros(n, bool)
        total = np.zeros(n, F)
        with np.errstate(all="ignore"):
            for mode in range(K):
                act = mode < nm
                if not act.any():
                    break
                weight = alpha1 * Wt[:, mode] + prune
                pos = np.full(n, mode)
                test = act & ~fits
                var = V[:, mode].copy()
                dD = M[:, mode, :] - d
                dist2 = np.zeros(n, F)
                for c in range(cn):
                    dist2 = dist2 + dD[:, c] * dD[:, c]
                background |= test & (total < TB) & (dist2 < Tb * var)
                fit = test & (dist2 < Tg * var)
                fits |= fit
                cnt["fits"] += int(fit.sum())
                weight = np.where(fit, weight + alphaT, weight)
                k = alphaT / weight
                M[fit, mode, :] = (M[:, mode, :] - k[:, None] * dD)[fit]
                varnew = var + k * (dist2 - var)
                lo = fit & (varnew < var_min)
                varnew = np.where(varnew < var_min, var_min, varnew)
                hi = fit & (varnew > var_max)
                varnew = np.where(varnew > var_max, var_max, varnew)
                cnt["var_min_clamps"] += int(lo.sum())
                cnt["var_max_clamps"] += int(hi.sum())
                V[fit, mode] = varnew[fit]
                moving = fit.copy()
                for i in range(mode, 0, -1):
                    moving &= ~(weight < Wt[:, i - 1])
                    idx = np.flatnonzero(moving)
                    if idx.size == 0:
                        break
                    self._swap(idx, i, i - 1)
                    pos[idx] = i - 1
                cnt["fit_sorts"] += int((fit & (pos != mode)).sum())
                pr = act & (weight < -prune)
                cnt["prunes"] += int(pr.sum())
                weight = np.where(pr, F(0), weight)
                nm = nm - pr
                Wt[rows[act], pos[act]] = weight[act]
                total = np.where(act, total + weight, total)

            inv = np.where(np.abs(total) > FLT_EPSILON, F(1) / total, F(0)).astype(F)
            for mode in range(K):
                a = mode < nm
                Wt[a, mode] = (Wt[:, mode] * inv)[a]

            new = ~fits if alphaT > 0 else np.zeros(n, bool)
            if new.any():
                full = new & (nm == K)
                cnt["new_modes"] += int(new.sum())
                cnt["replacements"] += int(full.sum())
                mode = np.where(full, K - 1, nm)
                nm = nm + (new & ~full)
                one = new & (nm == 1)
                many = new & ~one
                for j in range(K):
                    dec = many & (j < nm - 1)
                    Wt[dec, j] = (Wt[:, j] * alpha1)[dec]
                r = rows[new]
                Wt[r, mode[new]] = np.where(one[new], F(1), alphaT)
                V[r, mode[new]] = self.var_init
                M[r, mode[new], :] = d[new]
                moving = new.copy()
                moved = np.zeros(n, bool)
                for i in range(K - 1, 0, -1):
                    on = moving & (i <= nm - 1)
                    stop = on & (alphaT < Wt[:, i - 1])
                    moving &= ~stop
                    idx = np.flatnonzero(on & ~stop)
                    if idx.size:
                        self._swap(idx, i, i - 1)
                        moved[idx] = True
                cnt["new_sorts"] += int(moved.sum())

            self.modes_used = nm
            mask = np.where(background, 0, 255).astype(np.uint8)
            if self.detect_shadows:
                sh = self._shadow(d, nm, ~background, Tb)
                mask[sh] = self.shadow_value
                cnt["shadows"] += int(sh.sum())
                cnt["foreground"] += int((~background & ~sh).sum())
            else:
                cnt["foreground"] += int((~background).sum())
        return mask.reshape(self.shape[:2])

    def _shadow(self, d, nm, todo, Tb):
        n = d.shape[0]
        Wt, V, M = self.weight, self.variance, self.mean
        verdict = np.where(todo, -1, 0)
        tW = np.zeros(n, F)
        for mode in range(self.K):
            live = (verdict < 0) & (mode < nm)
            if not live.any():
                break
            num, den = np.zeros(n, F), np.zeros(n, F)
            for c in range(self.cn):
                num = num + d[:, c] * M[:, mode, c]
                den = den + M[:, mode, c] * M[:, mode, c]
            zero = live & (den == 0)
            self.counts["zero_denominators"] += int(zero.sum())
            verdict[zero] = 0
            live &= ~zero
            inr = live & (num <= den) & (num >= self.tau * den)
            a = num / den
            dist2a = np.zeros(n, F)
            for c in range(self.cn):
                dDc = a * M[:, mode, c] - d[:, c]
                dist2a = dist2a + dDc * dDc
            yes = inr & (dist2a < Tb * V[:, mode] * a * a)
            verdict[yes] = 1
            live &= ~yes
            tW = np.where(live, tW + Wt[:, mode], tW)
            verdict[live & (tW > self.TB)] = 0
        return verdict == 1

    def background_image(self):
        n = self.weight.shape[0]
        acc = np.zeros((n, self.cn), F)
        total = np.zeros(n, F)
        live = np.ones(n, bool)
        with np.errstate(all="ignore"):
            for mode in range(self.K):
                on = live & (mode < self.modes_used)
                if not on.any():
                    break
                w = self.weight[:, mode]
                acc = np.where(on[:, None], acc + w[:, None] * self.mean[:, mode, :], acc)
                total = np.where(on, total + w, total)
                live &= ~(on & (total > self.TB))
            inv = np.where(np.abs(total) > FLT_EPSILON, F(1) / total, F(0)).astype(F)
            out = acc * inv[:, None]
        if self.dtype == np.uint8:
            out = saturate_u8(out)
        return out.reshape(self.shape)


@functools.lru_cache(maxsize=None)
def expected(i):
    """(masks, {frame: background}, model, counts) of recorded case i, computed once and shared: do not modify"""
    import _mog2_cases as GC

    case = GC.cases()[i]
    masks, bgs, m = run_case(case, GC.params(case), GC.case_frames(case))
    return masks, bgs, m.model(), dict(m.counts)


def run_case(case, params, frames):
    """(masks (n, h, w), {frame: background}, MOG2) of a case of tests/_mog2_cases.py"""
    m = MOG2(**params)
    masks, bgs = [], {}
    for t in range(case["n"]):
        masks.append(m.apply(frames[t], float(case["rates"][t])))
        if t + 1 in case["bg"]:
            bgs[t + 1] = m.background_image()
    return np.stack(masks), bgs, m
