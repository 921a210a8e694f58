"""The case table of tests/test_gpu_streams.py: every stream-taking entry point
of include/tbdk.h on a side stream behind a late producer (tests/_streams.py).

A case is a short sequence of library calls (most have one).  For call i it
names the real inputs and a decoy of the same shapes and types, the oracle that
turns inputs into the reference, the closure that makes the call on the stream,
and the comparison: the one the entry point already has in its own test_gpu_*
file, bit for bit.  tests/test_streams_cases.py checks on the CPU, from the
oracle alone, that the decoy gives another answer than the real inputs, that
the real case is active, and that every `tbdk_*` symbol of the header that takes
a `void* stream` is named here, by a case or by an exclusion with its reason.

Shapes are the smallest the suite already has (tests/test_gpu_dirty_state.py's
160x120 frame and ROIs, its Farneback / dense PyrLK pairs, HOG frames, front-end
sizes and pyramid frames).

sync: the header (or wrapper docstring) line by which the call is documented
as synchronising; such a case gets the ordering check only.  None: the call is
asynchronous and also gets the asynchrony check.
keep: inputs that the header says must outlive the call, with the line."""
from dataclasses import dataclass, field

import numpy as np

import _frontend_oracle as FE
import _gftt_f32_oracle as O32
import _gftt_mask_cases as MC
import _gftt_mask_oracle as MO
import _klt_tracker_oracle as KO
import _mog2_cases as GC
import _mog2_oracle as M2
import _oracle as O
import test_gpu_dirty_state as D
from _streams import POISON
from test_gpu_extreme import _reflect_frame, same_bits
from test_gpu_klt import assert_exact

SYNC_HOG = "tbdk.h, tbdk_hog_detect_multiscale: \"Synchronous: returns when the results are in the host buffers.\""
SYNC_HOG_DETECT = "tbdk.h, tbdk_hog_detect: \"window corners (x, y) and scores in window order; synchronous.\""
SYNC_FRONT_NEW = "tbdk.h, tbdk_resize_linear_u8: \"A new size synchronises `stream` once and uploads its tables\""
SYNC_STEP = "tbdk.h, tbdk_tbd_step: \"Synchronises the stream once (predictions -> host tracker).\""
# the header documents the other two through tbdk_tbd_step: both lines are cited, and both are checked
SYNC_STEP_AHEAD = ("tbdk.h, tbdk_tbd_step_ahead: \"tbdk_tbd_step when the next frame is already on the device\"; "
                   "tbdk_tbd_step: \"Synchronises the stream once (predictions -> host tracker).\"")
SYNC_RUN = ("tbdk.h, tbdk_tbd_run: \"Equivalent to tbdk_tbd_step_ahead over the sequence.\"; " +
            SYNC_STEP_AHEAD[len("tbdk.h, "):])
SYNC_STEP_IMAGE = "tbdk.h, tbdk_tbd_step_image: \"Synchronous, as HOG is.\""
KEEP_BORROWED = ("tbdk.h, tbdk_pyr_build_borrowed: \"The frame must stay valid and unchanged while the pyramid "
                 "is read\"")
KEEP_NEXT = ("tbdk.h, tbdk_tbd_step_ahead: \"next_frame must keep its pixels until the next step, which must pass "
             "the same pointer\"")


def K():
    from opencv_amd import klt

    return klt


def farneback_module():
    from opencv_amd import farneback

    return farneback


def hog_module():
    from opencv_amd import hog

    return hog


def flip(a):
    return np.ascontiguousarray(a[::-1, ::-1])


def flat(v):
    """the arrays of a nest of tuples / lists / dicts, in order"""
    if isinstance(v, dict):
        v = list(v.values())
    if isinstance(v, (tuple, list)):
        return [x for e in v for x in flat(e)]
    return [np.asarray(v)]


def differs_any(a, b):
    fa, fb = flat(a), flat(b)
    return len(fa) != len(fb) or any(x.shape != y.shape or not np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
                                     for x, y in zip(fa, fb))


def flow_differs(a, b):
    """two flows differ in at least 1 % of the pixels"""
    fa, fb = np.asarray(flat(a)[0]), np.asarray(flat(b)[0])
    return fa.shape != fb.shape or (fa.reshape(-1, 2) != fb.reshape(-1, 2)).any(1).mean() >= 0.01


def check_bits(got, ref, what):
    g, r = flat(got), flat(ref)
    assert len(g) == len(r), f"{what}: {len(g)} outputs vs {len(r)}"
    for i, (x, y) in enumerate(zip(g, r)):
        same_bits(x, y, f"{what}: output {i}")


@dataclass
class Case:
    name: str
    symbols: tuple
    inputs: object                  # which ("real" / "decoy") -> [ {name: array} per call ]
    oracle: object                  # [ {name: array} per call ] -> [ reference per call ]
    run: object                     # (ctx, state, S, bufs, outs, i) -> the outputs of call i
    check: object = check_bits      # (got, reference of call i, what)
    differs: object = differs_any   # (reference of the real inputs, of the decoy) -> bool, per call
    active: object = None           # (references of the real inputs) -> bool
    setup: object = None            # (ctx) -> state, before the stream is blocked
    outs: object = None             # (i) -> {name: (shape, torch dtype name)} caller-owned outputs
    keep: dict = field(default_factory=dict)
    sync: str = None
    options: dict = field(default_factory=dict)
    poison: bool = True             # outputs are the caller's: poison them after the consumer
    prefill: object = None          # (state) -> None: poisons library-owned output memory before the spin
    called: object = None           # (i) -> the symbols call i reaches; None: all of `symbols`

    def symbols_of(self, i):
        return tuple(self.symbols if self.called is None else self.called(i))


CASES = []
_refs = {}


def add(case):
    assert case.name not in [c.name for c in CASES], case.name
    CASES.append(case)
    return case


def refs(case, which):
    """the oracle's result for the case's real or decoy inputs, computed once and shared (read only)"""
    key = (case.name, which)
    if key not in _refs:
        _refs[key] = case.oracle(case.inputs(which))
    return _refs[key]


def one(real, decoy=None):
    """inputs of a one-call case; decoy None: every image flipped"""
    def inputs(which):
        r = real()
        if which == "real":
            return [r]
        return [decoy() if decoy is not None else {k: flip(v) for k, v in r.items()}]

    return inputs


def single(f):
    """an oracle of one call"""
    return lambda ins: [f(ins[0])]


def nonempty(refs_):
    return all(sum(x.size for x in flat(r)) > 0 for r in refs_)


# ---- pyramids ------------------------------------------------------------------------------------------

PYR_WIN, PYR_ML = (9, 9), 3


def _pyr_frame(kind):
    a, _ = D.pyr_frames()
    if kind == "cn3":
        return D.X.to_cn(a, 3)
    if kind == "f16_f16":
        return a.astype(np.float16)
    if kind == "f32_u16":
        return D.X.to_u16(a, 65535)
    if kind == "f32_f32":
        return (a.astype(np.float32) * np.float32(1.0 / 255))
    return a


def _pyr_oracle(kind):
    def f(i):
        img = i["img"]
        if kind in ("u8", "levels", "cn3", "borrowed"):
            R = O.Pyramid(img, PYR_WIN, PYR_ML)
            lv = [R.level(k) for k in range(R.nlevels)]
            dv = [O.scharr(L) for L in lv] if kind in ("u8", "cn3") else []
            return {"lv": lv[1:] if kind == "borrowed" else lv, "dv": dv}
        R = O.Pyramid16(img, PYR_WIN, PYR_ML, f32=kind.startswith("f32"))
        return {"lv": list(R.levels), "dv": list(R.derivs)}

    return single(f)


def _pyr_setup(kind):
    def setup(ctx):
        import torch

        dt = torch.float16 if kind.startswith("f16") else torch.float32 if kind.startswith("f32") else torch.uint8
        return K().Pyramid(ctx, D.PW, D.PH, PYR_ML, PYR_WIN, dt, derivs=kind not in ("levels", "borrowed"),
                           channels=3 if kind == "cn3" else 1)

    return setup


def pyr_views(P, first=0):
    """device views (bytes) of the padded levels and derivative planes of a pyramid, and their geometry"""
    import torch

    k = K()
    lv, dv, geo = [], [], []
    for i in range(first, P.nlevels):
        L, Dv = P.pyr.lv[i], P.pyr.dv[i]
        lv.append(k._device_view(L.data, (L.height + 2 * L.pad, L.pitch), torch.uint8, P.ctx.device))
        if Dv.data:
            dv.append(k._device_view(Dv.data, (Dv.height + 2 * Dv.pad, Dv.pitch), torch.uint8, P.ctx.device))
        geo.append((L.width, L.height, L.pad))
    return {"lv": lv, "dv": dv, "geo": geo}


def poison_pyramid(P, first=0):
    """the poison byte over every level (border included) and the interior of every derivative plane of a
    pyramid, so that what a consumer sees after a build is the build's; the planes' zero frame, written once at
    creation (pyr_create), stays"""
    v = pyr_views(P, first)
    for t in v["lv"]:
        t.fill_(POISON)
    bpp = (8 if P.pyr.depth == 5 else 4) * P.channels  # an (Ix, Iy) pair of int16 / fp16 or of fp32, per channel
    for t, (w, h, pad) in zip(v["dv"], v["geo"]):
        t[pad:pad + h, pad * bpp:(pad + w) * bpp].fill_(POISON)


def _pyr_run(kind):
    def run(ctx, P, S, b, o, i):
        if kind == "borrowed":
            P.build_borrowed(b["img"], stream=S)
            return pyr_views(P, 1)
        P.build(b["img"], stream=S)
        return pyr_views(P)

    return run


def _pyr_check(kind):
    dt = np.float16 if kind.startswith("f16") else np.float32 if kind.startswith("f32") else np.uint8
    ddt = np.int16 if dt == np.uint8 else dt
    cn = 3 if kind == "cn3" else 1

    def check(got, ref, what):
        assert len(got["lv"]) == len(ref["lv"]) and len(got["dv"]) == len(ref["dv"]), f"{what}: level count"
        for k, (raw, want) in enumerate(zip(got["lv"], ref["lv"])):
            w, h, pad = got["geo"][k]
            g = np.ascontiguousarray(raw[:, :(w + 2 * pad) * cn * dt().itemsize]).view(dt)
            g = g.reshape((h + 2 * pad, w + 2 * pad) + ((cn,) if cn > 1 else ()))
            same_bits(g, _reflect_frame(want, pad), f"{what}: level {k} with border")
        for k, (raw, want) in enumerate(zip(got["dv"], ref["dv"])):
            w, h, pad = got["geo"][k]
            bpp = 2 * cn * ddt().itemsize
            g = np.ascontiguousarray(raw[pad:pad + h, pad * bpp:(pad + w) * bpp]).view(ddt).reshape(h, w, 2 * cn)
            same_bits(g, want, f"{what}: derivative plane {k}")

    return check


for _kind, _sym in (("u8", "tbdk_pyr_build"), ("levels", "tbdk_pyr_build"), ("cn3", "tbdk_pyr_build"),
                    ("f16_u8", "tbdk_pyr_build"), ("f16_f16", "tbdk_pyr_build_f16"), ("f32_u16", "tbdk_pyr_build_u16"),
                    ("f32_f32", "tbdk_pyr_build_f32"), ("borrowed", "tbdk_pyr_build_borrowed")):
    add(Case(f"pyramid_{_kind}", (_sym,), one(lambda k=_kind: {"img": _pyr_frame(k)}), _pyr_oracle(_kind),
             _pyr_run(_kind), _pyr_check(_kind), setup=_pyr_setup(_kind), poison=False,
             prefill=lambda P, k=_kind: poison_pyramid(P, 1 if k == "borrowed" else 0),
             keep={"img": KEEP_BORROWED} if _kind == "borrowed" else {}))

add(Case("pyr_down", ("tbdk_pyr_down_u8",), one(lambda: {"img": D.small_frame()}),
         single(lambda i: O.pyr_down(i["img"])),
         lambda ctx, st, S, b, o, i: K().pyr_down(b["img"], ctx=ctx, stream=S)))


# ---- sparse PyrLK ----------------------------------------------------------------------------------------

LK_WIN, LK_ML = (9, 9), 2


def _lk_inputs(kind):
    def real():
        a, b = D.pyr_frames()
        r = {"a": a, "b": b, "pts": D.border_points()}
        if kind == "init":
            r["init"] = (r["pts"] + np.float32([0.75, -0.5])).astype(np.float32)
        if kind == "cn3":
            r["a"], r["b"] = D.X.to_cn(a, 3), D.X.to_cn(b, 3)
        if kind == "f32cn3":
            r["a"], r["b"] = D.X.to_u16(D.X.to_cn(a, 3), 65535), D.X.to_u16(D.X.to_cn(b, 3), 65535)
        return r

    def decoy():
        r = real()
        d = {"a": flip(r["b"]), "b": flip(r["a"]),
             "pts": np.ascontiguousarray((r["pts"][::-1] * np.float32(0.5) + np.float32(7)).astype(np.float32))}
        if "init" in r:
            d["init"] = (d["pts"] - np.float32([1.25, 0.5])).astype(np.float32)
        return d

    return one(real, decoy)


def _lk_oracle(kind):
    def f(i):
        init = i.get("init")
        flags = O.OPTFLOW_USE_INITIAL_FLOW if init is not None else 0
        if kind in ("f16", "f32", "f32cn3"):
            f32 = kind != "f16"
            return O.lk16(O.Pyramid16(i["a"], LK_WIN, LK_ML, f32=f32), O.Pyramid16(i["b"], LK_WIN, LK_ML, f32=f32),
                          i["pts"], LK_WIN, LK_ML)
        Pa, Pb = O.Pyramid(i["a"], LK_WIN, LK_ML), O.Pyramid(i["b"], LK_WIN, LK_ML)
        if kind == "fb":
            import _fb_oracle as FBO

            return FBO.checked_trace(Pa, Pb, i["pts"], LK_WIN[0], LK_ML, 30, 0.01, 1e-4, 1.0, O.ACCUM_EXACT)
        return O.lk(Pa, Pb, i["pts"], LK_WIN, LK_ML, 30, 0.01, flags, accum=O.ACCUM_EXACT, init=init)

    return single(f)


def _lk_setup(kind):
    def setup(ctx):
        import torch

        k = K()
        dt = {"f16": torch.float16, "f32": torch.float32, "f32cn3": torch.float32}.get(kind, torch.uint8)
        cn = 3 if kind in ("cn3", "f32cn3") else 1
        pyr = [k.Pyramid(ctx, D.PW, D.PH, LK_ML, LK_WIN, dt, channels=cn) for _ in range(2)]
        return pyr, k.SparsePyrLKOpticalFlow(LK_WIN, LK_ML, 30, useInitialFlow=kind == "init")

    return setup


def _lk_run(kind):
    def run(ctx, st, S, b, o, i):
        (Pa, Pb), lk = st
        Pa.build(b["a"], stream=S)
        Pb.build(b["b"], stream=S)
        if kind == "fb":
            r = lk.calc_checked(Pa, Pb, b["pts"], back_threshold=1.0, want_iters=True, stream=S)
            return {"next_pts": r.next_pts, "status": r.status, "err": r.err, "iters": r.iters,
                    "back_pts": r.back_pts, "fb_err": r.fb_err}
        r = lk.calc(Pa, Pb, b["pts"], b.get("init"), want_iters=True, stream=S)
        return (r.next_pts, r.status, r.err, r.iters)

    return run


def _lk_check(kind):
    def check(g, ref, what):
        if kind == "fb":
            from test_gpu_lk_fb import back_equal

            same_bits(g["status"], ref.status, f"{what}: checked status")
            same_bits(g["iters"], ref.iters, f"{what}: iters")
            ok = ref.fwd_status == 1
            same_bits(g["next_pts"][ok], ref.next_pts[ok], f"{what}: next_pts of the points tracked forward")
            back_equal(g, ref)
        elif kind in ("f16", "f32cn3"):  # tests/test_gpu_f16.py assert_same; test_gpu_dirty_state.py (fp32, channels)
            for k, part in enumerate(("next_pts", "status", "err", "iters")):
                same_bits(g[k], ref[k], f"{what}: {part}")
        elif kind == "f32":  # tests/test_gpu_f32.py
            ok = ref[1] == 1
            same_bits(g[1], ref[1], f"{what}: status")
            same_bits(g[3], ref[3], f"{what}: iters")
            same_bits(g[0][ok], ref[0][ok], f"{what}: next_pts of the tracked points")
            same_bits(g[2][ok], ref[2][ok], f"{what}: err of the tracked points")
        else:
            assert_exact(tuple(g), ref)

    return check


def _lk_status(kind):
    return lambda r: (r[0].status if kind == "fb" else r[0][1]).sum() > 0


for _kind, _sym in (("plain", "tbdk_lk_sparse"), ("init", "tbdk_lk_sparse"), ("cn3", "tbdk_lk_sparse"),
                    ("f16", "tbdk_lk_sparse"), ("f32", "tbdk_lk_sparse"), ("f32cn3", "tbdk_lk_sparse"),
                    ("fb", "tbdk_lk_sparse_fb")):
    add(Case(f"lk_sparse_{_kind}", (_sym, "tbdk_pyr_build_u16" if _kind == "f32cn3" else "tbdk_pyr_build"),
             _lk_inputs(_kind), _lk_oracle(_kind), _lk_run(_kind), _lk_check(_kind), setup=_lk_setup(_kind),
             prefill=lambda st: [poison_pyramid(P) for P in st[0]],
             active=_lk_status(_kind)))


# ---- dense PyrLK -----------------------------------------------------------------------------------------

def _dense_oracle(win, ml):
    def f(i):
        a, b = i["a"], i["b"]
        h, w = a.shape
        ys, xs = np.mgrid[0:h, 0:w]
        pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
        nx, st, _, _ = O.lk(O.Pyramid(a, win, ml), O.Pyramid(b, win, ml), pts, win=win, max_level=ml,
                            accum=O.ACCUM_EXACT, want_err=False)
        return (nx - pts).astype(np.float32), st

    return single(f)


def _dense_setup(win, ml, size):
    def setup(ctx):
        k = K()
        return ([k.Pyramid(ctx, size[0], size[1], ml, win) for _ in range(2)],
                k.DensePyrLKOpticalFlow.create(win, ml, 30))

    return setup


def _dense_run(ctx, st, S, b, o, i):
    (Pa, Pb), lk = st
    Pa.build(b["a"], stream=S)
    Pb.build(b["b"], stream=S)
    return lk.calc(Pa, Pb, want_status=True, stream=S)


def _dense_check(g, ref, what):
    flow, st = g[0].reshape(-1, 2), g[1].ravel()
    same_bits(st, ref[1], f"{what}: status")
    same_bits(flow[ref[1] == 1], ref[0][ref[1] == 1], f"{what}: flow of the tracked pixels")


def _dense_differs(a, b):
    ok = (a[1] == 1) & (b[1] == 1)
    return (a[1] != b[1]).any() or ((a[0] != b[0]).any(1) & ok).mean() >= 0.01


def _dense_small():
    a, b = D.dense_pair()
    return {"a": a, "b": b}


def _dense_big():
    big = np.ascontiguousarray(D.large_frame()[:120, :160])
    return {"a": big, "b": np.ascontiguousarray(np.roll(big, (1, -2), axis=(0, 1)))}


for _name, _win, _ml, _size, _real in (("dense_lk_case_images_7", (7, 7), 2, (D.DW, D.DH), _dense_small),
                                       ("dense_lk_per_pixel_9x7", (9, 7), 2, (D.DW, D.DH), _dense_small),
                                       ("dense_lk_160x120_13", (13, 13), 3, (160, 120), _dense_big)):
    add(Case(_name, ("tbdk_lk_dense", "tbdk_pyr_build"), one(_real, lambda r=_real: {"a": flip(r()["b"]),
                                                                                      "b": flip(r()["a"])}),
             _dense_oracle(_win, _ml), _dense_run, _dense_check, _dense_differs, setup=_dense_setup(_win, _ml, _size),
             prefill=lambda st: [poison_pyramid(P) for P in st[0]],
             active=lambda r: r[0][1].sum() > 0))


# ---- GFTT and the corner response maps -----------------------------------------------------------------------

def _gftt_run(prm, rois, block=3, harris=False):
    def run(ctx, st, S, b, o, i):
        det = K().GoodFeaturesToTrackDetector(prm[0], prm[1], prm[2], block, harris, 0.04)
        return det.detect_rois(b["img"], rois, stream=S, mask=b.get("mask"))

    return run


def _gftt_check(g, ref, what):
    D.lists_same((g[0], g[1]), ref, what)


def _corners(refs_):
    return sum(len(r) for r in refs_[0]) > 0


def _lists_differ(a, b):
    return any(len(x) != len(y) or not np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


for _name, _opts in (("gftt_lds", {}), ("gftt_wide", {"gftt_wide": 1}), ("gftt_table_in_memory", {"gftt_inline": 0}),
                     ("gftt_dense_plane", {"gftt_compact": 0})):
    add(Case(_name, ("tbdk_gftt_rois",), one(lambda: {"img": D.small_frame()}),
             single(lambda i: O.gftt_rois(i["img"], D.ROIS, *D.GFTT_PRM, 3, False, 0.04)),
             _gftt_run(D.GFTT_PRM, D.ROIS), _gftt_check, _lists_differ, _corners, options=_opts))

BIG_ROI = [(3, 5, 150, 111)]
add(Case("gftt_one_larger_roi", ("tbdk_gftt_rois",), one(lambda: {"img": D.large_frame()}),
         single(lambda i: O.gftt_rois(i["img"], BIG_ROI, 300, 0.01, 1.0, 5, True, 0.04)),
         _gftt_run((300, 0.01, 1.0), BIG_ROI, 5, True), _gftt_check, _lists_differ, _corners))

add(Case("gftt_masked", ("tbdk_gftt_rois_masked",),
         one(lambda: {"img": D.small_frame(), "mask": MC.checker(160, 120, 8)},
             lambda: {"img": flip(D.small_frame()), "mask": np.ascontiguousarray(255 - MC.checker(160, 120, 8))}),
         single(lambda i: MO.gftt_rois_masked(i["img"], i["mask"], D.ROIS, *D.GFTT_PRM)),
         _gftt_run(D.GFTT_PRM, D.ROIS), _gftt_check, _lists_differ, _corners))


def _typed(depth):
    base = D.small_frame()
    return (base.astype(np.float32) * np.float32(1.0 / 255)) if depth == "32f" else base.astype(np.uint16) * np.uint16(257)


def _resp32(img, block, harris):
    with np.errstate(over="ignore", invalid="ignore"):
        return O32.response(img, block, harris, 0.04)


for _depth in ("32f", "16u"):
    add(Case(f"gftt_px_{_depth}", ("tbdk_gftt_rois_px",), one(lambda d=_depth: {"img": _typed(d)}),
             single(lambda i: O32.gftt_rois(i["img"], None, D.ROIS, *D.GFTT_PRM, 3, False, 0.04)),
             _gftt_run(D.GFTT_PRM, D.ROIS), _gftt_check, _lists_differ, _corners))
    add(Case(f"corner_response_px_{_depth}", ("tbdk_corner_response_px",), one(lambda d=_depth: {"img": _typed(d)}),
             single(lambda i: _resp32(i["img"], 5, True)),
             lambda ctx, st, S, b, o, i: K().corner_response(b["img"], 5, True, 0.04, ctx=ctx, stream=S)))

add(Case("corner_min_eigen_val", ("tbdk_corner_min_eig_val",), one(lambda: {"img": D.small_frame()}),
         single(lambda i: O.min_eig(i["img"])),
         lambda ctx, st, S, b, o, i: K().corner_min_eigen_val(b["img"], ctx=ctx, stream=S)))
add(Case("corner_response_harris5", ("tbdk_corner_response",), one(lambda: {"img": D.small_frame()}),
         single(lambda i: O.corner_response(i["img"], 5, True, 0.04)),
         lambda ctx, st, S, b, o, i: K().corner_response(b["img"], 5, True, 0.04, ctx=ctx, stream=S)))


# ---- the front end ---------------------------------------------------------------------------------------------

def _front_src(k):
    (sw, sh), d = D.FRONT_PAIRS[k]
    return FE.pattern(sw, sh, 3, 900 + k), d


def _u8_out(shape):
    return lambda i: {"dst": (shape, "uint8")}


for _k in (0, 3):  # 90x70 -> 31x20 and 50x40 -> 150x99
    _d = D.FRONT_PAIRS[_k][1]
    add(Case(f"resize_linear_{_d[0]}x{_d[1]}", ("tbdk_resize_linear_u8",), one(lambda k=_k: {"src": _front_src(k)[0]}),
             single(lambda i, d=_d: FE.resize_linear(i["src"], d)),
             lambda ctx, st, S, b, o, i, d=_d: K().resize_linear(b["src"], d, dst=o["dst"], ctx=ctx, stream=S),
             outs=_u8_out((_d[1], _d[0], 3))))
    add(Case(f"cvt_resize_gray_{_d[0]}x{_d[1]}", ("tbdk_cvt_resize_gray_u8",),
             one(lambda k=_k: {"src": _front_src(k)[0]}),
             single(lambda i, d=_d: FE.cvt_resize_gray(i["src"], FE.COLOR_BGR2GRAY, d)),
             lambda ctx, st, S, b, o, i, d=_d: K().cvt_resize_gray(b["src"], FE.COLOR_BGR2GRAY, d, dst=o["dst"], ctx=ctx,
                                                                   stream=S),
             outs=_u8_out((_d[1], _d[0]))))

NEW_SIZE = (57, 43)  # a destination no other test resizes 90x70 to: the first call uploads its tables
add(Case("resize_linear_new_size", ("tbdk_resize_linear_u8",), one(lambda: {"src": _front_src(0)[0]}),
         single(lambda i: FE.resize_linear(i["src"], NEW_SIZE)),
         lambda ctx, st, S, b, o, i: K().resize_linear(b["src"], NEW_SIZE, dst=o["dst"], ctx=ctx, stream=S),
         outs=_u8_out((NEW_SIZE[1], NEW_SIZE[0], 3)), sync=SYNC_FRONT_NEW,
         setup=lambda ctx: ctx.debug_fill_scratch(0)))  # forgets the table cache: the size is new again

add(Case("cvt_resize_gray_new_size", ("tbdk_cvt_resize_gray_u8",), one(lambda: {"src": _front_src(0)[0]}),
         single(lambda i: FE.cvt_resize_gray(i["src"], FE.COLOR_BGR2GRAY, NEW_SIZE)),
         lambda ctx, st, S, b, o, i: K().cvt_resize_gray(b["src"], FE.COLOR_BGR2GRAY, NEW_SIZE, dst=o["dst"], ctx=ctx,
                                                         stream=S),
         outs=_u8_out((NEW_SIZE[1], NEW_SIZE[0])), sync=SYNC_FRONT_NEW,
         setup=lambda ctx: ctx.debug_fill_scratch(0)))

for _code in ("BGR2GRAY", "BGR2BGRA"):
    _dcn = {"BGR2GRAY": 1, "BGR2BGRA": 4}[_code]
    add(Case(f"cvt_color_{_code}", ("tbdk_cvt_color_u8",), one(lambda: {"src": _front_src(0)[0]}),
             single(lambda i, c=_code: FE.cvt_color(i["src"], FE.CODES[c])),
             lambda ctx, st, S, b, o, i, c=_code: K().cvt_color(b["src"], FE.CODES[c], dst=o["dst"], ctx=ctx, stream=S),
             outs=_u8_out((70, 90) if _dcn == 1 else (70, 90, _dcn))))


# ---- Farneback ----------------------------------------------------------------------------------------------------

def _fb_inputs(init):
    def real():
        a, b = D.fb_pair()
        r = {"a": a, "b": b}
        if init:
            r["flow"] = D.fb_init()
        return r

    def decoy():
        r = real()
        d = {"a": flip(r["b"]), "b": flip(r["a"])}
        if init:
            d["flow"] = (-r["flow"] * np.float32(0.5)).astype(np.float32)
        return d

    return one(real, decoy)


def _fb_run(flags):
    def run(ctx, st, S, b, o, i):
        from opencv_amd import farneback as F

        fb = F.FarnebackOpticalFlow.create(ctx=ctx, numLevels=3, numIters=2, flags=flags)
        return fb.calc(b["a"], b["b"], b["flow"] if flags & O.OPTFLOW_USE_INITIAL_FLOW else o["flow"], stream=S)

    return run


for _variant, _flags in (("box", 0), ("gauss_init", O.FARNEBACK_GAUSSIAN | O.OPTFLOW_USE_INITIAL_FLOW)):
    for _ahead in (1, 0):
        _init = bool(_flags & O.OPTFLOW_USE_INITIAL_FLOW)
        add(Case(f"farneback_{_variant}_ahead{_ahead}", ("tbdk_farneback",), _fb_inputs(_init),
                 single(lambda i, fl=_flags: O.farneback(i["a"], i["b"], levels=3, iterations=2, flags=fl,
                                                         box_direct=not fl & O.FARNEBACK_GAUSSIAN,
                                                         init_flow=i.get("flow"))),
                 _fb_run(_flags), differs=flow_differs, options={"fb_prep_ahead": _ahead},
                 outs=(lambda i: {}) if _init else (lambda i: {"flow": ((D.FB_H, D.FB_W, 2), "float32")})))


def _fb_big():
    big = D.large_frame()
    return {"a": big, "b": np.ascontiguousarray(np.roll(big, (2, -3), axis=(0, 1)))}


def _fb_big_run(ctx, st, S, b, o, i):
    from opencv_amd import farneback as F

    fb = F.FarnebackOpticalFlow.create(ctx=ctx, numLevels=4, numIters=1, polyN=7, polySigma=1.5,
                                       flags=O.FARNEBACK_GAUSSIAN)
    return fb.calc(b["a"], b["b"], o["flow"], stream=S)


add(Case("farneback_320x240_gauss", ("tbdk_farneback",),
         one(_fb_big, lambda: {"a": flip(_fb_big()["b"]), "b": flip(_fb_big()["a"])}),
         single(lambda i: O.farneback(i["a"], i["b"], levels=4, iterations=1, poly_n=7, poly_sigma=1.5,
                                      flags=O.FARNEBACK_GAUSSIAN, box_direct=False)),
         _fb_big_run, differs=flow_differs, outs=lambda i: {"flow": ((240, 320, 2), "float32")}))

FB_STAGE = (97, 61)
add(Case("fb_level_image", ("tbdk_fb_level_image",), one(lambda: {"img": FE.pattern(*FB_STAGE, 1, 77)}),
         single(lambda i: O.fb_level_image(i["img"], (31, 20), 9, 1.5)),
         lambda ctx, st, S, b, o, i: farneback_module().level_image(
             b["img"], (31, 20), 9, 1.5, ctx=ctx, stream=S)))
add(Case("fb_poly_exp", ("tbdk_fb_poly_exp",), one(lambda: {"lvl": FE.pattern(*FB_STAGE, 1, 77).astype(np.float32)}),
         single(lambda i: O.fb_poly_exp(i["lvl"], 5, 1.1)),
         lambda ctx, st, S, b, o, i: farneback_module().poly_exp(
             b["lvl"], 5, 1.1, ctx=ctx, stream=S)))


# ---- HOG ------------------------------------------------------------------------------------------------------------

def _hog_obj(ctx, win, hit=None, levels=None):
    from test_gpu_hog import _hog

    hg = _hog(ctx, win)
    if levels is not None:
        hg.setNumLevels(levels)
        hg.setGroupThreshold(0)
    if hit is not None:
        hg.setHitThreshold(hit)
    return hg


def _hog_ms_oracle(win):
    def f(i):
        from test_gpu_hog import _prm

        hg = _hog_obj(None, win)
        r, w = O.hog_detect_multiscale(i["img"], _prm(hg), hg.svm, hit_threshold=D.HOG_HIT[win], nlevels=15,
                                       scale0=1.05, group_threshold=0)
        return sorted(zip(map(tuple, r.tolist()), w.tolist()))

    return single(f)


def _hog_ms_run(win):
    def run(ctx, st, S, b, o, i):
        hg = _hog_obj(ctx, win, D.HOG_HIT[win], 15)
        return [sorted(zip(*hg.detectMultiScale(b["img"], confidences=True, stream=S)))]

    return run


def _hog200():
    from test_gpu_hog import _bgr

    return {"img": _bgr(41, 200, 280, cn=3)}


def _hog320():
    from test_gpu_hog import _bgr

    return {"img": np.clip(_bgr(53, 320, 240, cn=3).astype(np.int32) * 3 // 2 + 40, 0, 255).astype(np.uint8)}


for _lanes in (1, 3):
    add(Case(f"hog_detect_multiscale_lanes{_lanes}", ("tbdk_hog_detect_multiscale",), one(_hog200),
             _hog_ms_oracle((64, 128)), _hog_ms_run((64, 128)), lambda g, ref, what: D.hog_same(g[0], ref, what),
             differs=lambda a, b: a != b, active=lambda r: len(r[0]) > 0, sync=SYNC_HOG,
             options={"hog_level_streams": _lanes}))
add(Case("hog_detect_multiscale_320x240_48x96", ("tbdk_hog_detect_multiscale",), one(_hog320),
         _hog_ms_oracle((48, 96)), _hog_ms_run((48, 96)), lambda g, ref, what: D.hog_same(g[0], ref, what),
         differs=lambda a, b: a != b, active=lambda r: len(r[0]) > 0, sync=SYNC_HOG))


def _hog96():
    from test_gpu_hog import _bgr

    w, h = D.X.HOG_SIZE
    return {"img": _bgr(43, w, h, cn=3)}


def _hog_detect_oracle(i):
    from test_gpu_hog import _prm

    hg = _hog_obj(None, (64, 128))
    return O.hog_detect(i["img"], _prm(hg), hg.svm, hit_threshold=-1e9)


def _hog_detect_check(g, ref, what):
    same_bits(np.array(g[0][0], np.int32).reshape(-1, 2), ref[0], f"{what}: window positions")
    same_bits(np.array(g[0][1], np.float64), ref[1], f"{what}: window scores")


add(Case("hog_detect", ("tbdk_hog_detect",), one(_hog96), single(_hog_detect_oracle),
         lambda ctx, st, S, b, o, i: [_hog_obj(ctx, (64, 128), -1e9).detect(b["img"], confidences=True, stream=S)],
         _hog_detect_check, active=lambda r: len(r[0][0]) > 0, sync=SYNC_HOG_DETECT))


def _hog_gray():
    from test_gpu_hog import _bgr

    return _bgr(47, 151, 97, cn=1)


add(Case("hog_resize", ("tbdk_hog_resize",), one(lambda: {"img": _hog96()["img"]}),
         single(lambda i: O.hog_resize(i["img"], (61, 97))),
         lambda ctx, st, S, b, o, i: hog_module().resize_exact(
             b["img"], (61, 97), ctx=ctx, stream=S)))
add(Case("hog_gradient", ("tbdk_hog_gradient",), one(lambda: {"img": _hog_gray()}),
         single(lambda i: O.hog_gradient(i["img"], nbins=9)),
         lambda ctx, st, S, b, o, i: hog_module().gradient(
             b["img"], _hog_obj(ctx, (64, 128)), ctx=ctx, stream=S)))


def _hog_blocks_inputs():
    g, q = O.hog_gradient(_hog_gray(), nbins=9)
    return {"grad": g, "qangle": q}


def _hog_blocks_oracle(i):
    from test_gpu_hog import _prm

    return O.hog_blocks(i["grad"], i["qangle"], _prm(_hog_obj(None, (64, 128))))


add(Case("hog_blocks", ("tbdk_hog_blocks",),
         one(_hog_blocks_inputs, lambda: dict(zip(("grad", "qangle"), O.hog_gradient(flip(_hog_gray()), nbins=9)))),
         single(_hog_blocks_oracle),
         lambda ctx, st, S, b, o, i: hog_module().blocks(
             b["grad"], b["qangle"], _hog_obj(ctx, (64, 128)), ctx=ctx, stream=S)))


# ---- mask_circles and the HBM copy ------------------------------------------------------------------------------------

def _circle_inputs():
    pts = np.float32([[24.7, 20.2], [-3, 2], [47, 39], [53.5, 20], [20, -6], [100.9, 60.1], [159, 119]])
    return {"mask": MC.checker(160, 120, 8), "pts": pts, "count": np.int32([6])}


def _circle_decoy():
    r = _circle_inputs()
    return {"mask": np.ascontiguousarray(255 - r["mask"]), "pts": (r["pts"][::-1] + np.float32(9)).astype(np.float32),
            "count": np.int32([2])}


add(Case("mask_circles", ("tbdk_mask_circles_u8",), one(_circle_inputs, _circle_decoy),
         single(lambda i: KO.draw_discs(i["mask"].copy(), i["pts"][:int(i["count"][0])], 5, 0)),
         lambda ctx, st, S, b, o, i: K().mask_circles(b["mask"], b["pts"], 5, 0, count=b["count"], ctx=ctx, stream=S),
         poison=False))  # the mask is the input buffer itself: the decoy goes back over it

add(Case("hbm_copy", ("tbdk_hbm_copy",), one(lambda: {"src": D.small_frame()}), single(lambda i: i["src"]),
         lambda ctx, st, S, b, o, i: K().hbm_copy(o["dst"], b["src"], ctx=ctx, stream=S),
         outs=_u8_out((120, 160))))


# ---- MOG2 -----------------------------------------------------------------------------------------------------------------

MOG2_FRAMES = 6


def _mog2_case(k):
    case = dict(GC.cases()[k])
    case.update(n=MOG2_FRAMES, rates=case["rates"][:MOG2_FRAMES], bg=(MOG2_FRAMES,))
    return case


def _mog2_inputs(k):
    def inputs(which):
        fr = GC.case_frames(GC.cases()[k])
        sel = range(MOG2_FRAMES) if which == "real" else range(20, 20 + MOG2_FRAMES)  # the decoy: later frames
        return [{"frame": np.ascontiguousarray(fr[t])} for t in sel]

    return inputs


def _mog2_oracle(k):
    def f(ins):
        case = _mog2_case(k)
        masks, bgs, m = M2.run_case(case, GC.params(case), [i["frame"] for i in ins])
        out = [{"mask": masks[t]} for t in range(MOG2_FRAMES)]
        out[-1].update(bg=bgs[MOG2_FRAMES], model=m.model())
        return out

    return f


def _mog2_setup(k):
    def setup(ctx):
        from test_gpu_mog2 import subtractor

        return subtractor(_mog2_case(k)["params"], ctx)

    return setup


def _mog2_run(k):
    def run(ctx, m, S, b, o, i):
        case = _mog2_case(k)
        out = {"mask": m.apply(b["frame"], o["mask"], float(case["rates"][i]), stream=S)}
        if i == MOG2_FRAMES - 1:
            out.update(bg=m.getBackgroundImage(stream=S), model=m.model(stream=S))
        return out

    return run


def _mog2_check(g, ref, what):
    same_bits(g["mask"], ref["mask"], f"{what}: mask")
    if "bg" in ref:
        same_bits(g["bg"], ref["bg"], f"{what}: background image")
        for name, x, y in zip(("weight", "variance", "mean", "modes_used"), g["model"], ref["model"]):
            same_bits(x, y, f"{what}: model {name}")


def _mog2_active(k):
    """some mask has background and foreground, and every single frame matters: the first frame's mask does not
    depend on its pixels (every pixel starts a mode), so a frame read too early shows in what is compared later;
    with frame t alone replaced by the decoy's, a later mask or the final model differs"""
    def active(r):
        real, decoy = _mog2_inputs(k)("real"), _mog2_inputs(k)("decoy")
        for t in range(MOG2_FRAMES):
            mixed = _mog2_oracle(k)(real[:t] + [decoy[t]] + real[t + 1:])
            if not differs_any(mixed[t:], r[t:]):
                return False
        return any(0 < (x["mask"] == 0).mean() < 1 for x in r[1:])

    return active


for _k in (0, 19):  # 8UC1 and 32FC3 on the base sequence
    _c = GC.cases()[_k]
    add(Case(f"mog2_{_c['name'].replace(' ', '_')}",
             ("tbdk_mog2_apply", "tbdk_mog2_get_background", "tbdk_mog2_get_model"), _mog2_inputs(_k), _mog2_oracle(_k),
             _mog2_run(_k), _mog2_check, setup=_mog2_setup(_k), active=_mog2_active(_k),
             called=lambda i: ("tbdk_mog2_apply",) + (("tbdk_mog2_get_background", "tbdk_mog2_get_model")
                                                      if i == MOG2_FRAMES - 1 else ()),
             differs=lambda a, b: "bg" not in a or differs_any(a, b),  # per frame: see _mog2_active
             outs=lambda i, c=_c: {"mask": ((c["h"], c["w"]), "uint8")}))


# ---- the KLT tracker ---------------------------------------------------------------------------------------------------------

KLT_CFG = dict(win=9, max_level=2, lk_iters=30, lk_epsilon=0.01, max_corners=40, quality_level=0.05, min_distance=3.0,
               block_size=3, track_len=3, detect_interval=2, mask_radius=3)
KLT_FRAMES = 4  # detection at frames 0 and 2: one detect_interval crossed
KLT_ADD = np.float32([[40.5, 30.25], [100, 60], [12.75, 100.5]])


def _klt_inputs(which):
    seed = 31 if which == "real" else 32
    fr = O.synth(seed, 160, 120, 6, 0, KLT_FRAMES)[0]
    ins = [{"frame": np.ascontiguousarray(fr[t])} for t in range(KLT_FRAMES)]
    ins[0]["pts"] = KLT_ADD if which == "real" else (KLT_ADD[::-1] * np.float32(0.5)).astype(np.float32)
    return ins


def _klt_oracle(ins):
    t = KO.KltTracker(160, 120, **KLT_CFG)
    out = []
    for k, i in enumerate(ins):
        if k == 0:
            t.add_points(i["pts"])
        t.step(i["frame"])
        out.append(t.state())
    return out


def _klt_run(ctx, t, S, b, o, i):
    if i == 0:
        t.add_points(b["pts"], stream=S)
    t.step(b["frame"], stream=S)
    return t.device_state()


def _klt_check(g, ref, what):
    n = int(g[0][0])
    assert n == len(ref[0]), f"{what}: {n} live tracks vs {len(ref[0])}"
    for name, x, y in zip(("ids", "last_pts", "lens", "hist"), g[1:], ref):
        same_bits(x[:n], y, f"{what}: {name}")


add(Case("klt_tracker", ("tbdk_klt_tracker_step", "tbdk_klt_tracker_add_points"), _klt_inputs, _klt_oracle, _klt_run,
         _klt_check, setup=lambda ctx: K().KltTracker(ctx=ctx, width=160, height=120, **KLT_CFG),
         called=lambda i: ("tbdk_klt_tracker_step",) + (("tbdk_klt_tracker_add_points",) if i == 0 else ()),
         active=lambda r: all(len(s[0]) > 3 for s in r) and r[-1][2].max() == 3,
         poison=False))  # the outputs are views of the tracker's state; the frame is overwritten: the step copied it


# ---- cornerSubPix: corners and device counts produced late ------------------------------------------------------------

SUBPIX_CAP = D.GFTT_PRM[0]


def _subpix_inputs():
    img = D.small_frame()
    found = O.gftt_rois(img, D.ROIS, *D.GFTT_PRM)
    corners = np.zeros((len(found), SUBPIX_CAP, 2), np.float32)
    for r, c in enumerate(found):
        corners[r, :len(c)] = c
    return {"img": img, "corners": corners, "counts": np.int32([len(c) for c in found])}


def _subpix_decoy():
    r = _subpix_inputs()
    return {"img": flip(r["img"]), "corners": (r["corners"][::-1] * np.float32(0.75) + np.float32(11.5)).astype(np.float32),
            "counts": np.ascontiguousarray((r["counts"][::-1] // 2 + 1).astype(np.int32))}


def _subpix_oracle(i):
    import _subpix_oracle as SP

    return SP.refine_rows(i["img"], i["corners"], i["counts"], (5, 5))


add(Case("corner_sub_pix", ("tbdk_corner_sub_pix",), one(_subpix_inputs, _subpix_decoy), single(_subpix_oracle),
         lambda ctx, st, S, b, o, i: K().corner_sub_pix(b["img"], b["corners"], (5, 5), counts=b["counts"], ctx=ctx,
                                                        stream=S),
         active=lambda r: (r[0] != _subpix_inputs()["corners"]).any(2).sum() > 10))


# ---- box fit (through the C entry points: the Python wrappers copy the fits to the host) -----------------------------

def _box_inputs(seed):
    def f():
        from test_gpu_box_ransac import make_boxes

        prev, nxt, st, offs, boxes = make_boxes(seed, 6, 40)
        return {"prev": prev, "next": nxt, "status": st.astype(np.uint8), "offsets": offs.astype(np.int32),
                "boxes": np.asarray(boxes, np.int32).reshape(-1, 4)}

    return f


def _box_decoy(seed):
    def f():
        r = _box_inputs(seed)()
        n = len(r["prev"])
        offs = np.int32(np.round(np.linspace(0, n, len(r["offsets"]))))
        return {"prev": np.ascontiguousarray(r["next"][::-1]), "next": np.ascontiguousarray(r["prev"][::-1]),
                "status": np.ascontiguousarray(1 - r["status"]), "offsets": offs,
                "boxes": np.ascontiguousarray(r["boxes"][::-1] + np.int32(3))}

    return f


def _box_sets(i):
    for k, box in enumerate(i["boxes"]):
        sl = slice(int(i["offsets"][k]), int(i["offsets"][k + 1]))
        sel = i["status"][sl] != 0
        yield k, tuple(int(v) for v in box), i["prev"][sl][sel], i["next"][sl][sel]


def _box_oracle(i):
    """per box: (pairs used, getRTMatrix or None, the propagated centre)"""
    from test_gpu_box_fit import BF

    out = []
    for k, box, a, b in _box_sets(i):
        M = BF.get_rt_matrix(a, b) if len(a) >= 2 else None
        out.append((len(a), M, BF.propagate_box(M, box) if M is not None else None))
    return out


def _box_ransac_oracle(i):
    """per box: the restatement's consensus (found, round, inliers among the used pairs, M)"""
    import _rigid_oracle as R

    out = []
    for k, box, a, b in _box_sets(i):
        r = R.estimate(a, b, 500, 0.5)
        out.append((bool(r.found), int(r.k), np.asarray(r.inliers), np.asarray(r.M) if r.found else np.eye(2, 3),
                    (float(r.resid_margin), float(r.collin_margin))))
    return out


def _box_run(ransac):
    def run(ctx, st, S, b, o, i):
        import ctypes as C

        import torch
        from opencv_amd import _lib
        from opencv_amd.klt import BOX_FIT_DTYPE, _stream_ptr

        nb, npts = b["boxes"].shape[0], b["prev"].shape[0]
        out = torch.zeros(nb * BOX_FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        if not ransac:
            _lib.check(ctx.lib.tbdk_box_propagate(ctx.handle, p(b["prev"]), p(b["next"]), p(b["status"]),
                                                  p(b["offsets"]), p(b["boxes"]), nb, 4, p(out), _stream_ptr(S)),
                       "tbdk_box_propagate")
            return (out,)
        par = _lib.RansacParams()
        _lib.check(ctx.lib.tbdk_ransac_default_params(C.byref(par)), "tbdk_ransac_default_params")
        iters = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
        inl = torch.full((npts,), 9, dtype=torch.uint8, device="cuda")
        _lib.check(ctx.lib.tbdk_box_propagate_ransac(ctx.handle, p(b["prev"]), p(b["next"]), p(b["status"]),
                                                     p(b["offsets"]), p(b["boxes"]), nb, 4, C.byref(par), p(out),
                                                     p(iters), p(inl), _stream_ptr(S)), "tbdk_box_propagate_ransac")
        return (out, iters, inl)

    return run


def _box_check(seed):
    """tests/test_gpu_box_fit.py's comparison, box by box"""
    def check(g, ref, what):
        from opencv_amd.klt import BOX_FIT_DTYPE
        from test_gpu_box_fit import BF

        i = _box_inputs(seed)()
        got = np.frombuffer(g[0].tobytes(), BOX_FIT_DTYPE)
        for k, box, a, b in _box_sets(i):
            n, M, centre = ref[k]
            assert got["npoints"][k] == n, f"{what}: box {k} used {got['npoints'][k]} pairs, not {n}"
            if n < 2:
                continue
            scale = np.hypot(M[0, 0], M[1, 0])
            assert bool(got["valid"][k]) == (n >= 4 and 0.5 < scale < 2.0), f"{what}: box {k} valid"
            gm = got["m"][k].reshape(2, 3)
            tol = 64 * np.finfo(np.float64).eps * np.linalg.cond(BF.rt_sums(a, b)[0])
            assert np.all(np.abs(gm - M) <= tol * np.maximum(1.0, np.abs(M))), f"{what}: box {k} matrix"
            assert abs(got["cx"][k] - centre[0]) <= 1e-4 and abs(got["cy"][k] - centre[1]) <= 1e-4, f"{what}: box {k}"

    return check


def _box_ransac_check(seed):
    """tests/test_gpu_box_ransac.py's check (the restatement's margins asserted, then the exact comparison)"""
    def check(g, ref, what):
        from opencv_amd.klt import BOX_FIT_DTYPE
        from test_gpu_box_ransac import check as ransac_check

        i = _box_inputs(seed)()
        fit = np.frombuffer(g[0].tobytes(), BOX_FIT_DTYPE)
        found = ransac_check((fit, g[1], g[2]), i["prev"], i["next"], i["status"], i["offsets"],
                             [tuple(int(v) for v in bx) for bx in i["boxes"]], 4)
        assert found == sum(r[0] for r in ref), what

    return check


def _box_differs(a, b):
    return a[0] != b[0] or differs_any(a[1:], b[1:])


add(Case("box_propagate", ("tbdk_box_propagate",), one(_box_inputs(5), _box_decoy(5)),
         lambda ins: [_box_oracle(ins[0])], _box_run(False), _box_check(5),
         differs=lambda a, b: any(_box_differs(x, y) for x, y in zip(a, b)),
         active=lambda r: sum(n >= 4 for n, _, _ in r[0]) >= 3))
add(Case("box_propagate_ransac", ("tbdk_box_propagate_ransac",), one(_box_inputs(5), _box_decoy(5)),
         lambda ins: [_box_ransac_oracle(ins[0])], _box_run(True), _box_ransac_check(5),
         differs=lambda a, b: any(_box_differs(x, y) for x, y in zip(a, b)),
         # the precondition of test_gpu_box_ransac.py's exact comparison: no residual near the threshold
         active=lambda r: sum(x[0] for x in r[0]) >= 2 and all(x[4][0] >= 1e-4 and x[4][1] >= 1e-9 for x in r[0])))


# ---- the point-set estimators: two sets in one launch, offsets and status produced late --------------------------------

def _sets_inputs(points, truth_a, truth_b, seed):
    def real():
        sa, da = points("plane", 65, 20, truth_a, seed)
        sb, db = points("plane", 64, 10, truth_b, seed + 1)
        st = np.ones(129, np.uint8)
        st[3::7] = 0
        return {"src": np.concatenate([sa, sb]), "dst": np.concatenate([da, db]), "status": st,
                "offsets": np.int32([0, 65, 129])}

    def decoy():
        r = real()
        st = np.ones(129, np.uint8)
        st[::3] = 0
        return {"src": np.ascontiguousarray(r["dst"][::-1]), "dst": np.ascontiguousarray(r["src"][::-1] + np.float32(2)),
                "status": st, "offsets": np.int32([0, 40, 129])}

    return one(real, decoy)


def _sets_of(i):
    for k in range(len(i["offsets"]) - 1):
        sl = slice(int(i["offsets"][k]), int(i["offsets"][k + 1]))
        sel = i["status"][sl] != 0
        yield sl, sel, np.ascontiguousarray(i["src"][sl][sel]), np.ascontiguousarray(i["dst"][sl][sel])


def _estimator_oracle(estimate, matrix):
    """per set: (valid, npoints, ninliers, iters), the mask over all its pairs, the matrix before the LM step"""
    def f(i):
        out = []
        for sl, sel, s, d in _sets_of(i):
            r = estimate(s, d)
            mask = np.zeros(len(sel), np.uint8)
            mask[sel] = r.mask
            out.append(((int(r.valid), len(s), int(r.ninliers), int(r.iters)), mask,
                        np.asarray(getattr(r, matrix), np.float64)))
        return out

    return single(f)


def _estimator_check(ndoubles):
    """contract A of tests/test_gpu_affine2d.py and tests/test_gpu_homography.py (refinement off): valid, npoints,
    ninliers, iters, the whole mask and the matrix, bit for bit"""
    def check(g, ref, what):
        raw, mask = g
        size = 8 * ndoubles + 16
        off = 0
        for k, (fields, want_mask, M) in enumerate(ref):
            rec = np.ascontiguousarray(raw[k * size:(k + 1) * size])
            got = tuple(int(v) for v in rec[8 * ndoubles:].view(np.int32)[[3, 0, 1, 2]])  # valid, npoints, ninliers, iters
            assert got == fields, f"{what}: set {k}: (valid, npoints, ninliers, iters) {got} vs {fields}"
            same_bits(mask[off:off + len(want_mask)], want_mask, f"{what}: set {k} mask")
            same_bits(rec[:8 * ndoubles].view(np.float64), M.ravel(), f"{what}: set {k} matrix", nan_any=True)
            off += len(want_mask)

    return check


def _affine_case(name, model, method):
    import _affine2d_cases as AC
    import _affine2d_oracle as AO

    def run(ctx, st, S, b, o, i):
        fn = K().estimate_affine_2d if model == AC.FULL else K().estimate_affine_partial_2d
        r = fn(b["src"], b["dst"], method=method, refineIters=0, status=b["status"], offsets=b["offsets"], ctx=ctx,
               stream=S)
        return r.raw, r.mask

    add(Case(name, ("tbdk_estimate_affine_2d",), _sets_inputs(AC.points, "shear", "similarity", 77),
             _estimator_oracle(lambda s, d: AO.estimate(s, d, model, method, refine_iters=0), "M0"), run,
             _estimator_check(6), active=lambda r: all(f[0] == 1 and 3 < f[2] < f[1] for f, _, _ in r[0])))


def _homography_case(name, method):
    import _homography_cases as HC
    import _homography_oracle as HO

    def run(ctx, st, S, b, o, i):
        r = K().find_homography(b["src"], b["dst"], method=method, status=b["status"], offsets=b["offsets"],
                                refine=False, ctx=ctx, stream=S)
        return r.raw, r.mask

    add(Case(name, ("tbdk_find_homography",), _sets_inputs(HC.points, "mild", "mild", 78),
             _estimator_oracle(lambda s, d: HO.find_homography(s, d, method, refine=False), "H0"), run,
             _estimator_check(9),
             active=lambda r: all(f[0] == 1 and 4 < f[2] <= f[1] for f, _, _ in r[0])))


_affine_case("estimate_affine_2d_ransac", 0, 8)
_affine_case("estimate_affine_2d_lmeds", 0, 4)
_affine_case("estimate_affine_partial_2d_ransac", 1, 8)
_affine_case("estimate_affine_partial_2d_lmeds", 1, 4)
_homography_case("find_homography_all_pairs", 0)
_homography_case("find_homography_ransac", 8)


# ---- warps ---------------------------------------------------------------------------------------------------------------

import _remap_cases as PC  # noqa: E402
import _remap_oracle as RO  # noqa: E402

WARP_SRC, WARP_DST = (130, 121), (130, 33)  # (width, height): tests/_remap_cases.py's largest source and destination
_a = np.deg2rad(0.8)
WARP_M = np.array([[1.01 * np.cos(_a), -1.01 * np.sin(_a), 2.5], [1.01 * np.sin(_a), 1.01 * np.cos(_a), -1.75]])


def _warp_src(cn=1):
    return PC.image(*WARP_SRC, cn, "8u", 41)


def _warp_out(cn=1):
    return lambda i: {"dst": ((WARP_DST[1], WARP_DST[0]) + ((cn,) if cn > 1 else ()), "uint8")}


def _zeros(cn=1):
    return np.zeros((WARP_DST[1], WARP_DST[0]) + ((cn,) if cn > 1 else ()), np.uint8)


add(Case("warp_affine_host_matrix", ("tbdk_warp_affine_u8",), one(lambda: {"src": _warp_src()}),
         single(lambda i: O.warp_affine(i["src"], WARP_M, WARP_DST, O.INTER_LINEAR, O.BORDER_REFLECT_101)),
         lambda ctx, st, S, b, o, i: K().warp_affine(b["src"], WARP_M, WARP_DST, K().INTER_LINEAR,
                                                     K().BORDER_REFLECT_101, dst=o["dst"], ctx=ctx, stream=S),
         outs=_warp_out()))
add(Case("remap", ("tbdk_remap",),
         one(lambda: {"src": _warp_src(3), "map": PC.float_map("smooth", *WARP_SRC, *WARP_DST, 3)},
             lambda: {"src": flip(_warp_src(3)), "map": PC.float_map("noise", *WARP_SRC, *WARP_DST, 4)}),
         single(lambda i: RO.remap(i["src"], _zeros(3), i["map"], None, RO.MAP_32FC2, RO.INTER_LINEAR,
                                   RO.BORDER_REFLECT_101)),
         lambda ctx, st, S, b, o, i: K().remap(b["src"], b["map"], None, RO.INTER_LINEAR, RO.BORDER_REFLECT_101,
                                               dst=o["dst"], ctx=ctx, stream=S), outs=_warp_out(3)))


def _flow(seed):
    return ((PC._unit(*WARP_DST, seed) - 0.5) * 12).astype(np.float32)


add(Case("remap_flow", ("tbdk_remap_flow",),
         one(lambda: {"src": _warp_src(3)[:WARP_DST[1]].copy(), "flow": _flow(170)},
             lambda: {"src": flip(_warp_src(3)[:WARP_DST[1]]), "flow": -_flow(171)}),
         single(lambda i: RO.remap_flow(i["src"], _zeros(3), i["flow"], 1, RO.INTER_LINEAR, RO.BORDER_REFLECT_101)),
         lambda ctx, st, S, b, o, i: K().remap_flow(b["src"], b["flow"], 1, RO.INTER_LINEAR, RO.BORDER_REFLECT_101,
                                                    dst=o["dst"], ctx=ctx, stream=S), outs=_warp_out(3)))
WARP_H = PC.matrix("mild", *WARP_SRC, *WARP_DST)
add(Case("warp_perspective_host_matrix", ("tbdk_warp_perspective",), one(lambda: {"src": _warp_src(3)}),
         single(lambda i: RO.warp_perspective(i["src"], _zeros(3), WARP_H, RO.INTER_LINEAR, RO.BORDER_REFLECT_101)),
         lambda ctx, st, S, b, o, i: K().warp_perspective(b["src"], WARP_H, WARP_DST, RO.INTER_LINEAR,
                                                          RO.BORDER_REFLECT_101, dst=o["dst"], ctx=ctx, stream=S),
         outs=_warp_out(3)))


def _dev_matrix_inputs(points, truth, seed):
    def real():
        s, d = points("plane", 65, 10, truth, seed)
        return {"src": _warp_src(), "from": s, "to": d, "offsets": np.int32([0, 65])}

    def decoy():
        r = real()
        return {"src": flip(r["src"]), "from": np.ascontiguousarray(r["to"][::-1]),
                "to": np.ascontiguousarray(r["from"][::-1] * np.float32(0.5)), "offsets": np.int32([0, 30])}

    return one(real, decoy)


def _warp_by_affine_oracle(i):
    import _affine2d_oracle as AO

    n = int(i["offsets"][1])
    r = AO.estimate(i["from"][:n], i["to"][:n], 0, 8, refine_iters=0)
    M = np.asarray(r.M0, np.float64).reshape(2, 3)
    return {"valid": int(r.valid), "M": M,
            "dst": O.warp_affine(i["src"], M, WARP_DST, O.INTER_LINEAR, O.BORDER_REFLECT_101)}


def _warp_by_affine_run(ctx, st, S, b, o, i):
    k = K()
    r = k.estimate_affine_2d(b["from"], b["to"], refineIters=0, offsets=b["offsets"], ctx=ctx, stream=S)
    out = k.warp_affine(b["src"], r.M[0], WARP_DST, k.INTER_LINEAR, k.BORDER_REFLECT_101, dst=o["dst"], ctx=ctx,
                        stream=S, valid=r.valid[0:1])  # no synchronisation in between
    return {"valid": r.valid[0:1], "M": r.M[0], "dst": out}


def _warp_by_homography_oracle(i):
    import _homography_oracle as HO

    n = int(i["offsets"][1])
    r = HO.find_homography(i["from"][:n], i["to"][:n], 8, refine=False)
    H = np.asarray(r.H0, np.float64).reshape(3, 3)
    return {"valid": int(r.valid), "M": H,
            "dst": RO.warp_perspective(i["src"], _zeros(), H, RO.INTER_LINEAR, RO.BORDER_REFLECT_101)}


def _warp_by_homography_run(ctx, st, S, b, o, i):
    k = K()
    r = k.find_homography(b["from"], b["to"], refine=False, offsets=b["offsets"], ctx=ctx, stream=S)
    out = k.warp_perspective(b["src"], r.H[0], WARP_DST, RO.INTER_LINEAR, RO.BORDER_REFLECT_101, dst=o["dst"], ctx=ctx,
                             stream=S, valid=r.valid[0:1])  # no synchronisation in between
    return {"valid": r.valid[0:1], "M": r.H[0], "dst": out}


def _dev_matrix_check(g, ref, what):
    """the matrix is the estimator's, bit for bit (its contract A), and the image is the warp by it"""
    assert int(g["valid"][0]) == ref["valid"] == 1, f"{what}: valid"
    same_bits(g["M"], ref["M"], f"{what}: the matrix the warp read")
    same_bits(g["dst"], ref["dst"], f"{what}: the warped image")


def _dev_matrix_cases():
    import _affine2d_cases as AC
    import _homography_cases as HC

    add(Case("warp_affine_device_matrix", ("tbdk_warp_affine_u8_dev", "tbdk_estimate_affine_2d"),
             _dev_matrix_inputs(AC.points, "shear", 77), single(_warp_by_affine_oracle), _warp_by_affine_run,
             _dev_matrix_check, differs=lambda a, b: differs_any(a["dst"], b["dst"]),
             active=lambda r: r[0]["valid"] == 1 and r[0]["dst"].any(), outs=_warp_out()))
    add(Case("warp_perspective_device_matrix", ("tbdk_warp_perspective_dev", "tbdk_find_homography"),
             _dev_matrix_inputs(HC.points, "mild", 78), single(_warp_by_homography_oracle), _warp_by_homography_run,
             _dev_matrix_check, differs=lambda a, b: differs_any(a["dst"], b["dst"]),
             active=lambda r: r[0]["valid"] == 1 and r[0]["dst"].any(), outs=_warp_out()))


_dev_matrix_cases()


# ---- the TBD loop: every frame produced late, and next_frame as well --------------------------------------------------

import _loop_pair as LP  # noqa: E402

# tests/_loop_pair.py's smallest case (160x120, 6 objects, window 21), cut to the shortest sequence on which the
# oracle predicts, refreshes point sets and tracks points (LP.check_oracle_activity's rule; _loop_active below)
LW, LH, LN, LF, LSEED, LDROP = 160, 120, 6, 5, 31, 0.1
LCFG = {"bounds_xmax": LW, "bounds_ymax": LH, "win": 21, "max_level": 3, "redetect_every": 2}
SUBPIX_WIN = 10  # tests/test_gpu_tbd_subpix.py's


def _loop_frames(which):
    return LP.L.O.synth(LSEED if which == "real" else LSEED + 1, LW, LH, LN, 0, LF)[0]


def _loop_dets():
    """the oracle's and the library's detections of the real sequence (host inputs: never late)"""
    from opencv_amd import tbd

    _, ogt, keep = LP.sequence(LSEED, LW, LH, LN, LF, LDROP)
    gpu = []
    for f in range(LF):
        d = tbd.detections_from_gt(ogt[f])
        gpu.append(np.ascontiguousarray(d[keep[f][d["id"]]]))
    return [LP.L.detections(ogt[f], f, keep[f]) for f in range(LF)], gpu


def _loop_inputs(how):
    def inputs(which):
        fr = [np.ascontiguousarray(x) for x in _loop_frames(which)]
        if how == "run":
            return [{f"f{k}": x for k, x in enumerate(fr)}]
        if how == "step":
            return [{"frame": x} for x in fr]
        # ahead: the next frame arrives late with step f and is step f + 1's frame, in the same buffer
        return [dict(([("frame", fr[0])] if f == 0 else []) + ([("next", fr[f + 1])] if f + 1 < LF else []))
                for f in range(LF)]

    return inputs


def _frames_of(ins):
    if "f0" in ins[0]:
        return [ins[0][f"f{k}"] for k in range(LF)]
    if "next" in ins[0]:
        return [ins[0]["frame"]] + [i["next"] for i in ins if "next" in i]
    return [i["frame"] for i in ins]


def _loop_oracle(how, fb=0, ransac=0, subpix=0):
    def f(ins):
        import _subpix_oracle as SO

        L = LP.L
        kw = dict(nthreads=1 if subpix else min(16, LP.os.cpu_count() or 1), **LP.oracle_kwargs(LCFG))
        saved_bf, saved_gftt = L.BF, L.O.gftt_rois
        try:
            if ransac:
                from test_gpu_tbd_ransac import RansacFitShim

                L.BF = RansacFitShim
            if subpix:
                L.O.gftt_rois = lambda frame, rois, max_corners=256, quality=0.01, min_distance=3.0: \
                    SO.gftt_rois_subpix(frame, rois, max_corners, quality, min_distance, win=(subpix, subpix))
            if fb:
                import _fb_oracle as FB

                ora = FB.FbKltTbdLoop(LW, LH, fb_thr=fb / 1024.0, **kw)
            else:
                ora = L.KltTbdLoop(LW, LH, **kw)
            dets, out = _loop_dets()[0], []
            for k, frame in enumerate(_frames_of(ins)):
                m = dict(ora.step(frame, k, dets[k]))
                out.append((m, dict(ora.preds), tuple(ora.track_rows())))
        finally:
            L.BF, L.O.gftt_rois = saved_bf, saved_gftt
        return [([o[0] for o in out], out[-1][1], out[-1][2])] if how == "run" else out

    return f


def _loop_setup(fb=0, ransac=0, subpix=0):
    def setup(ctx):
        from opencv_amd import tbd

        opts = {"tbd_fb_check": fb, "tbd_fit_ransac": ransac, "tbd_subpix": subpix}
        try:  # taken by tbdk_tbd_create; the shared context goes back to its defaults
            for k, v in opts.items():
                ctx.set_option(k, v)
            loop = tbd.TbdLoop(tbd.default_config(LW, LH, **LCFG), ctx=ctx)
        finally:
            for k in opts:
                ctx.set_option(k, 0)
        return {"loop": loop, "dets": _loop_dets()[1], "carry": None}

    return setup


def _loop_run(how):
    def run(ctx, st, S, b, o, i):
        loop, dets = st["loop"], st["dets"]
        if how == "run":
            ms = loop.run([b[f"f{k}"] for k in range(LF)], 0, dets, stream=S)
            return ([LP.gpu_metrics(m) for m in ms], loop.predictions(), LP.gpu_rows(loop.tracks()))
        frame = b["frame"] if "frame" in b else st["carry"]
        m = loop.step(frame, i, dets[i], stream=S, next_frame=b.get("next"))
        st["carry"] = b.get("next")
        return (LP.gpu_metrics(m), loop.predictions(), LP.gpu_rows(loop.tracks()))

    return run


def _loop_check(g, ref, what):
    """tests/_loop_pair.py run_pair's comparison of one frame"""
    gm, gp, rows = g
    om, op, orows = ref
    assert gm == om, f"{what}: metrics {gm} vs oracle {om}"
    assert gp.keys() == op.keys(), f"{what}: predicted tracks differ"
    for k, (cx, cy) in gp.items():
        assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= LP.PRED_TOL, f"{what}: track {k} centre"
    assert [tuple(r) for r in rows] == [tuple(r) for r in orows], f"{what}: tracks differ"


def _loop_active(how):
    def active(r):
        ms = r[0][0] if how == "run" else [x[0] for x in r]
        return (sum(m["klt_predicted"] for m in ms) > 0 and sum(m["redetected"] for m in ms) > 0 and
                sum(m["lk_points"] for m in ms) > 0)

    return active


for _name, _how, _opt, _syms in (
        ("tbd_step", "step", {}, ("tbdk_tbd_step",)),
        ("tbd_step_ahead", "ahead", {}, ("tbdk_tbd_step_ahead", "tbdk_tbd_step")),
        ("tbd_run", "run", {}, ("tbdk_tbd_run",)),
        ("tbd_step_ahead_fb_check", "ahead", {"fb": 1024}, ("tbdk_tbd_step_ahead", "tbdk_tbd_step")),
        ("tbd_step_fit_ransac", "step", {"ransac": 500}, ("tbdk_tbd_step",)),
        ("tbd_step_ahead_subpix", "ahead", {"subpix": SUBPIX_WIN}, ("tbdk_tbd_step_ahead", "tbdk_tbd_step"))):
    add(Case(_name, _syms, _loop_inputs(_how), _loop_oracle(_how, **_opt), _loop_run(_how), _loop_check,
             differs=lambda a, b: a != b, active=_loop_active(_how), setup=_loop_setup(**_opt),
             sync={"step": SYNC_STEP, "ahead": SYNC_STEP_AHEAD, "run": SYNC_RUN}[_how],
             keep={"next": KEEP_NEXT} if _how == "ahead" else {}))


def _image_frames(which):
    import test_gpu_tbd_detect as TD

    fr = TD.bgr_frames((320, 240))[:3]
    return [{"frame": x if which == "real" else flip(x)} for x in fr]


def _image_oracle(ins):
    """tests/test_gpu_tbd_detect.py's oracle_front and oracle_run over the given frames (confidence mode 1)"""
    import test_gpu_tbd_detect as TD

    L, T_ = TD.L, TD.T
    prm, svm = O.hog_params(win=(48, 96)), TD.svm48()
    ora = L.KltTbdLoop(TD.W, TD.H, bounds=TD.BOUNDS, nthreads=min(16, LP.os.cpu_count() or 1),
                       track_confidence_threshold=-1.0)
    out = []
    for f, i in enumerate(ins):
        gray = FE.cvt_resize_gray(i["frame"], FE.COLOR_BGR2GRAY, (TD.W, TD.H))
        r, w = O.hog_detect_multiscale(np.ascontiguousarray(gray), prm, svm, hit_threshold=TD.HIT, nlevels=TD.NLEVELS,
                                       scale0=TD.SCALE0, group_threshold=TD.GROUP)
        dets = [T_.Detection(-1, f, T_.Rect(*(int(v) for v in rr)), float(w[k])) for k, rr in enumerate(r)]
        m = dict(ora.step(np.ascontiguousarray(gray), f, dets))
        out.append((r.copy(), w.copy(), m, dict(ora.preds), ora.track_rows()))
    return out


def _image_setup(ctx):
    import test_gpu_tbd_detect as TD

    loop = TD.gpu_loop(ctx, -1.0)
    loop.attach_detector(TD.gpu_hog(ctx), src_size=(320, 240), make_gray=True, confidence_mode=1)
    return loop


def _image_run(ctx, loop, S, b, o, i):
    import test_gpu_tbd_detect as TD

    m, dets = loop.step_image(b["frame"], i, stream=S)
    return (dets, TD.metrics_of(m), loop.predictions(), TD.gpu_rows(loop.tracks()))


def _image_check(g, ref, what):
    dets, gm, gp, rows = g
    rects, wts, om, op, orows = ref
    got = np.stack([dets["x"], dets["y"], dets["width"], dets["height"]], 1) if len(dets) else np.zeros((0, 4))
    assert np.array_equal(got, rects), f"{what}: rects differ"
    assert np.array_equal(dets["confidence"], wts), f"{what}: confidences differ"
    assert gm == om, f"{what}: metrics {gm} vs oracle {om}"
    assert gp.keys() == op.keys(), f"{what}: predicted tracks differ"
    for k, (cx, cy) in gp.items():
        assert max(abs(cx - op[k][0]), abs(cy - op[k][1])) <= 1e-4, f"{what}: track {k}"
    assert rows == orows, f"{what}: tracks differ"


add(Case("tbd_step_image", ("tbdk_tbd_step_image",), _image_frames, _image_oracle, _image_run, _image_check,
         differs=lambda a, b: differs_any(a[:2], b[:2]) or a[2:] != b[2:],
         active=lambda r: all(len(x[0]) >= 8 for x in r) and len(r[-1][4]) > 0 and r[-1][2]["klt_predicted"] > 0,
         setup=_image_setup, sync=SYNC_STEP_IMAGE))


# ---- pairs: two different calls of one entry point behind one spin ---------------------------------------------------

PAIRS = [("gftt_lds", "gftt_one_larger_roi"), ("gftt_table_in_memory", "gftt_one_larger_roi"),
         ("resize_linear_31x20", "resize_linear_150x99"), ("cvt_resize_gray_31x20", "cvt_resize_gray_150x99"),
         ("hog_detect_multiscale_lanes3", "hog_detect_multiscale_320x240_48x96"),
         ("farneback_box_ahead1", "farneback_320x240_gauss"), ("farneback_box_ahead0", "farneback_320x240_gauss"),
         ("dense_lk_case_images_7", "dense_lk_160x120_13"), ("dense_lk_per_pixel_9x7", "dense_lk_160x120_13"),
         ("mog2_8UC1_history_12", "mog2_32FC3_frac")]


# ---- stream-taking symbols without a case ----------------------------------------------------------------------------------

EXCLUDED = {
    "tbdk_synth_render": "a test-input generator with no device input, so nothing can be produced late; its frames "
                         "are compared with the oracle's wherever a test renders them (tests/_loop_pair.py "
                         "gpu_inputs, tests/test_gpu_klt.py)",
    "tbdk_tbd_run_host": "its frames are host memory: there is no device input to produce late; its results are "
                         "compared with tbdk_tbd_run's in tests/test_gpu_tbd.py and tests/test_gpu_tbd_fb.py",
}

BY_NAME = {c.name: c for c in CASES}
# the cases of several calls on one object, none of which synchronises: their frames are also queued behind one spin
SEQUENCES = [c.name for c in CASES if c.sync is None and c.called is not None]

