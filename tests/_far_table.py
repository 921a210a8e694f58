"""The case table of tests/test_gpu_far_views.py: every pitch-taking entry point of
include/tbdk.h with one of its images (or every image that shares that pitch
parameter) placed in the far arena of tests/_far.py, the others ordinary tensors.

A case names the case of tests/_streams_table.py whose input generator, oracle
and comparison it reuses (those of the entry point's own test_gpu_* file, bit for
bit), or builds such a case here (`local`); `far` names the inputs and
caller-owned outputs that go into the arena; `covers` the (symbol, pitch
parameter) pairs of the header that this puts far.  Where the Python wrapper
allocates an output itself or passes a packed pitch, `run` calls the C entry
point with the far view.

A `bound` case reads the caller's image through a buffer descriptor; it cites the
header line that states the bound, and under a layout beyond it runs twice: at the
largest accepted pitch the results equal the oracle, at the smallest rejected one
the call returns TBDK_EINVAL with every output and the arena untouched.

tests/test_far_cases.py holds, from this table and the header alone, that every
pitch parameter has its case, that the layouts' arithmetic is as claimed, and that
the rectangles of a case keep apart."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

import _far as F
import _frontend_oracle as FE
import _gftt_f32_oracle as O32
import _gftt_mask_oracle as MO
import _oracle as O
import _streams_table as T
import test_blobs_streams  # noqa: F401  (registers the morphology and labelling cases with the streams table)
import test_gpu_dirty_state as D
from test_gpu_extreme import same_bits

K = T.K
LIMIT = (1 << 32) - 1


@dataclass(frozen=True)
class Bound:
    cite: str     # the header line that states it
    kind: str     # "span": (h - 1) * pitch + row <= 2^32 - 1; "pitch_height": pitch * h <= 2^32 - 1

    def accepts(self, h, pitch, row):
        return (F.extent(h, pitch, row) if self.kind == "span" else pitch * h) <= LIMIT

    def last_accepted(self, h, row, unit):
        p = (LIMIT - row) // (h - 1) if self.kind == "span" else LIMIT // h
        return p - p % unit


ROI_SPAN = Bound("tbdk.h, image layout: \"each ROI's rows may span at most 4294967295 bytes\"", "span")
MASK_SPAN = Bound("tbdk.h, image layout: \"(height - 1) * mask_pitch + width at most 4294967295\"", "span")
MAP_SPAN = Bound("tbdk.h, image layout: \"(height - 1) * pitch + width * pixel bytes at most 4294967295\"", "span")
BORROWED = Bound("tbdk.h, image layout: \"tbdk_pyr_build_borrowed: pitch * height at most 4294967295\"", "pitch_height")
RUN = Bound("tbdk.h, image layout: \"tbdk_tbd_run: pitch * height at most 4294967295\"", "pitch_height")


@dataclass
class FarCase:
    name: str
    base: object                    # a _streams_table.Case: inputs, oracle, setup, comparison (and run unless `run`)
    far: tuple                      # names of inputs / caller-owned outputs placed in the arena
    covers: tuple                   # ((symbol, pitch parameter), ...)
    run: object = None              # (ctx, state, bufs, outs, i) -> outputs; None: the base's run
    outs: object = None             # (i) -> {name: (shape, dtype name)}; None: the base's
    units: dict = field(default_factory=dict)   # pixel bytes of two-value planes (pitch and pointer alignment)
    share: dict = field(default_factory=dict)   # {name: group}: images under one pitch parameter
    bound: Bound = None
    options: dict = field(default_factory=dict)
    hold: tuple = ()                # far inputs the library reads until the case ends (others the base keeps: one more call)

    def outs_of(self, i):
        f = self.outs or self.base.outs
        return dict(f(i)) if f else {}

    def images(self, i):
        """[(name, shape, numpy dtype, unit)] of the far images of call i"""
        inp, outs, res = self.base.inputs("real")[i], self.outs_of(i), []
        for n in self.far:
            if n in inp:
                shape, dt = inp[n].shape, inp[n].dtype
            elif n in outs:
                shape, dt = tuple(outs[n][0]), np.dtype(outs[n][1])
            else:
                continue
            res.append((n, tuple(shape), np.dtype(dt), self.units.get(n, np.dtype(dt).itemsize)))
        return res

    def ncalls(self):
        return len(self.base.inputs("real"))


CASES = []


def add(name, base, far, covers, **kw):
    base = T.BY_NAME[base] if isinstance(base, str) else base
    assert name not in [c.name for c in CASES], name
    covers = tuple((covers,) if isinstance(covers[0], str) else covers)
    CASES.append(FarCase(name, base, tuple(far), covers, **kw))


def ptr(t):
    return C.c_void_p(t.data_ptr())


def pitch(t):
    return int(t.stride(0)) * t.element_size()


def stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(status, what):
    from opencv_amd import _lib

    _lib.check(status, what)


def local(name, symbols, inputs, oracle, run, check=T.check_bits, **kw):
    """a case of the streams table's kind that lives here only"""
    return T.Case(name, symbols, inputs, oracle, run, check, **kw)


# ---- pyramids -----------------------------------------------------------------------------------------------------------

for _kind, _sym in (("u8", "tbdk_pyr_build"), ("levels", "tbdk_pyr_build"), ("cn3", "tbdk_pyr_build"),
                    ("f16_u8", "tbdk_pyr_build"), ("f16_f16", "tbdk_pyr_build_f16"), ("f32_u16", "tbdk_pyr_build_u16"),
                    ("f32_f32", "tbdk_pyr_build_f32")):
    add(f"pyramid_{_kind}", f"pyramid_{_kind}", ("img",), (_sym, "pitch"))
add("pyramid_borrowed", "pyramid_borrowed", ("img",), ("tbdk_pyr_build_borrowed", "pitch"), bound=BORROWED)

add("pyr_down_src", "pyr_down", ("img",), ("tbdk_pyr_down_u8", "src_pitch"))


def _pyr_down_dst(ctx, st, b, o, i):
    h, w = b["img"].shape
    ok(ctx.lib.tbdk_pyr_down_u8(ctx.handle, ptr(b["img"]), w, h, pitch(b["img"]), ptr(o["dst"]), pitch(o["dst"]), stream()),
       "tbdk_pyr_down_u8")
    return o["dst"]


add("pyr_down_dst", "pyr_down", ("dst",), ("tbdk_pyr_down_u8", "dst_pitch"), run=_pyr_down_dst,
    outs=lambda i: {"dst": ((60, 80), "uint8")})


# ---- PyrLK on a level 0 borrowed from the caller (tbdk_pyr_build_borrowed, then tbdk_lk_sparse / _fb) ----------------

def _borrowed_setup(ctx):
    import torch

    k = K()
    pyr = [k.Pyramid(ctx, D.PW, D.PH, T.LK_ML, T.LK_WIN, torch.uint8, derivs=False) for _ in range(2)]
    return pyr, k.SparsePyrLKOpticalFlow(T.LK_WIN, T.LK_ML, 30)


def _borrowed_run(kind):
    def run(ctx, st, S, b, o, i):
        (Pa, Pb), lk = st
        Pa.build_borrowed(b["a"], stream=S)
        Pb.build_borrowed(b["b"], stream=S)
        if kind == "fb":
            r = lk.calc_checked(Pa, Pb, b["pts"], back_threshold=1.0, want_iters=True, stream=S)
            return {"next_pts": r.next_pts, "status": r.status, "err": r.err, "iters": r.iters,
                    "back_pts": r.back_pts, "fb_err": r.fb_err}
        r = lk.calc(Pa, Pb, b["pts"], None, want_iters=True, stream=S)
        return (r.next_pts, r.status, r.err, r.iters)

    return run


for _kind, _sym in (("plain", "tbdk_lk_sparse"), ("fb", "tbdk_lk_sparse_fb")):
    _base = local(f"lk_borrowed_{_kind}", (_sym, "tbdk_pyr_build_borrowed"), T._lk_inputs(_kind), T._lk_oracle(_kind),
                  _borrowed_run(_kind), T._lk_check(_kind), setup=_borrowed_setup, active=T._lk_status(_kind))
    for _far in (("a",), ("b",), ("a", "b")):
        add(f"lk_borrowed_{_kind}_{'_'.join(_far)}", _base, _far, ("tbdk_pyr_build_borrowed", "pitch"), bound=BORROWED)


# ---- dense PyrLK: the flow and status planes -------------------------------------------------------------------------------

def _dense_run(ctx, st, b, o, i):
    import torch

    (Pa, Pb), lk = st
    Pa.build(b["a"])
    Pb.build(b["b"])
    h, w = b["a"].shape
    flow = o.get("flow", torch.empty((h, w, 2), dtype=torch.float32, device="cuda"))
    status = o.get("status", torch.empty((h, w), dtype=torch.uint8, device="cuda"))
    prm = lk.params()
    ok(ctx.lib.tbdk_lk_dense(ctx.handle, C.byref(Pa.pyr), C.byref(Pb.pyr), ptr(flow), pitch(flow), ptr(status),
                             pitch(status), C.byref(prm), stream()), "tbdk_lk_dense")
    return flow, status


add("dense_lk_flow", "dense_lk_case_images_7", ("flow",), ("tbdk_lk_dense", "flow_pitch"), run=_dense_run,
    outs=lambda i: {"flow": ((D.DH, D.DW, 2), "float32")}, units={"flow": 8})
add("dense_lk_status", "dense_lk_per_pixel_9x7", ("status",), ("tbdk_lk_dense", "status_pitch"), run=_dense_run,
    outs=lambda i: {"status": ((D.DH, D.DW), "uint8")})


# ---- GFTT: a whole-frame ROI (spans the boundary), a ROI wholly beyond it, a ROI wholly below it ------------------------

GW, GH = 160, 120
GFTT_ROIS = {"whole": [(0, 0, GW, GH)], "beyond": [(20, GH - F.EDGE_ROWS, 120, F.EDGE_ROWS)], "below": [(20, 15, 77, 51)]}


def gftt_mask():
    """4 x 4 blocks of 0 and 255 from hashed noise, about half set: no two rows 8 or more apart agree, so mask rows
    read 2^31 or 2^32 bytes low (whole pitches lower, a few bytes aside) cannot pass for the right ones, as the
    periodic checker of the other mask tests would"""
    b = FE.pattern(GW // 4, GH // 4, 1, 4712).reshape(GH // 4, GW // 4)
    return np.ascontiguousarray(np.kron(np.where(b < 128, 255, 0).astype(np.uint8), np.ones((4, 4), np.uint8)))


def _gftt_img(depth):
    return D.small_frame() if depth == "8u" else T._typed(depth)


def _gftt_oracle(depth, masked, rois):
    def f(i):
        if depth != "8u":
            return O32.gftt_rois(i["img"], i.get("mask"), rois, *D.GFTT_PRM, 3, False, 0.04)
        if masked:
            return MO.gftt_rois_masked(i["img"], i["mask"], rois, *D.GFTT_PRM)
        return O.gftt_rois(i["img"], rois, *D.GFTT_PRM, 3, False, 0.04)

    return T.single(f)


for _roi, _rois in GFTT_ROIS.items():
    for _depth, _masked, _sym in (("8u", False, "tbdk_gftt_rois"), ("8u", True, "tbdk_gftt_rois_masked"),
                                  ("16u", False, "tbdk_gftt_rois_px"), ("32f", True, "tbdk_gftt_rois_px")):
        _ins = (lambda d=_depth, m=_masked: dict({"img": _gftt_img(d)}, **({"mask": gftt_mask()} if m else {})))
        _base = local(f"gftt_{_depth}{'_masked' if _masked else ''}_{_roi}", (_sym,), T.one(_ins),
                      _gftt_oracle(_depth, _masked, _rois), T._gftt_run(D.GFTT_PRM, _rois), T._gftt_check,
                      differs=T._lists_differ, active=T._corners)
        _b = ROI_SPAN if _roi == "whole" else None
        add(f"{_base.name}_img", _base, ("img",), (_sym, "pitch"), bound=_b)
        if _masked:
            add(f"{_base.name}_mask", _base, ("mask",), (_sym, "mask_pitch"), bound=_b)


# ---- the corner response maps ---------------------------------------------------------------------------------------------

def _corner_dst(block, harris, min_eig=False):
    def run(ctx, st, b, o, i):
        from opencv_amd import klt

        img, dst = b["img"], o["dst"]
        h, w = img.shape
        pix = klt._PIX[img.dtype]
        if min_eig:
            ok(ctx.lib.tbdk_corner_min_eig_val(ctx.handle, ptr(img), w, h, pitch(img), ptr(dst), pitch(dst), stream()),
               "tbdk_corner_min_eig_val")
        elif img.element_size() == 1:
            ok(ctx.lib.tbdk_corner_response(ctx.handle, ptr(img), w, h, pitch(img), ptr(dst), pitch(dst), block,
                                            int(harris), 0.04, stream()), "tbdk_corner_response")
        else:
            ok(ctx.lib.tbdk_corner_response_px(ctx.handle, ptr(img), pix, w, h, pitch(img), ptr(dst), pitch(dst), block,
                                               int(harris), 0.04, stream()), "tbdk_corner_response_px")
        return dst

    return run


_MAP_OUT = lambda i: {"dst": ((GH, GW), "float32")}  # noqa: E731
for _name, _sym, _run in (("corner_min_eigen_val", "tbdk_corner_min_eig_val", _corner_dst(3, False, True)),
                          ("corner_response_harris5", "tbdk_corner_response", _corner_dst(5, True)),
                          ("corner_response_px_32f", "tbdk_corner_response_px", _corner_dst(5, True)),
                          ("corner_response_px_16u", "tbdk_corner_response_px", _corner_dst(5, True))):
    add(f"{_name}_src", _name, ("img",), (_sym, "pitch"), bound=MAP_SPAN if _name == "corner_min_eigen_val" else None)
    add(f"{_name}_dst", _name, ("dst",), (_sym, "dst_pitch"), run=_run, outs=_MAP_OUT)

# block size 3 without Harris is the minimum-eigenvalue walk (the descriptor kernel) through the other two symbols too
for _depth, _sym in (("8u", "tbdk_corner_response"), ("32f", "tbdk_corner_response_px")):
    _base = local(f"corner_response_block3_{_depth}", (_sym,), T.one(lambda d=_depth: {"img": _gftt_img(d)}),
                  T.single((lambda i: O.min_eig(i["img"])) if _depth == "8u" else (lambda i: T._resp32(i["img"], 3, False))),
                  lambda ctx, st, S, b, o, i: K().corner_response(b["img"], 3, False, 0.04, ctx=ctx, stream=S))
    add(f"{_base.name}_src", _base, ("img",), (_sym, "pitch"), bound=MAP_SPAN)

add("corner_sub_pix_img", "corner_sub_pix", ("img",), ("tbdk_corner_sub_pix", "pitch"))


# ---- warps ---------------------------------------------------------------------------------------------------------------

for _name, _sym in (("warp_affine_host_matrix", "tbdk_warp_affine_u8"), ("warp_affine_device_matrix", "tbdk_warp_affine_u8_dev"),
                    ("warp_perspective_host_matrix", "tbdk_warp_perspective"),
                    ("warp_perspective_device_matrix", "tbdk_warp_perspective_dev"), ("remap", "tbdk_remap"),
                    ("remap_flow", "tbdk_remap_flow")):
    add(f"{_name}_src", _name, ("src",), (_sym, "src_pitch"))
    add(f"{_name}_dst", _name, ("dst",), (_sym, "dst_pitch"))
add("remap_map1", "remap", ("map",), ("tbdk_remap", "map1_pitch"), units={"map": 8})
add("remap_flow_flow", "remap_flow", ("flow",), ("tbdk_remap_flow", "flow_pitch"), units={"flow": 8})

_REMAP_PAIR = local(
    "remap_32fc1_pair", ("tbdk_remap",),
    T.one(lambda: {"src": T._warp_src(3), "mapx": np.ascontiguousarray(T.PC.float_map("smooth", *T.WARP_SRC, *T.WARP_DST, 3)[..., 0]),
                   "mapy": np.ascontiguousarray(T.PC.float_map("smooth", *T.WARP_SRC, *T.WARP_DST, 3)[..., 1])}),
    T.single(lambda i: T.RO.remap(i["src"], T._zeros(3), i["mapx"], i["mapy"], T.RO.MAP_32FC1, T.RO.INTER_LINEAR,
                                  T.RO.BORDER_REFLECT_101)),
    lambda ctx, st, S, b, o, i: K().remap(b["src"], b["mapx"], b["mapy"], T.RO.INTER_LINEAR, T.RO.BORDER_REFLECT_101,
                                          dst=o["dst"], ctx=ctx, stream=S), outs=T._warp_out(3))
add("remap_pair_map1", _REMAP_PAIR, ("mapx",), ("tbdk_remap", "map1_pitch"))
add("remap_pair_map2", _REMAP_PAIR, ("mapy",), ("tbdk_remap", "map2_pitch"))


# ---- the front end ------------------------------------------------------------------------------------------------------------

for _name, _sym in (("cvt_color_BGR2GRAY", "tbdk_cvt_color_u8"), ("cvt_color_BGR2BGRA", "tbdk_cvt_color_u8"),
                    ("resize_linear_150x99", "tbdk_resize_linear_u8"), ("cvt_resize_gray_150x99", "tbdk_cvt_resize_gray_u8")):
    add(f"{_name}_src", _name, ("src",), (_sym, "src_pitch"))
    add(f"{_name}_dst", _name, ("dst",), (_sym, "dst_pitch"))


# ---- Farneback ------------------------------------------------------------------------------------------------------------------

add("farneback_frames", "farneback_box_ahead1", ("a", "b"), ("tbdk_farneback", "pitch"), share={"a": "f", "b": "f"})
add("farneback_frames_no_prep_ahead", "farneback_box_ahead0", ("a", "b"), ("tbdk_farneback", "pitch"),
    share={"a": "f", "b": "f"}, options={"fb_prep_ahead": 0})


def _fb_flow(ctx, st, b, o, i):
    from opencv_amd import farneback as FB

    fb = FB.FarnebackOpticalFlow.create(ctx=ctx, numLevels=3, numIters=2, flags=0)
    h, w = b["a"].shape
    ok(ctx.lib.tbdk_farneback(ctx.handle, ptr(b["a"]), ptr(b["b"]), w, h, pitch(b["a"]), ptr(o["flow"]), pitch(o["flow"]),
                              C.byref(fb.p), stream()), "tbdk_farneback")
    return o["flow"]


add("farneback_flow", "farneback_box_ahead1", ("flow",), ("tbdk_farneback", "flow_pitch"), run=_fb_flow, units={"flow": 8})

FB_LEVEL = (49, 33)  # a destination of at least 32 rows (the streams case's has 20)


def _fb_level(ctx, st, S, b, o, i):
    img = b["img"]
    h, w = img.shape
    ok(ctx.lib.tbdk_fb_level_image(ctx.handle, ptr(img), w, h, pitch(img), FB_LEVEL[0], FB_LEVEL[1], 9, 1.5, ptr(o["dst"]),
                                   pitch(o["dst"]), stream()), "tbdk_fb_level_image")
    return o["dst"]


_FB_LEVEL = local("fb_level_image_49x33", ("tbdk_fb_level_image",), T.one(lambda: {"img": FE.pattern(*T.FB_STAGE, 1, 77)}),
                  T.single(lambda i: O.fb_level_image(i["img"], FB_LEVEL, 9, 1.5)), _fb_level,
                  outs=lambda i: {"dst": ((FB_LEVEL[1], FB_LEVEL[0]), "float32")})
add("fb_level_image_src", _FB_LEVEL, ("img",), ("tbdk_fb_level_image", "pitch"))
add("fb_level_image_dst", _FB_LEVEL, ("dst",), ("tbdk_fb_level_image", "dst_pitch"))

PW_, PH_ = T.FB_STAGE  # 97 x 61


def _poly_exp(ctx, st, S, b, o, i):
    src = b["lvl"]
    ok(ctx.lib.tbdk_fb_poly_exp(ctx.handle, ptr(src), PW_, PH_, pitch(src), 5, 1.1, ptr(o["dst"]), pitch(o["dst"]), stream()),
       "tbdk_fb_poly_exp")
    return o["dst"].reshape(5, PH_, PW_).permute(1, 2, 0) if o["dst"].is_contiguous() else o["dst"]


def _poly_check(g, ref, what):
    g = np.asarray(g)
    if g.shape == (5 * PH_, PW_):  # the five planes, stacked dst_pitch * height apart, as the far view holds them
        g = g.reshape(5, PH_, PW_).transpose(1, 2, 0)
    same_bits(g, ref[0] if isinstance(ref, (list, tuple)) else ref, f"{what}: polynomial expansion")


_POLY = local("fb_poly_exp_planes", ("tbdk_fb_poly_exp",), T.one(lambda: {"lvl": FE.pattern(PW_, PH_, 1, 77).astype(np.float32)}),
              T.single(lambda i: O.fb_poly_exp(i["lvl"], 5, 1.1)), _poly_exp, _poly_check,
              outs=lambda i: {"dst": ((5 * PH_, PW_), "float32")})
add("fb_poly_exp_src", _POLY, ("lvl",), ("tbdk_fb_poly_exp", "src_pitch"))
add("fb_poly_exp_dst", _POLY, ("dst",), ("tbdk_fb_poly_exp", "dst_pitch"))


# ---- HOG ----------------------------------------------------------------------------------------------------------------------------

add("hog_detect_multiscale_img", "hog_detect_multiscale_lanes3", ("img",), ("tbdk_hog_detect_multiscale", "pitch"),
    options={"hog_level_streams": 3})
add("hog_detect_multiscale_one_lane_img", "hog_detect_multiscale_lanes1", ("img",), ("tbdk_hog_detect_multiscale", "pitch"),
    options={"hog_level_streams": 1})
add("hog_detect_img", "hog_detect", ("img",), ("tbdk_hog_detect", "pitch"))
add("hog_resize_src", "hog_resize", ("img",), ("tbdk_hog_resize", "pitch"))
add("hog_gradient_img", "hog_gradient", ("img",), ("tbdk_hog_gradient", "pitch"))


def _hog_resize_dst(ctx, st, b, o, i):
    img = b["img"]
    h, w, cn = img.shape
    ok(ctx.lib.tbdk_hog_resize(ctx.handle, ptr(img), w, h, pitch(img), cn, ptr(o["dst"]), 61, 97, pitch(o["dst"]), stream()),
       "tbdk_hog_resize")
    return o["dst"]


add("hog_resize_dst", "hog_resize", ("dst",), ("tbdk_hog_resize", "dst_pitch"), run=_hog_resize_dst,
    outs=lambda i: {"dst": ((97, 61, 3), "uint8")})

HOG_W, HOG_H = 151, 97  # _streams_table._hog_gray


def _hog_gradient(ctx, st, b, o, i):
    import torch

    img = b["img"]
    hg = T._hog_obj(ctx, (64, 128))
    grad = o.get("grad", torch.empty((HOG_H, HOG_W, 2), dtype=torch.float32, device="cuda"))
    qa = o.get("qangle", torch.empty((HOG_H, HOG_W, 2), dtype=torch.uint8, device="cuda"))
    ok(ctx.lib.tbdk_hog_gradient(ctx.handle, ptr(img), HOG_W, HOG_H, pitch(img), 1, C.byref(hg.p), ptr(grad), pitch(grad),
                                 ptr(qa), pitch(qa), stream()), "tbdk_hog_gradient")
    return grad, qa


add("hog_gradient_grad", "hog_gradient", ("grad",), ("tbdk_hog_gradient", "grad_pitch"), run=_hog_gradient,
    outs=lambda i: {"grad": ((HOG_H, HOG_W, 2), "float32")}, units={"grad": 8})
add("hog_gradient_qangle", "hog_gradient", ("qangle",), ("tbdk_hog_gradient", "qangle_pitch"), run=_hog_gradient,
    outs=lambda i: {"qangle": ((HOG_H, HOG_W, 2), "uint8")}, units={"qangle": 2})


def _hog_blocks(ctx, st, b, o, i):
    import torch

    hg = T._hog_obj(ctx, (64, 128))
    p = hg.p
    csx, csy = np.gcd(p.win_stride_x, p.block_stride_x), np.gcd(p.win_stride_y, p.block_stride_y)
    nbx, nby = (HOG_W - p.block_w) // csx + 1, (HOG_H - p.block_h) // csy + 1
    out = torch.empty((nby, nbx, hg.getBlockHistogramSize()), dtype=torch.float32, device="cuda")
    ok(ctx.lib.tbdk_hog_blocks(ctx.handle, ptr(b["grad"]), pitch(b["grad"]), ptr(b["qangle"]), pitch(b["qangle"]), HOG_W,
                               HOG_H, C.byref(p), ptr(out), stream()), "tbdk_hog_blocks")
    return out


add("hog_blocks_grad", "hog_blocks", ("grad",), ("tbdk_hog_blocks", "grad_pitch"), run=_hog_blocks, units={"grad": 8})
add("hog_blocks_qangle", "hog_blocks", ("qangle",), ("tbdk_hog_blocks", "qangle_pitch"), run=_hog_blocks,
    units={"qangle": 2})


# ---- mask_circles, MOG2, morphology, labelling ------------------------------------------------------------------------------------

add("mask_circles_mask", "mask_circles", ("mask",), ("tbdk_mask_circles_u8", "pitch"))

for _c in ("mog2_8UC1_history_12", "mog2_32FC3_frac"):
    add(f"{_c}_frame", _c, ("frame",), ("tbdk_mog2_apply", "pitch"))
    add(f"{_c}_mask", _c, ("mask",), ("tbdk_mog2_apply", "mask_pitch"))


def _mog2_bg(k):
    def run(ctx, m, b, o, i):
        case = T._mog2_case(k)
        out = {"mask": m.apply(b["frame"], o["mask"], float(case["rates"][i]))}
        if i == T.MOG2_FRAMES - 1:
            out.update(bg=m.getBackgroundImage(o["bg"]), model=m.model())
        return out

    return run


def _mog2_outs(k):
    c = T.GC.cases()[k]
    shape = (c["h"], c["w"]) + ((3,) if c["cn"] == 3 else ())
    dt = "uint8" if c["content"] == "u8" else "float32"

    def outs(i):
        o = {"mask": ((c["h"], c["w"]), "uint8")}
        if i == T.MOG2_FRAMES - 1:
            o["bg"] = (shape, dt)
        return o

    return outs


for _k, _c in ((0, "mog2_8UC1_history_12"), (19, "mog2_32FC3_frac")):
    add(f"{_c}_background", _c, ("bg",), ("tbdk_mog2_get_background", "pitch"), run=_mog2_bg(_k), outs=_mog2_outs(_k))

add("morph_src", "morph_open_130x121", ("src",), ("tbdk_morph_u8", "src_pitch"))
add("morph_dst", "morph_open_130x121", ("dst",), ("tbdk_morph_u8", "dst_pitch"))


def _morph_in_place(ctx, st, b, o, i):
    from opencv_amd import imgproc

    return imgproc.morphology_ex(b["src"], test_blobs_streams.MPO.OPEN, test_blobs_streams.BC.elements()["ellipse5x5"],
                                 dst=b["src"], ctx=ctx)


add("morph_in_place", "morph_open_130x121", ("src",), (("tbdk_morph_u8", "src_pitch"), ("tbdk_morph_u8", "dst_pitch")),
    run=_morph_in_place)
add("connected_components_img", "connected_components_130x121", ("src",), ("tbdk_connected_components", "pitch"))
add("connected_components_labels", "connected_components_130x121", ("labels",),
    ("tbdk_connected_components", "labels_pitch"))


# ---- the KLT tracker and the TBD loop ---------------------------------------------------------------------------------------------------

add("klt_tracker_frames", "klt_tracker", ("frame",), ("tbdk_klt_tracker_step", "pitch"))
add("tbd_step_frames", "tbd_step", ("frame",), ("tbdk_tbd_step", "pitch"))
add("tbd_step_ahead_frames", "tbd_step_ahead", ("frame", "next"),
    (("tbdk_tbd_step_ahead", "pitch"), ("tbdk_tbd_step_ahead", "next_pitch")), share={"frame": "f", "next": "f"})
_RUN_FRAMES = tuple(f"f{k}" for k in range(T.LF))
add("tbd_run_frames", "tbd_run", _RUN_FRAMES, ("tbdk_tbd_run", "pitch"), share={n: "f" for n in _RUN_FRAMES}, bound=RUN)
add("tbd_run_frames_borrowed_l0", "tbd_run", _RUN_FRAMES, ("tbdk_tbd_run", "pitch"), share={n: "f" for n in _RUN_FRAMES},
    bound=RUN, options={"tbd_borrow_l0": 1})
add("tbd_step_image_frames", "tbd_step_image", ("frame",), ("tbdk_tbd_step_image", "pitch"))


def loop_mask():
    """byte 1 everywhere except x < 60 or y >= LH - 20"""
    m = np.ones((T.LH, T.LW), np.uint8)
    m[:, :60] = 0
    m[T.LH - 20:, :] = 0
    return m


def _masked_loop_inputs(which):
    ins = T._loop_inputs("step")(which)
    ins[0] = dict(ins[0], mask=loop_mask() if which == "real" else np.ascontiguousarray(1 - loop_mask()))
    return ins


def _masked_loop_oracle(ins):
    L = T.LP.L
    mask, saved = ins[0]["mask"], L.O.gftt_rois
    try:
        L.O.gftt_rois = lambda frame, rois, max_corners=256, quality=0.01, min_distance=3.0: \
            MO.gftt_rois_masked(frame, mask, rois, max_corners, quality, min_distance)
        ora = L.KltTbdLoop(T.LW, T.LH, nthreads=1, **T.LP.oracle_kwargs(T.LCFG))
        dets, out = T._loop_dets()[0], []
        for k, i in enumerate(ins):
            m = dict(ora.step(i["frame"], k, dets[k]))
            out.append((m, dict(ora.preds), tuple(ora.track_rows())))
    finally:
        L.O.gftt_rois = saved
    return out


def _masked_loop_run(ctx, st, S, b, o, i):
    if i == 0:
        st["loop"].set_corner_mask(b["mask"])
    return T._loop_run("step")(ctx, st, S, b, o, i)


KEEP_MASK = "tbdk.h, tbdk_tbd_set_corner_mask: \"which the caller keeps alive and\""
_MASKED_LOOP = local("tbd_step_under_mask", ("tbdk_tbd_set_corner_mask", "tbdk_tbd_step"), _masked_loop_inputs,
                     _masked_loop_oracle, _masked_loop_run, T._loop_check, differs=lambda a, b: a != b,
                     active=T._loop_active("step"), setup=T._loop_setup(), sync=T.SYNC_STEP, keep={"mask": KEEP_MASK})
add("tbd_corner_mask", _MASKED_LOOP, ("mask",), ("tbdk_tbd_set_corner_mask", "mask_pitch"), bound=MASK_SPAN,
    hold=("mask",))


# ---- the synthetic renderer: two frames, stacked height * pitch apart -------------------------------------------------------------------

SYNTH = (20261020, 160, 120, 6, 2)  # seed, width, height, objects, frames


def _synth_run(ctx, st, S, b, o, i):
    import torch

    seed, w, h, nobj, nf = SYNTH
    gt = torch.zeros((nf, nobj, 5), dtype=torch.int32)
    ok(ctx.lib.tbdk_synth_render(ctx.handle, seed, w, h, nobj, 0, nf, ptr(o["out"]), pitch(o["out"]), ptr(gt), stream()),
       "tbdk_synth_render")
    return o["out"]


_SYNTH = local("synth_render_two_frames", ("tbdk_synth_render",), lambda which: [{}],
               lambda ins: [np.concatenate(list(O.synth(*SYNTH[:4], 0, SYNTH[4])[0]))], _synth_run,
               outs=lambda i: {"out": ((SYNTH[4] * SYNTH[2], SYNTH[1]), "uint8")})
add("synth_render_out", _SYNTH, ("out",), ("tbdk_synth_render", "pitch"))


# ---- pitch parameters without a case ------------------------------------------------------------------------------------------------------

EXCLUDED = {
    ("tbdk_pyr_download", "host_pitch"): "tbdk.h, tbdk_pyr_download: \"Synchronous copy of level `level` to host memory\": "
                                         "the pitch is that of host memory",
    ("tbdk_pyr_download_deriv", "host_pitch"): "tbdk.h, tbdk_pyr_download_deriv: \"host_pitch in bytes\": host memory",
    ("tbdk_tbd_run_host", "pitch"): "tbdk.h, tbdk_tbd_run_host: \"frames = host pointers (same pitch\": the frames are host "
                                    "memory, which the arena cannot hold; the uploads are hipMemcpy2DAsync with size_t pitches",
}

BY_NAME = {c.name: c for c in CASES}
OPTION_DEFAULTS = dict(D.DEFAULTS, tbd_borrow_l0=0)
