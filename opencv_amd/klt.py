"""Host-side mirror of the reference's KLT operator interfaces over libtbdk.

Device memory is plain torch tensors on a HIP device (plumbing only; every
computation runs in the HIP kernels of libtbdk.so).  The classes keep the
shape of the reference's CUDA interfaces:

  * SparsePyrLKOpticalFlow  <- cv::cuda::SparsePyrLKOpticalFlow
        (modules/cudaoptflow/include/opencv2/cudaoptflow.hpp:160-180)
  * Pyramid / build_pyramid <- cv::buildOpticalFlowPyramid
        (modules/video/src/lkpyramid.cpp:697-793)
  * pyr_down                <- cv::cuda::pyrDown
        (modules/cudawarping/include/opencv2/cudawarping.hpp:201)

Argument meaning and error behaviour follow the reference: `calc` accepts
images or prebuilt pyramids, empty point sets return empty outputs
(pyrlk.cpp:221-227), invalid arguments raise (CV_Assert -> TbdkError).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

_ctx_cache: dict[int, "Context"] = {}


def _stream_ptr(stream) -> C.c_void_p:
    if stream is None:
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


class Context:
    """One tbdk_ctx per HIP device (the C ABI allows one per thread x device)."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.tbdk_ctx_create(int(device), C.byref(h)), "tbdk_ctx_create")
        self.handle = h
        self.device = int(device)

    def __del__(self):
        self.close()

    def close(self) -> None:
        """tbdk_ctx_destroy; every object made from the context must be gone by then."""
        h = getattr(self, "handle", None)
        if h and h.value:
            try:
                self.lib.tbdk_ctx_destroy(h)
            except Exception:
                pass
            self.handle = None

    @staticmethod
    def get(device: int = 0) -> "Context":
        c = _ctx_cache.get(device)
        if c is None:
            c = Context(device)
            _ctx_cache[device] = c
        return c

    def timing_enable(self, on: bool = True) -> None:
        _lib.check(self.lib.tbdk_timing_enable(self.handle, int(bool(on))), "tbdk_timing_enable")

    def set_option(self, name: str, value: int) -> None:
        """tbdk_ctx_set_option (see include/tbdk.h)."""
        _lib.check(self.lib.tbdk_ctx_set_option(self.handle, name.encode(), int(value)), "tbdk_ctx_set_option")

    def debug_fill_scratch(self, byte: int) -> int:
        """tbdk_ctx_debug_fill_scratch (a test aid, see include/tbdk.h): every device
        buffer the context owns filled with `byte`, every cache forgotten; the bytes filled."""
        n = C.c_int64()
        _lib.check(self.lib.tbdk_ctx_debug_fill_scratch(self.handle, int(byte), C.byref(n)),
                   "tbdk_ctx_debug_fill_scratch")
        return int(n.value)

    def timing_select(self, names=None) -> None:
        """Record only these kernels (iterable of names; None = all)."""
        arg = ",".join(names).encode() if names else None
        _lib.check(self.lib.tbdk_timing_select(self.handle, arg), "tbdk_timing_select")

    def timing_calls(self, name: str) -> int:
        """Selected launches of `name` since timing_enable, timed or not (ctx option timing_every)."""
        n = C.c_int64()
        _lib.check(self.lib.tbdk_timing_calls(self.handle, name.encode(), C.byref(n)), "tbdk_timing_calls")
        return int(n.value)

    def timing_query(self, name: str) -> tuple[int, float]:
        n = C.c_int64()
        ms = C.c_double()
        _lib.check(self.lib.tbdk_timing_query(self.handle, name.encode(), C.byref(n), C.byref(ms)),
                   "tbdk_timing_query")
        return int(n.value), float(ms.value)


DEPTH_8U, DEPTH_16F = 0, 7  # TBDK_DEPTH_* (cv::Mat depth codes; 7 = OpenCV 4's CV_16F)


class Pyramid:
    """A padded pyramid in device memory (tbdk_pyr): u8 levels with int16 Scharr
    planes, or (dtype=torch.float16) the fp16 pixel path's fp16 levels with fp16
    (Ix, Iy) planes, or (dtype=torch.float32) the fp32 pixel path (16U / 32F
    frames) with fp32 levels and planes."""

    def __init__(self, ctx: Context, width: int, height: int, max_level: int = 3, win=(21, 21),
                 dtype: torch.dtype = torch.uint8, derivs: bool = True, channels: int = 1):
        """derivs=False (u8 only): levels without derivative planes
        (tbdk_pyr_create_levels); PyrLK then derives the window's Scharr values
        itself, with the same results.  channels 2..4: interleaved multi-channel
        frames, u8 (tbdk_pyr_create_cn) or the fp32 pixel path for 16U / 32F
        frames (tbdk_pyr_create_f32_cn)."""
        if dtype not in (torch.uint8, torch.float16, torch.float32):
            raise _lib.TbdkError("Pyramid dtype must be torch.uint8, torch.float16 or torch.float32")
        if not derivs and dtype != torch.uint8:
            raise _lib.TbdkError("levels-only pyramids are u8")
        if channels != 1 and (dtype == torch.float16 or not derivs):
            raise _lib.TbdkError("multi-channel pyramids are u8 or fp32, with derivative planes")
        self.ctx = ctx
        self.dtype = dtype
        self.channels = int(channels)
        self.pyr = _lib.Pyr()
        if channels != 1 and dtype == torch.float32:
            _lib.check(ctx.lib.tbdk_pyr_create_f32_cn(ctx.handle, int(width), int(height), int(channels),
                                                      int(max_level), int(win[0]), int(win[1]), C.byref(self.pyr)),
                       "tbdk_pyr_create_f32_cn")
        elif channels != 1:
            _lib.check(ctx.lib.tbdk_pyr_create_cn(ctx.handle, int(width), int(height), int(channels), int(max_level),
                                                  int(win[0]), int(win[1]), C.byref(self.pyr)), "tbdk_pyr_create_cn")
        else:
            create = ctx.lib.tbdk_pyr_create_f16 if dtype == torch.float16 else \
                ctx.lib.tbdk_pyr_create_f32 if dtype == torch.float32 else \
                ctx.lib.tbdk_pyr_create if derivs else ctx.lib.tbdk_pyr_create_levels
            _lib.check(create(ctx.handle, int(width), int(height), int(max_level), int(win[0]), int(win[1]),
                              C.byref(self.pyr)), "tbdk_pyr_create")
        self.width, self.height = int(width), int(height)

    @property
    def nlevels(self) -> int:
        return int(self.pyr.nlevels)

    def build(self, img: torch.Tensor, stream=None) -> "Pyramid":
        """From a 2-D uint8 frame (either depth) or, for an fp16 pyramid, a float16 frame;
        a multi-channel pyramid from an (H, W, C) uint8 frame (fp32 multi-channel
        pyramids also uint16 / float32)."""
        if self.channels != 1:
            ok_types = (torch.uint8, torch.uint16, torch.float32) if self.dtype == torch.float32 else (torch.uint8,)
            if img.dim() != 3 or not img.is_cuda or img.dtype not in ok_types or \
                    tuple(img.shape) != (self.height, self.width, self.channels) or img.stride(2) != 1 or \
                    img.stride(1) != self.channels:
                raise _lib.TbdkError("Pyramid.build expects an (H, W, C) device tensor of the pyramid's size and "
                                     "depth")
            fn = {torch.uint8: self.ctx.lib.tbdk_pyr_build, torch.uint16: self.ctx.lib.tbdk_pyr_build_u16,
                  torch.float32: self.ctx.lib.tbdk_pyr_build_f32}[img.dtype]
            _lib.check(fn(self.ctx.handle, C.c_void_p(img.data_ptr()), int(img.stride(0)) * img.element_size(),
                          C.byref(self.pyr), _stream_ptr(stream)), "tbdk_pyr_build (multi-channel)")
            return self
        if self.dtype == torch.float32 and img.dim() == 2 and img.is_cuda and img.stride(1) == 1 and \
                img.dtype in (torch.uint16, torch.float32):
            if img.shape[0] != self.height or img.shape[1] != self.width:
                raise _lib.TbdkError("image size does not match the pyramid")
            fn = self.ctx.lib.tbdk_pyr_build_u16 if img.dtype == torch.uint16 else self.ctx.lib.tbdk_pyr_build_f32
            _lib.check(fn(self.ctx.handle, C.c_void_p(img.data_ptr()), int(img.stride(0)) * img.element_size(),
                          C.byref(self.pyr), _stream_ptr(stream)), "tbdk_pyr_build (fp32 path)")
            return self
        if img.dim() != 2 or not img.is_cuda or not (img.dtype == torch.uint8 or
                                                     (img.dtype == torch.float16 and self.dtype == torch.float16)):
            raise _lib.TbdkError("Pyramid.build expects a 2-D uint8 (or, fp16 pyramid, float16) device tensor")
        if img.shape[0] != self.height or img.shape[1] != self.width or img.stride(1) != 1:
            raise _lib.TbdkError("image size / layout does not match the pyramid")
        if img.dtype == torch.float16:
            _lib.check(self.ctx.lib.tbdk_pyr_build_f16(self.ctx.handle, C.c_void_p(img.data_ptr()),
                                                       int(img.stride(0)) * 2, C.byref(self.pyr),
                                                       _stream_ptr(stream)), "tbdk_pyr_build_f16")
        else:
            _lib.check(self.ctx.lib.tbdk_pyr_build(self.ctx.handle, C.c_void_p(img.data_ptr()), int(img.stride(0)),
                                                   C.byref(self.pyr), _stream_ptr(stream)), "tbdk_pyr_build")
        return self

    def build_borrowed(self, img: torch.Tensor, stream=None) -> "Pyramid":
        """Levels-only u8 pyramid whose level 0 is `img` itself (no padded copy;
        tbdk_pyr_build_borrowed, the reference GPU class's pyramid,
        cudaoptflow/src/pyrlk.cpp:144-145).  `img` must stay alive and unchanged
        while the pyramid is read; the pyramid keeps a reference to it."""
        if self.dtype != torch.uint8 or self.channels != 1:
            raise _lib.TbdkError("borrowed level 0: u8 single-channel levels-only pyramids")
        if img.dim() != 2 or not img.is_cuda or img.dtype != torch.uint8 or img.shape[0] != self.height or \
                img.shape[1] != self.width or img.stride(1) != 1:
            raise _lib.TbdkError("Pyramid.build_borrowed expects a 2-D uint8 device tensor of the pyramid's size")
        _lib.check(self.ctx.lib.tbdk_pyr_build_borrowed(self.ctx.handle, C.c_void_p(img.data_ptr()),
                                                        int(img.stride(0)), C.byref(self.pyr), _stream_ptr(stream)),
                   "tbdk_pyr_build_borrowed")
        self._borrowed = img
        return self

    def level(self, i: int, with_border: bool = False):
        """Host copy of level i as a (H, W) numpy array, uint8 or float16 (test / download helper)."""
        import numpy as np
        L = self.pyr.lv[i]
        h = L.height + (2 * L.pad if with_border else 0)
        w = L.width + (2 * L.pad if with_border else 0)
        dt = {torch.float16: np.float16, torch.float32: np.float32}.get(self.dtype, np.uint8)
        out = np.empty((h, w) if self.channels == 1 else (h, w, self.channels), dtype=dt)
        _lib.check(self.ctx.lib.tbdk_pyr_download(self.ctx.handle, C.byref(self.pyr), int(i),
                                                  out.ctypes.data_as(C.c_void_p), out.strides[0],
                                                  int(bool(with_border))),
                   "tbdk_pyr_download")
        return out

    def deriv(self, i: int):
        """Host copy of the Scharr derivative plane of level i: (H, W, 2) (Ix, Iy), int16
        (or float16 for an fp16 pyramid)."""
        import numpy as np
        L = self.pyr.dv[i]
        out = np.empty((L.height, L.width, 2 * self.channels),
                       dtype={torch.float16: np.float16, torch.float32: np.float32}.get(self.dtype, np.int16))
        _lib.check(self.ctx.lib.tbdk_pyr_download_deriv(self.ctx.handle, C.byref(self.pyr), int(i),
                                                        out.ctypes.data_as(C.c_void_p), out.strides[0]),
                   "tbdk_pyr_download_deriv")
        return out

    def __del__(self):
        if getattr(self, "pyr", None) is not None and self.pyr.storage:
            try:
                self.ctx.lib.tbdk_pyr_destroy(self.ctx.handle, C.byref(self.pyr))
            except Exception:
                pass


def build_pyramid(img: torch.Tensor, win=(21, 21), max_level: int = 3, ctx: Context | None = None,
                  stream=None, dtype: torch.dtype | None = None, derivs: bool = True) -> Pyramid:
    """cv::buildOpticalFlowPyramid (withDerivatives = derivs); dtype
    torch.float16 (or a float16 frame) selects the fp16 pixel path, torch.float32
    (or a uint16 / float32 frame) the fp32 pixel path; an (H, W, C) uint8 frame
    (C = 2..4, interleaved) a multi-channel pyramid."""
    ctx = ctx or Context.get(img.device.index or 0)
    dtype = dtype or (torch.float16 if img.dtype == torch.float16 else
                      torch.float32 if img.dtype in (torch.uint16, torch.float32) else torch.uint8)
    cn = int(img.shape[2]) if img.dim() == 3 else 1
    return Pyramid(ctx, img.shape[1], img.shape[0], max_level, win, dtype, derivs, channels=cn).build(img, stream)


def pyr_down(src: torch.Tensor, ctx: Context | None = None, stream=None) -> torch.Tensor:
    """cv::cuda::pyrDown for CV_8UC1: ((w+1)/2, (h+1)/2), bit-exact with the CPU pyrDown."""
    if src.dtype != torch.uint8 or src.dim() != 2 or not src.is_cuda or src.stride(1) != 1:
        raise _lib.TbdkError("pyr_down expects a 2-D uint8 device tensor")
    ctx = ctx or Context.get(src.device.index or 0)
    h, w = src.shape
    dst = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.uint8, device=src.device)
    _lib.check(ctx.lib.tbdk_pyr_down_u8(ctx.handle, C.c_void_p(src.data_ptr()), w, h, src.stride(0),
                                        C.c_void_p(dst.data_ptr()), dst.stride(0), _stream_ptr(stream)),
               "tbdk_pyr_down_u8")
    return dst


_PIX = {torch.uint8: _lib.TBDK_PIX_U8, torch.uint16: _lib.TBDK_PIX_U16, torch.float32: _lib.TBDK_PIX_F32}


def _corner_image(img: torch.Tensor, what: str) -> tuple[int, int]:
    """(pix, row pitch in bytes) of a GFTT / corner-map source: a 2-D uint8,
    uint16 or float32 device tensor with stride(1) == 1 (any row stride; the
    library checks pointer and pitch against the pixel's alignment)"""
    if not isinstance(img, torch.Tensor) or img.dtype not in _PIX or img.dim() != 2 or not img.is_cuda or \
            img.stride(1) != 1:
        raise _lib.TbdkError(f"{what} expects a 2-D uint8, uint16 or float32 device tensor")
    return _PIX[img.dtype], img.stride(0) * img.element_size()


def corner_min_eigen_val(src: torch.Tensor, ctx: Context | None = None, stream=None) -> torch.Tensor:
    """cv::cuda::createMinEigenValCorner(CV_8UC1 / CV_32FC1, 3, 3)->compute: float32 (h, w)
    minimum-eigenvalue map, bit-exact with the CPU cornerMinEigenVal.  A uint16
    source gives the float32 result of the same values."""
    if isinstance(src, torch.Tensor) and src.dtype != torch.uint8:
        return corner_response(src, 3, False, ctx=ctx, stream=stream)
    if src.dtype != torch.uint8 or src.dim() != 2 or not src.is_cuda or src.stride(1) != 1:
        raise _lib.TbdkError("corner_min_eigen_val expects a 2-D uint8, uint16 or float32 device tensor")
    ctx = ctx or Context.get(src.device.index or 0)
    h, w = src.shape
    dst = torch.empty((h, w), dtype=torch.float32, device=src.device)
    _lib.check(ctx.lib.tbdk_corner_min_eig_val(ctx.handle, C.c_void_p(src.data_ptr()), w, h, src.stride(0),
                                               C.c_void_p(dst.data_ptr()), dst.stride(0) * 4, _stream_ptr(stream)),
               "tbdk_corner_min_eig_val")
    return dst


def corner_response(src: torch.Tensor, block_size: int = 3, harris: bool = False, k: float = 0.04,
                    ctx: Context | None = None, stream=None) -> torch.Tensor:
    """cv::cuda::createMinEigenValCorner(srcType, blockSize, 3) / createHarrisCorner(srcType,
    blockSize, 3, k) ->compute (cudaimgproc.hpp:548-566), srcType CV_8UC1 or CV_32FC1: float32
    (h, w) response map with the CPU cornerMinEigenVal / cornerHarris numerics
    (corner.cpp:52-152,237-326).  A uint16 source gives the float32 result of the same
    values; float pixels must be finite."""
    pix, pitch = _corner_image(src, "corner_response")
    ctx = ctx or Context.get(src.device.index or 0)
    h, w = src.shape
    dst = torch.empty((h, w), dtype=torch.float32, device=src.device)
    if pix == _lib.TBDK_PIX_U8:
        _lib.check(ctx.lib.tbdk_corner_response(ctx.handle, C.c_void_p(src.data_ptr()), w, h, pitch,
                                                C.c_void_p(dst.data_ptr()), dst.stride(0) * 4, int(block_size),
                                                1 if harris else 0, float(k), _stream_ptr(stream)),
                   "tbdk_corner_response")
    else:
        _lib.check(ctx.lib.tbdk_corner_response_px(ctx.handle, C.c_void_p(src.data_ptr()), pix, w, h, pitch,
                                                   C.c_void_p(dst.data_ptr()), dst.stride(0) * 4, int(block_size),
                                                   1 if harris else 0, float(k), _stream_ptr(stream)),
                   "tbdk_corner_response_px")
    return dst


# numpy mirror of tbdk_box_fit (include/tbdk.h)
BOX_FIT_DTYPE = np.dtype([("m", "<f8", 6), ("cx", "<f8"), ("cy", "<f8"), ("npoints", "<i4"), ("valid", "<i4")])


def box_propagate(prev_pts: torch.Tensor, next_pts: torch.Tensor, status, offsets: torch.Tensor,
                  boxes: torch.Tensor, min_points: int = 4, ctx: Context | None = None, stream=None) -> np.ndarray:
    """tbdk_box_propagate: per box b, the 4-DOF similarity (getRTMatrix, non
    full-affine) fitted to points offsets[b]..offsets[b+1] (status != 0 only)
    and the box centre it carries.  Device tensors: prev/next float32 (N, 2),
    status uint8 (N) or None, offsets int32 (nboxes + 1), boxes int32
    (nboxes, 4).  Returns a BOX_FIT_DTYPE array (synchronises the stream)."""
    for t in (prev_pts, next_pts, offsets, boxes) + ((status,) if status is not None else ()):
        if not t.is_cuda or not t.is_contiguous():
            raise _lib.TbdkError("box_propagate expects contiguous device tensors")
    nb = boxes.shape[0]
    if offsets.dtype != torch.int32 or boxes.dtype != torch.int32 or offsets.numel() != nb + 1:
        raise _lib.TbdkError("offsets: int32 (nboxes + 1), boxes: int32 (nboxes, 4)")
    ctx = ctx or Context.get(prev_pts.device.index or 0)
    out = torch.zeros(max(1, nb) * BOX_FIT_DTYPE.itemsize, dtype=torch.uint8, device=prev_pts.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    _lib.check(ctx.lib.tbdk_box_propagate(ctx.handle, ptr(prev_pts), ptr(next_pts), ptr(status), ptr(offsets),
                                          ptr(boxes), nb, int(min_points), ptr(out), _stream_ptr(stream)),
               "tbdk_box_propagate")
    res = out.cpu().numpy()
    return np.frombuffer(res.tobytes(), BOX_FIT_DTYPE)[:nb].copy()


def box_propagate_ransac(prev_pts: torch.Tensor, next_pts: torch.Tensor, status, offsets: torch.Tensor,
                          boxes: torch.Tensor, min_points: int = 4, max_iters: int | None = None,
                          good_ratio: float | None = None, ctx: Context | None = None, stream=None):
    """tbdk_box_propagate_ransac: cv::estimateRigidTransform(prev, next, False,
    max_iters, good_ratio, 3) per box (the reference's RANSAC consensus, then
    getRTMatrix over its inliers) and the box centre the transform carries.
    Arguments as box_propagate; max_iters / good_ratio default to the
    reference's 500 / 0.5.  Returns (fit, iters, inliers): a BOX_FIT_DTYPE array
    (npoints = consensus size, -1 for a box of more than 1024 tracked pairs),
    int32 per box (the round that reached consensus, -1: none) and uint8 per
    point (1 = consensus member).  Synchronises the stream."""
    for t in (prev_pts, next_pts, offsets, boxes) + ((status,) if status is not None else ()):
        if not t.is_cuda or not t.is_contiguous():
            raise _lib.TbdkError("box_propagate_ransac expects contiguous device tensors")
    nb = boxes.shape[0]
    if offsets.dtype != torch.int32 or boxes.dtype != torch.int32 or offsets.numel() != nb + 1:
        raise _lib.TbdkError("offsets: int32 (nboxes + 1), boxes: int32 (nboxes, 4)")
    ctx = ctx or Context.get(prev_pts.device.index or 0)
    par = _lib.RansacParams()
    _lib.check(ctx.lib.tbdk_ransac_default_params(C.byref(par)), "tbdk_ransac_default_params")
    if max_iters is not None:
        par.max_iters = int(max_iters)
    if good_ratio is not None:
        par.good_ratio = float(good_ratio)
    npts = prev_pts.shape[0]
    out = torch.zeros(max(1, nb) * BOX_FIT_DTYPE.itemsize, dtype=torch.uint8, device=prev_pts.device)
    iters = torch.full((max(1, nb),), -1, dtype=torch.int32, device=prev_pts.device)
    inl = torch.zeros(max(1, npts), dtype=torch.uint8, device=prev_pts.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    _lib.check(ctx.lib.tbdk_box_propagate_ransac(ctx.handle, ptr(prev_pts), ptr(next_pts), ptr(status), ptr(offsets),
                                                 ptr(boxes), nb, int(min_points), C.byref(par), ptr(out), ptr(iters),
                                                 ptr(inl), _stream_ptr(stream)),
               "tbdk_box_propagate_ransac")
    res = out.cpu().numpy()
    return (np.frombuffer(res.tobytes(), BOX_FIT_DTYPE)[:nb].copy(), iters.cpu().numpy()[:nb].copy(),
            inl.cpu().numpy()[:npts].copy())


# cv::findHomography's methods (calib3d.hpp); LMEDS (4) and RHO (16) are not implemented
LSQ, RANSAC = 0, 8


class Homography:
    """What find_homography returns, all on the device: H float64 [nsets, 3, 3]
    (a view; the identity where valid is 0), mask uint8 per pair, and npoints
    (-1 for a set of more than 4096 status != 0 pairs), ninliers, iters and
    valid as int32 [nsets] views."""

    def __init__(self, raw: torch.Tensor, mask: torch.Tensor, nsets: int):
        self.raw, self.mask = raw, mask
        f = raw.view(torch.float64).view(-1, C.sizeof(_lib.Homography) // 8)[:nsets]
        i = raw.view(torch.int32).view(-1, C.sizeof(_lib.Homography) // 4)[:nsets]
        self.H = f[:, :9].unflatten(1, (3, 3))
        self.npoints, self.ninliers, self.iters, self.valid = i[:, 18], i[:, 19], i[:, 20], i[:, 21]


def find_homography(src_pts: torch.Tensor, dst_pts: torch.Tensor, method: int = RANSAC,
                    ransacReprojThreshold: float = 3.0, maxIters: int = 2000, confidence: float = 0.995,
                    status: torch.Tensor | None = None, offsets: torch.Tensor | None = None, refine: bool = True,
                    ctx: Context | None = None, stream=None) -> Homography:
    """tbdk_find_homography: cv::findHomography(src, dst, method,
    ransacReprojThreshold, mask, maxIters, confidence) per point set, on the
    device.  src_pts / dst_pts: contiguous device float32 (N, 2); status: device
    uint8 (N) or None (status == 0 pairs are dropped); offsets: device int32
    (nsets + 1) or None for one set of all N pairs.  refine=False stops before
    the reference's LM step.  Asynchronous: nothing is copied to the host and
    the stream is not synchronised."""
    for t in (src_pts, dst_pts) + tuple(t for t in (status, offsets) if t is not None):
        if not t.is_cuda or not t.is_contiguous():
            raise _lib.TbdkError("find_homography expects contiguous device tensors")
    npts = src_pts.shape[0]
    if (src_pts.dtype != torch.float32 or dst_pts.dtype != torch.float32 or src_pts.shape != (npts, 2)
            or dst_pts.shape != (npts, 2)):
        raise _lib.TbdkError("src_pts, dst_pts: float32 (N, 2)")
    if status is not None and (status.dtype != torch.uint8 or status.numel() != npts):
        raise _lib.TbdkError("status: uint8 (N)")
    if offsets is None:
        offsets = torch.tensor([0, npts], dtype=torch.int32, device=src_pts.device)
    elif offsets.dtype != torch.int32 or offsets.numel() < 1:
        raise _lib.TbdkError("offsets: int32 (nsets + 1)")
    nsets = offsets.numel() - 1
    ctx = ctx or Context.get(src_pts.device.index or 0)
    par = _lib.HomographyParams()
    _lib.check(ctx.lib.tbdk_homography_default_params(C.byref(par)), "tbdk_homography_default_params")
    par.method, par.reproj_threshold, par.max_iters = int(method), float(ransacReprojThreshold), int(maxIters)
    par.confidence, par.refine = float(confidence), 1 if refine else 0
    raw = torch.zeros(max(1, nsets) * C.sizeof(_lib.Homography), dtype=torch.uint8, device=src_pts.device)
    mask = torch.zeros(npts, dtype=torch.uint8, device=src_pts.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    # an empty point tensor has no storage: any non-null pointer serves, nothing is read through it
    pts = lambda t: C.c_void_p(t.data_ptr() if t.numel() else raw.data_ptr())  # noqa: E731
    _lib.check(ctx.lib.tbdk_find_homography(ctx.handle, pts(src_pts), pts(dst_pts), ptr(status), ptr(offsets), nsets,
                                            C.byref(par), ptr(raw), ptr(mask), _stream_ptr(stream)),
               "tbdk_find_homography")
    return Homography(raw, mask, nsets)


# cv::estimateAffine2D's robust methods (calib3d.hpp); RANSAC is 8 as above
LMEDS = 4


class Affine2D:
    """What estimate_affine_2d / estimate_affine_partial_2d return, all on the
    device: M float64 [nsets, 2, 3] (a view; [1 0 0; 0 1 0] where valid is 0),
    mask uint8 per pair, and npoints (-1 for a set of more than 4096
    status != 0 pairs), ninliers, iters and valid as int32 [nsets] views."""

    def __init__(self, raw: torch.Tensor, mask: torch.Tensor, nsets: int):
        self.raw, self.mask = raw, mask
        f = raw.view(torch.float64).view(-1, C.sizeof(_lib.Affine2D) // 8)[:nsets]
        i = raw.view(torch.int32).view(-1, C.sizeof(_lib.Affine2D) // 4)[:nsets]
        self.M = f[:, :6].unflatten(1, (2, 3))
        self.npoints, self.ninliers, self.iters, self.valid = i[:, 12], i[:, 13], i[:, 14], i[:, 15]


def _estimate_affine(model: int, what: str, src_pts, dst_pts, method, thr, max_iters, confidence, refine_iters,
                     status, offsets, ctx, stream) -> Affine2D:
    for t in (src_pts, dst_pts) + tuple(t for t in (status, offsets) if t is not None):
        if not t.is_cuda or not t.is_contiguous():
            raise _lib.TbdkError(f"{what} expects contiguous device tensors")
    npts = src_pts.shape[0]
    if (src_pts.dtype != torch.float32 or dst_pts.dtype != torch.float32 or src_pts.shape != (npts, 2)
            or dst_pts.shape != (npts, 2)):
        raise _lib.TbdkError("from_pts, to_pts: float32 (N, 2)")
    if status is not None and (status.dtype != torch.uint8 or status.numel() != npts):
        raise _lib.TbdkError("status: uint8 (N)")
    if offsets is None:
        offsets = torch.tensor([0, npts], dtype=torch.int32, device=src_pts.device)
    elif offsets.dtype != torch.int32 or offsets.numel() < 1:
        raise _lib.TbdkError("offsets: int32 (nsets + 1)")
    nsets = offsets.numel() - 1
    ctx = ctx or Context.get(src_pts.device.index or 0)
    par = _lib.Affine2DParams()
    _lib.check(ctx.lib.tbdk_affine2d_default_params(C.byref(par)), "tbdk_affine2d_default_params")
    par.model, par.method, par.reproj_threshold = int(model), int(method), float(thr)
    par.max_iters, par.confidence, par.refine_iters = int(max_iters), float(confidence), int(refine_iters)
    raw = torch.zeros(max(1, nsets) * C.sizeof(_lib.Affine2D), dtype=torch.uint8, device=src_pts.device)
    mask = torch.zeros(npts, dtype=torch.uint8, device=src_pts.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
    # an empty point tensor has no storage: any non-null pointer serves, nothing is read through it
    pts = lambda t: C.c_void_p(t.data_ptr() if t.numel() else raw.data_ptr())  # noqa: E731
    _lib.check(ctx.lib.tbdk_estimate_affine_2d(ctx.handle, pts(src_pts), pts(dst_pts), ptr(status), ptr(offsets),
                                               nsets, C.byref(par), ptr(raw), ptr(mask), _stream_ptr(stream)),
               "tbdk_estimate_affine_2d")
    return Affine2D(raw, mask, nsets)


def estimate_affine_2d(from_pts: torch.Tensor, to_pts: torch.Tensor, method: int = RANSAC,
                       ransacReprojThreshold: float = 3.0, maxIters: int = 2000, confidence: float = 0.99,
                       refineIters: int = 10, status: torch.Tensor | None = None,
                       offsets: torch.Tensor | None = None, ctx: Context | None = None, stream=None) -> Affine2D:
    """tbdk_estimate_affine_2d with the 3-point model: cv::estimateAffine2D(from, to, inliers, method,
    ransacReprojThreshold, maxIters, confidence, refineIters) per point set, on the device (method RANSAC
    or LMEDS).  from_pts / to_pts: contiguous device float32 (N, 2); status: device uint8 (N) or None
    (status == 0 pairs are dropped); offsets: device int32 (nsets + 1) or None for one set of all N pairs.
    refineIters=0 stops before the reference's LM step.  Asynchronous: nothing is copied to the host and
    the stream is not synchronised."""
    return _estimate_affine(_lib.AFFINE2D_FULL, "estimate_affine_2d", from_pts, to_pts, method,
                            ransacReprojThreshold, maxIters, confidence, refineIters, status, offsets, ctx, stream)


def estimate_affine_partial_2d(from_pts: torch.Tensor, to_pts: torch.Tensor, method: int = RANSAC,
                               ransacReprojThreshold: float = 3.0, maxIters: int = 2000, confidence: float = 0.99,
                               refineIters: int = 10, status: torch.Tensor | None = None,
                               offsets: torch.Tensor | None = None, ctx: Context | None = None,
                               stream=None) -> Affine2D:
    """estimate_affine_2d with the 2-point model (rotation, uniform scale, translation):
    cv::estimateAffinePartial2D."""
    return _estimate_affine(_lib.AFFINE2D_PARTIAL, "estimate_affine_partial_2d", from_pts, to_pts, method,
                            ransacReprojThreshold, maxIters, confidence, refineIters, status, offsets, ctx, stream)


# interpolation flags / border modes (reference values, imgproc.hpp / core/base.hpp)
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, WARP_INVERSE_MAP = 0, 1, 2, 3, 16
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101, BORDER_TRANSPARENT = range(6)


def warp_affine(src: torch.Tensor, M, dsize, flags: int = INTER_LINEAR, borderMode: int = BORDER_CONSTANT,
                borderValue: int = 0, dst: torch.Tensor | None = None, ctx: Context | None = None,
                stream=None, valid: torch.Tensor | None = None) -> torch.Tensor:
    """cv::cuda::warpAffine(src, dst, M, dsize, flags, borderMode, borderValue) for CV_8UC1
    (cudawarping.hpp:126) with the CPU cv::warpAffine's fixed-point numerics (bit-exact).
    M: 2x3 (host array-like); dsize = (width, height).  `dst` may be passed to keep its
    contents where BORDER_TRANSPARENT leaves pixels untouched.

    M may also be a CUDA float64 tensor of six elements (estimate_affine_2d(...).M[i]): the matrix is
    then read and inverted on the device when the kernel runs, with no host synchronisation, and the
    result is byte-identical to the host-matrix call's.  `valid`: an optional device int32 element
    (estimate_affine_2d(...).valid[i]); where it reads 0, or M is not finite, dst is left as it was."""
    if src.dtype != torch.uint8 or src.dim() != 2 or not src.is_cuda or src.stride(1) != 1:
        raise _lib.TbdkError("warp_affine expects a 2-D uint8 device tensor")
    ctx = ctx or Context.get(src.device.index or 0)
    dw, dh = int(dsize[0]), int(dsize[1])
    if dst is None:
        dst = torch.zeros((dh, dw), dtype=torch.uint8, device=src.device)
    elif dst.shape != (dh, dw) or dst.dtype != torch.uint8 or dst.stride(1) != 1:
        raise _lib.TbdkError("dst must be a (height, width) uint8 device tensor")
    h, w = src.shape
    if isinstance(M, torch.Tensor) and M.is_cuda:
        if M.dtype != torch.float64 or M.numel() != 6 or not M.is_contiguous():
            raise _lib.TbdkError("warp_affine: a device M is a contiguous float64 tensor of six elements")
        if valid is not None and (not valid.is_cuda or valid.dtype != torch.int32 or valid.numel() != 1):
            raise _lib.TbdkError("warp_affine: valid is one device int32")
        _lib.check(ctx.lib.tbdk_warp_affine_u8_dev(ctx.handle, C.c_void_p(src.data_ptr()), w, h, src.stride(0),
                                                   C.c_void_p(dst.data_ptr()), dw, dh, dst.stride(0),
                                                   C.c_void_p(M.data_ptr()),
                                                   C.c_void_p(valid.data_ptr()) if valid is not None else None,
                                                   int(flags), int(borderMode), int(borderValue),
                                                   _stream_ptr(stream)),
                   "tbdk_warp_affine_u8_dev")
        return dst
    m = (C.c_double * 6)(*[float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)])
    _lib.check(ctx.lib.tbdk_warp_affine_u8(ctx.handle, C.c_void_p(src.data_ptr()), w, h, src.stride(0),
                                           C.c_void_p(dst.data_ptr()), dw, dh, dst.stride(0), m, int(flags),
                                           int(borderMode), int(borderValue), _stream_ptr(stream)),
               "tbdk_warp_affine_u8")
    return dst


# map kinds of remap (tbdk.h: TBDK_MAP_*)
MAP_32FC2, MAP_32FC1, MAP_16SC2 = 0, 1, 2
PIX_U8, PIX_F32 = 0, 2


def _rows_packed(t: torch.Tensor) -> bool:
    """every row contiguous (strides of one-element dimensions carry no meaning)"""
    return t.numel() == 0 or t[0].is_contiguous()


def _pitch(t: torch.Tensor) -> int:
    """row pitch in bytes"""
    row = t[0].numel() if t.shape[0] else 0
    return (t.stride(0) if t.shape[0] > 1 else row) * t.element_size()


def _warp_image(t: torch.Tensor, what: str):
    """(pix, cn) of an (H, W) or (H, W, C) uint8 / float32 device image with packed pixels"""
    if not t.is_cuda or t.dim() not in (2, 3) or t.dtype not in (torch.uint8, torch.float32):
        raise _lib.TbdkError(f"{what} expects an (H, W) or (H, W, C) uint8 or float32 device tensor")
    cn = 1 if t.dim() == 2 else t.shape[2]
    if not 1 <= cn <= 4 or not _rows_packed(t):
        raise _lib.TbdkError(f"{what}: 1 to 4 interleaved channels, packed along a row")
    return (PIX_U8 if t.dtype == torch.uint8 else PIX_F32), cn


def _warp_dst(src: torch.Tensor, dst, dh: int, dw: int, what: str) -> torch.Tensor:
    shape = (dh, dw) if src.dim() == 2 else (dh, dw, src.shape[2])
    if dst is None:
        return torch.zeros(shape, dtype=src.dtype, device=src.device)
    if tuple(dst.shape) != shape or dst.dtype != src.dtype or dst.device != src.device:
        raise _lib.TbdkError(f"{what}: dst must be a {shape} {src.dtype} tensor on src's device")
    _warp_image(dst, what)
    return dst


def _border_value(v):
    a = np.zeros(4, np.float64)
    v = np.atleast_1d(np.asarray(v, np.float64)).reshape(-1)[:4]
    a[:len(v)] = v
    return (C.c_double * 4)(*a)


def _image_args(t: torch.Tensor):
    return t.shape[1], t.shape[0], _pitch(t)


def remap(src: torch.Tensor, map1: torch.Tensor, map2: torch.Tensor | None = None, interpolation: int = INTER_LINEAR,
          borderMode: int = BORDER_CONSTANT, borderValue=0, dst: torch.Tensor | None = None,
          ctx: Context | None = None, stream=None) -> torch.Tensor:
    """cv::cuda::remap / cv::remap(src, dst, map1, map2, interpolation, borderMode, borderValue) for
    CV_8UC1..4 and CV_32FC1..4 with the CPU cv::remap's numerics (bit-exact, whatever the maps hold).
    map1: (H, W, 2) float32 [CV_32FC2]; (H, W) float32 with map2 (H, W) float32 [CV_32FC1 pair];
    (H, W, 2) int16 with map2 (H, W) int16/uint16 bits or None [CV_16SC2 (+ CV_16UC1)].  The result has
    the maps' size.  `dst` may be passed to keep its contents where BORDER_TRANSPARENT skips pixels."""
    pix, cn = _warp_image(src, "remap")
    if not map1.is_cuda or (map2 is not None and not map2.is_cuda):
        raise _lib.TbdkError("remap: device maps")
    dh, dw = map1.shape[0], map1.shape[1]
    packed = _rows_packed(map1) and (map2 is None or _rows_packed(map2))
    if packed and map1.dtype == torch.float32 and map1.dim() == 3 and map1.shape[2] == 2:
        kind, map2 = MAP_32FC2, None
    elif packed and map1.dtype == torch.float32 and map1.dim() == 2 and map2 is not None \
            and map2.dtype == torch.float32 and map2.shape == map1.shape:
        kind = MAP_32FC1
    elif packed and map1.dtype == torch.int16 and map1.dim() == 3 and map1.shape[2] == 2 \
            and (map2 is None or (map2.dtype in (torch.int16, torch.uint16) and map2.shape == map1.shape[:2])):
        kind = MAP_16SC2
    else:
        raise _lib.TbdkError("remap: maps must be CV_32FC2, CV_32FC1 + CV_32FC1, or CV_16SC2 (+ CV_16UC1)")
    ctx = ctx or Context.get(src.device.index or 0)
    dst = _warp_dst(src, dst, dh, dw, "remap")
    _lib.check(ctx.lib.tbdk_remap(ctx.handle, C.c_void_p(src.data_ptr()), pix, cn, *_image_args(src),
                                  C.c_void_p(dst.data_ptr()), *_image_args(dst), C.c_void_p(map1.data_ptr()),
                                  _pitch(map1), C.c_void_p(map2.data_ptr()) if map2 is not None else None,
                                  _pitch(map2) if map2 is not None else 0, kind,
                                  int(interpolation), int(borderMode), _border_value(borderValue), _stream_ptr(stream)),
               "tbdk_remap")
    return dst


def remap_flow(src: torch.Tensor, flow: torch.Tensor, sign: int = 1, interpolation: int = INTER_LINEAR,
               borderMode: int = BORDER_CONSTANT, borderValue=0, dst: torch.Tensor | None = None,
               ctx: Context | None = None, stream=None) -> torch.Tensor:
    """Warps `src` by a dense flow without storing a map: remap by (x + sign*flow.x, y + sign*flow.y),
    byte for byte what remap gives for that float32 map.  flow: (H, W, 2) float32, as
    FarnebackOpticalFlow.calc and DensePyrLKOpticalFlow.calc return it.  sign=+1 warps frame B onto
    frame A given the flow A -> B; sign=-1 is warp_flow of the reference's samples/python/opt_flow.py."""
    pix, cn = _warp_image(src, "remap_flow")
    if not flow.is_cuda or flow.dtype != torch.float32 or flow.dim() != 3 or flow.shape[2] != 2 \
            or not _rows_packed(flow):
        raise _lib.TbdkError("remap_flow: flow must be an (H, W, 2) float32 device tensor")
    ctx = ctx or Context.get(src.device.index or 0)
    dst = _warp_dst(src, dst, flow.shape[0], flow.shape[1], "remap_flow")
    _lib.check(ctx.lib.tbdk_remap_flow(ctx.handle, C.c_void_p(src.data_ptr()), pix, cn, *_image_args(src),
                                       C.c_void_p(dst.data_ptr()), *_image_args(dst), C.c_void_p(flow.data_ptr()),
                                       _pitch(flow), int(sign), int(interpolation), int(borderMode),
                                       _border_value(borderValue), _stream_ptr(stream)), "tbdk_remap_flow")
    return dst


def warp_perspective(src: torch.Tensor, M, dsize, flags: int = INTER_LINEAR, borderMode: int = BORDER_CONSTANT,
                     borderValue=0, dst: torch.Tensor | None = None, ctx: Context | None = None,
                     stream=None, valid: torch.Tensor | None = None) -> torch.Tensor:
    """cv::cuda::warpPerspective(src, dst, M, dsize, flags, borderMode, borderValue) for CV_8UC1..4 and
    CV_32FC1..4 with the CPU cv::warpPerspective's numerics (bit-exact).  M: 3x3 (host array-like, finite);
    dsize = (width, height).  Not equal to warp_affine for an affine M: the two round differently,
    as the reference's two functions do.

    M may also be a CUDA float64 tensor of nine elements (find_homography(...).H[i]): the matrix is
    then read and inverted on the device when the kernel runs, with no host synchronisation, and the
    result is byte-identical to the host-matrix call's.  `valid`: an optional device int32 element
    (find_homography(...).valid[i]); where it reads 0, or M is not finite, dst is left as it was."""
    pix, cn = _warp_image(src, "warp_perspective")
    ctx = ctx or Context.get(src.device.index or 0)
    dst = _warp_dst(src, dst, int(dsize[1]), int(dsize[0]), "warp_perspective")
    if isinstance(M, torch.Tensor) and M.is_cuda:
        if M.dtype != torch.float64 or M.numel() != 9 or not M.is_contiguous():
            raise _lib.TbdkError("warp_perspective: a device M is a contiguous float64 tensor of nine elements")
        if valid is not None and (not valid.is_cuda or valid.dtype != torch.int32 or valid.numel() != 1):
            raise _lib.TbdkError("warp_perspective: valid is one device int32")
        _lib.check(ctx.lib.tbdk_warp_perspective_dev(ctx.handle, C.c_void_p(src.data_ptr()), pix, cn,
                                                     *_image_args(src), C.c_void_p(dst.data_ptr()), *_image_args(dst),
                                                     C.c_void_p(M.data_ptr()),
                                                     C.c_void_p(valid.data_ptr()) if valid is not None else None,
                                                     int(flags), int(borderMode), _border_value(borderValue),
                                                     _stream_ptr(stream)),
                   "tbdk_warp_perspective_dev")
        return dst
    m = (C.c_double * 9)(*[float(v) for v in np.asarray(M, dtype=np.float64).reshape(9)])
    _lib.check(ctx.lib.tbdk_warp_perspective(ctx.handle, C.c_void_p(src.data_ptr()), pix, cn, *_image_args(src),
                                             C.c_void_p(dst.data_ptr()), *_image_args(dst), m, int(flags),
                                             int(borderMode), _border_value(borderValue), _stream_ptr(stream)),
               "tbdk_warp_perspective")
    return dst


# cv::ColorConversionCodes the front end knows (imgproc.hpp)
COLOR_BGR2BGRA, COLOR_BGR2GRAY, COLOR_RGB2GRAY = _lib.COLOR_BGR2BGRA, _lib.COLOR_BGR2GRAY, _lib.COLOR_RGB2GRAY
COLOR_GRAY2BGR, COLOR_BGRA2GRAY, COLOR_RGBA2GRAY = _lib.COLOR_GRAY2BGR, _lib.COLOR_BGRA2GRAY, _lib.COLOR_RGBA2GRAY
# code -> (source channels, destination channels)
_COLOR_CN = {COLOR_BGR2BGRA: (3, 4), COLOR_BGR2GRAY: (3, 1), COLOR_RGB2GRAY: (3, 1), COLOR_GRAY2BGR: (1, 3),
             COLOR_BGRA2GRAY: (4, 1), COLOR_RGBA2GRAY: (4, 1)}


def _image_cn(img: torch.Tensor, what: str) -> int:
    """Channel count of a u8 device image (H, W) or (H, W, cn) with packed pixels."""
    if img.dtype != torch.uint8 or not img.is_cuda or img.dim() not in (2, 3) or img.stride(-1) != 1:
        raise _lib.TbdkError(f"{what} expects a uint8 device tensor (H, W) or (H, W, cn)")
    if img.dim() == 3 and img.stride(1) != img.shape[2]:
        raise _lib.TbdkError(f"{what}: pixels must be packed (stride(1) == channels)")
    return 1 if img.dim() == 2 else int(img.shape[2])


def _image_dst(dst, h: int, w: int, cn: int, device, what: str) -> torch.Tensor:
    shape = (h, w) if cn == 1 else (h, w, cn)
    if dst is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if tuple(dst.shape) != shape or _image_cn(dst, what) != cn or dst.device != device:
        raise _lib.TbdkError(f"{what}: dst must be a {shape} uint8 device tensor")
    return dst


def cvt_color(src: torch.Tensor, code: int, dst: torch.Tensor | None = None, ctx: Context | None = None,
              stream=None) -> torch.Tensor:
    """cv::cuda::cvtColor(src, dst, code) for 8-bit images (cudaimgproc.hpp) with the
    CPU cv::cvtColor's bits: COLOR_BGR2GRAY / RGB2GRAY / BGRA2GRAY / RGBA2GRAY,
    COLOR_BGR2BGRA (alpha 255) and COLOR_GRAY2BGR.  Any other code, or a source
    whose channel count does not fit the code, raises."""
    cn = _image_cn(src, "cvt_color")
    if code not in _COLOR_CN:
        raise _lib.TbdkError(f"cvt_color: unknown colour conversion code {code}")
    if cn != _COLOR_CN[code][0]:
        raise _lib.TbdkError(f"cvt_color: code {code} needs {_COLOR_CN[code][0]} source channels, got {cn}")
    ctx = ctx or Context.get(src.device.index or 0)
    h, w = src.shape[:2]
    dst = _image_dst(dst, h, w, _COLOR_CN[code][1], src.device, "cvt_color")
    _lib.check(ctx.lib.tbdk_cvt_color_u8(ctx.handle, C.c_void_p(src.data_ptr()), w, h, src.stride(0),
                                         C.c_void_p(dst.data_ptr()), dst.stride(0), int(code), _stream_ptr(stream)),
               "tbdk_cvt_color_u8")
    return dst


def resize_linear(src: torch.Tensor, dsize, dst: torch.Tensor | None = None, ctx: Context | None = None,
                  stream=None) -> torch.Tensor:
    """cv::cuda::resize(src, dst, dsize, 0, 0, INTER_LINEAR) for 8-bit images of 1, 3 or 4
    channels (cudawarping.hpp) with the CPU cv::resize's fixed-point bits.  dsize = (width, height)."""
    cn = _image_cn(src, "resize_linear")
    if cn not in (1, 3, 4):
        raise _lib.TbdkError("resize_linear: 1, 3 or 4 channels")
    dw, dh = int(dsize[0]), int(dsize[1])
    if dw <= 0 or dh <= 0:
        raise _lib.TbdkError("resize_linear: empty dsize")
    ctx = ctx or Context.get(src.device.index or 0)
    h, w = src.shape[:2]
    dst = _image_dst(dst, dh, dw, cn, src.device, "resize_linear")
    _lib.check(ctx.lib.tbdk_resize_linear_u8(ctx.handle, C.c_void_p(src.data_ptr()), w, h, src.stride(0), cn,
                                             C.c_void_p(dst.data_ptr()), dw, dh, dst.stride(0), _stream_ptr(stream)),
               "tbdk_resize_linear_u8")
    return dst


def cvt_resize_gray(src: torch.Tensor, code: int, dsize, dst: torch.Tensor | None = None,
                    ctx: Context | None = None, stream=None) -> torch.Tensor:
    """resize_linear(cvt_color(src, code), dsize) for a *2GRAY code in one pass (the same bits)."""
    cn = _image_cn(src, "cvt_resize_gray")
    if _COLOR_CN.get(code, (0, 0))[1] != 1 or _COLOR_CN[code][0] != cn:
        raise _lib.TbdkError("cvt_resize_gray: a *2GRAY code matching the source's channels")
    dw, dh = int(dsize[0]), int(dsize[1])
    if dw <= 0 or dh <= 0:
        raise _lib.TbdkError("cvt_resize_gray: empty dsize")
    ctx = ctx or Context.get(src.device.index or 0)
    h, w = src.shape[:2]
    dst = _image_dst(dst, dh, dw, 1, src.device, "cvt_resize_gray")
    _lib.check(ctx.lib.tbdk_cvt_resize_gray_u8(ctx.handle, C.c_void_p(src.data_ptr()), w, h, src.stride(0), int(code),
                                               C.c_void_p(dst.data_ptr()), dw, dh, dst.stride(0),
                                               _stream_ptr(stream)), "tbdk_cvt_resize_gray_u8")
    return dst


@dataclass
class LkResult:
    next_pts: torch.Tensor
    status: torch.Tensor
    err: torch.Tensor | None
    iters: torch.Tensor | None


@dataclass
class LkCheckedResult(LkResult):
    """calc_checked: the forward pass's LkResult with the checked status, plus the
    points tracked back and their distance to prevPts"""
    back_pts: torch.Tensor
    fb_err: torch.Tensor


class SparsePyrLKOpticalFlow:
    """cv::cuda::SparsePyrLKOpticalFlow with the CPU calcOpticalFlowPyrLK numerics.

    create(winSize=(21,21), maxLevel=3, iters=30, useInitialFlow=False) mirrors
    cudaoptflow.hpp:175-179; epsilon / minEigThreshold / getMinEigenVals are the
    CPU calcOpticalFlowPyrLK parameters (video/include/opencv2/video/tracking.hpp:178-183).
    """

    def __init__(self, winSize=(21, 21), maxLevel: int = 3, iters: int = 30, useInitialFlow: bool = False,
                 epsilon: float = 0.01, minEigThreshold: float = 1e-4, getMinEigenVals: bool = False,
                 device: int = 0, impl: int = 0):
        self.win = (int(winSize[0]), int(winSize[1]))
        self.max_level = int(maxLevel)
        self.iters = int(iters)
        self.use_initial_flow = bool(useInitialFlow)
        self.epsilon = float(epsilon)
        self.min_eig = float(minEigThreshold)
        self.get_min_eig = bool(getMinEigenVals)
        self.impl = int(impl)
        self.ctx = Context.get(device)

    @staticmethod
    def create(winSize=(21, 21), maxLevel: int = 3, iters: int = 30, useInitialFlow: bool = False, **kw):
        return SparsePyrLKOpticalFlow(winSize, maxLevel, iters, useInitialFlow, **kw)

    # getters / setters of cudaoptflow.hpp:163-173
    def getWinSize(self):
        return self.win

    def setWinSize(self, win):
        self.win = (int(win[0]), int(win[1]))

    def getMaxLevel(self):
        return self.max_level

    def setMaxLevel(self, v):
        self.max_level = int(v)

    def getNumIters(self):
        return self.iters

    def setNumIters(self, v):
        self.iters = int(v)

    def getUseInitialFlow(self):
        return self.use_initial_flow

    def setUseInitialFlow(self, v):
        self.use_initial_flow = bool(v)

    def params(self) -> _lib.LkParams:
        flags = 0
        if self.use_initial_flow:
            flags |= _lib.OPTFLOW_USE_INITIAL_FLOW
        if self.get_min_eig:
            flags |= _lib.OPTFLOW_LK_GET_MIN_EIGENVALS
        return _lib.LkParams(self.win[0], self.win[1], self.max_level, self.iters, self.epsilon, flags,
                             self.min_eig, self.impl)

    def _as_pyr(self, img) -> Pyramid:
        if isinstance(img, Pyramid):
            return img  # prebuilt pyramids: any channel count, as calcOpticalFlowPyrLK
        if torch.is_tensor(img) and img.dim() == 3 and img.shape[2] == 2:
            # the CUDA class takes 1, 3 or 4 channels (CV_Assert, cudaoptflow/src/pyrlk.cpp:142,228)
            raise _lib.TbdkError("SparsePyrLKOpticalFlow.calc: frames must have 1, 3 or 4 channels")
        return build_pyramid(img, self.win, self.max_level, self.ctx)

    def calc(self, prevImg, nextImg, prevPts: torch.Tensor, nextPts: torch.Tensor | None = None,
             want_err: bool = True, want_iters: bool = False, stream=None) -> LkResult:
        if prevPts.dtype != torch.float32 or not prevPts.is_cuda:
            raise _lib.TbdkError("prevPts must be a float32 device tensor of shape (N, 2)")
        pts = prevPts.reshape(-1, 2).contiguous()
        n = pts.shape[0]
        dev = pts.device
        if n == 0:
            return LkResult(torch.empty((0, 2), dtype=torch.float32, device=dev),
                            torch.empty((0,), dtype=torch.uint8, device=dev), None, None)
        P, N = self._as_pyr(prevImg), self._as_pyr(nextImg)
        if self.use_initial_flow:
            if nextPts is None or nextPts.numel() != 2 * n:
                raise _lib.TbdkError("useInitialFlow requires nextPts of the same size as prevPts")
            out = nextPts.reshape(-1, 2).to(torch.float32).contiguous().clone()
        else:
            out = torch.empty((n, 2), dtype=torch.float32, device=dev)
        status = torch.empty((n,), dtype=torch.uint8, device=dev)
        err = torch.empty((n,), dtype=torch.float32, device=dev) if want_err else None
        iters = torch.empty((n,), dtype=torch.int32, device=dev) if want_iters else None
        prm = self.params()
        _lib.check(self.ctx.lib.tbdk_lk_sparse(
            self.ctx.handle, C.byref(P.pyr), C.byref(N.pyr), C.c_void_p(pts.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(status.data_ptr()), C.c_void_p(err.data_ptr()) if err is not None else None,
            C.c_void_p(iters.data_ptr()) if iters is not None else None, n, C.byref(prm), _stream_ptr(stream)),
            "tbdk_lk_sparse")
        return LkResult(out, status, err, iters)

    def calc_checked(self, prevImg, nextImg, prevPts: torch.Tensor, nextPts: torch.Tensor | None = None,
                     back_threshold: float = 1.0, want_err: bool = True, want_iters: bool = False,
                     stream=None) -> LkCheckedResult:
        """calc with the forward-backward check (tbdk_lk_sparse_fb; the reference
        samples' checkedTrace): the tracked points are tracked back nextImg ->
        prevImg, and status stays 1 only where both passes have status 1 and
        max(|dx|, |dy|) between prevPts and the point tracked back is below
        back_threshold.  next_pts / err / iters are calc's.  back_pts: the points
        tracked back (prevPts where the forward pass lost the point); fb_err: that
        distance (+inf where either pass lost the point).  8-bit one-channel
        frames only."""
        if prevPts.dtype != torch.float32 or not prevPts.is_cuda:
            raise _lib.TbdkError("prevPts must be a float32 device tensor of shape (N, 2)")
        pts = prevPts.reshape(-1, 2).contiguous()
        n = pts.shape[0]
        dev = pts.device
        P, N = self._as_pyr(prevImg), self._as_pyr(nextImg)
        if self.use_initial_flow:
            if nextPts is None or nextPts.numel() != 2 * n:
                raise _lib.TbdkError("useInitialFlow requires nextPts of the same size as prevPts")
            out = nextPts.reshape(-1, 2).to(torch.float32).contiguous().clone()
        else:
            out = torch.empty((n, 2), dtype=torch.float32, device=dev)
        status = torch.empty((n,), dtype=torch.uint8, device=dev)
        err = torch.empty((n,), dtype=torch.float32, device=dev) if want_err else None
        iters = torch.empty((n,), dtype=torch.int32, device=dev) if want_iters else None
        back = torch.empty((n, 2), dtype=torch.float32, device=dev)
        fb_err = torch.empty((n,), dtype=torch.float32, device=dev)
        prm = self.params()
        _lib.check(self.ctx.lib.tbdk_lk_sparse_fb(
            self.ctx.handle, C.byref(P.pyr), C.byref(N.pyr), C.c_void_p(pts.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(status.data_ptr()), C.c_void_p(err.data_ptr()) if err is not None else None,
            C.c_void_p(iters.data_ptr()) if iters is not None else None, C.c_void_p(back.data_ptr()),
            C.c_void_p(fb_err.data_ptr()), n, C.byref(prm), C.c_float(back_threshold), _stream_ptr(stream)),
            "tbdk_lk_sparse_fb")
        return LkCheckedResult(out, status, err, iters, back, fb_err)


class DensePyrLKOpticalFlow(SparsePyrLKOpticalFlow):
    """cv::cuda::DensePyrLKOpticalFlow (cudaoptflow.hpp:182-208; impl
    cudaoptflow/src/pyrlk.cpp:238-299): create(winSize=(13,13), maxLevel=3,
    iters=30, useInitialFlow=False); calc(I0, I1) -> (H, W, 2) float32 flow.
    Numerics: the CPU calcOpticalFlowPyrLK at every pixel (tbdk_lk_dense)."""

    def __init__(self, winSize=(13, 13), maxLevel: int = 3, iters: int = 30, useInitialFlow: bool = False, **kw):
        super().__init__(winSize, maxLevel, iters, useInitialFlow, **kw)

    @staticmethod
    def create(winSize=(13, 13), maxLevel: int = 3, iters: int = 30, useInitialFlow: bool = False, **kw):
        return DensePyrLKOpticalFlow(winSize, maxLevel, iters, useInitialFlow, **kw)

    def calc(self, prevImg, nextImg, flow: torch.Tensor | None = None, want_status: bool = False, stream=None):
        P, N = self._as_pyr(prevImg), self._as_pyr(nextImg)
        w, h = P.pyr.lv[0].width, P.pyr.lv[0].height
        dev = torch.device("cuda", self.ctx.device)
        if flow is None:
            flow = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
        if flow.shape != (h, w, 2) or flow.dtype != torch.float32 or not flow.is_contiguous():
            raise _lib.TbdkError("DensePyrLKOpticalFlow.calc: flow must be a contiguous (H, W, 2) float32 tensor")
        status = torch.empty((h, w), dtype=torch.uint8, device=dev) if want_status else None
        prm = self.params()
        _lib.check(self.ctx.lib.tbdk_lk_dense(
            self.ctx.handle, C.byref(P.pyr), C.byref(N.pyr), C.c_void_p(flow.data_ptr()), 8 * w,
            C.c_void_p(status.data_ptr()) if status is not None else None, w, C.byref(prm), _stream_ptr(stream)),
            "tbdk_lk_dense")
        return (flow, status) if want_status else flow


class GoodFeaturesToTrackDetector:
    """cv::cuda::createGoodFeaturesToTrackDetector(srcType, maxCorners, qualityLevel,
    minDistance, blockSize=3, useHarrisDetector=False, harrisK=0.04)
    (cudaimgproc.hpp:603-604) with the CPU goodFeaturesToTrack semantics, applied
    to a batch of box ROIs of one image, optionally under an 8-bit mask
    (goodFeaturesToTrack's `mask`: the quality threshold comes from the maximum
    over the masked-in pixels, and only they can be corners).  The image is
    uint8 (CV_8UC1), float32 (CV_32FC1, finite pixels) or uint16 (the float32
    result of the same values)."""

    def __init__(self, maxCorners: int = 1000, qualityLevel: float = 0.01, minDistance: float = 0.0,
                 blockSize: int = 3, useHarrisDetector: bool = False, harrisK: float = 0.04, device: int = 0):
        self.prm = _lib.GfttParams(int(maxCorners), float(qualityLevel), float(minDistance), int(blockSize),
                                   1 if useHarrisDetector else 0, float(harrisK))
        self.ctx = Context.get(device)

    def detect_rois(self, image: torch.Tensor, rois, stream=None, mask: torch.Tensor | None = None):
        """rois: iterable of (x, y, w, h).  Returns (corners (nroi, maxCorners, 2) f32,
        counts (nroi,) i32) device tensors; corners are in image coordinates.
        counts are never negative: a ROI with more candidates (or a longer
        accepted list) than the one-workgroup LDS selection holds, a whole frame
        for instance, is selected by the wide path in global scratch, with the
        same corners (context option "gftt_wide" = 1 sends every ROI there).
        mask: optional 2-D uint8 device tensor of the image's shape with
        stride(1) == 1 (any row stride: a slice of a larger tensor works); each
        ROI reads its own rectangle of it (tbdk_gftt_rois_masked).
        image: 2-D uint8, uint16 or float32 device tensor with stride(1) == 1
        (the wider types through tbdk_gftt_rois_px)."""
        pix, pitch = _corner_image(image, "detect")
        if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() != 2 or
                                 mask.device != image.device or mask.shape != image.shape or mask.stride(1) != 1):
            raise _lib.TbdkError("mask must be a 2-D uint8 tensor of the image's shape on its device, stride(1) == 1")
        rois = list(rois)
        n = len(rois)
        arr = (_lib.Roi * max(n, 1))(*[_lib.Roi(int(x), int(y), int(w), int(h)) for (x, y, w, h) in rois])
        corners = torch.zeros((n, self.prm.max_corners, 2), dtype=torch.float32, device=image.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=image.device)
        if pix != _lib.TBDK_PIX_U8:
            _lib.check(self.ctx.lib.tbdk_gftt_rois_px(
                self.ctx.handle, C.c_void_p(image.data_ptr()), pix, image.shape[1], image.shape[0], pitch,
                C.c_void_p(mask.data_ptr()) if mask is not None else None,
                int(mask.stride(0)) if mask is not None else 0, arr, n, C.byref(self.prm),
                C.c_void_p(corners.data_ptr()), C.c_void_p(counts.data_ptr()), _stream_ptr(stream)),
                "tbdk_gftt_rois_px")
        elif mask is None:
            _lib.check(self.ctx.lib.tbdk_gftt_rois(self.ctx.handle, C.c_void_p(image.data_ptr()), image.shape[1],
                                                   image.shape[0], image.stride(0), arr, n, C.byref(self.prm),
                                                   C.c_void_p(corners.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                   _stream_ptr(stream)), "tbdk_gftt_rois")
        else:
            _lib.check(self.ctx.lib.tbdk_gftt_rois_masked(
                self.ctx.handle, C.c_void_p(image.data_ptr()), image.shape[1], image.shape[0], image.stride(0),
                C.c_void_p(mask.data_ptr()), int(mask.stride(0)), arr, n, C.byref(self.prm),
                C.c_void_p(corners.data_ptr()), C.c_void_p(counts.data_ptr()), _stream_ptr(stream)),
                "tbdk_gftt_rois_masked")
        return corners, counts

    def detect(self, image: torch.Tensor, stream=None, mask: torch.Tensor | None = None) -> torch.Tensor:
        """Whole image as one ROI -> (K, 2) corners (CornersDetector::detect, with its mask).
        Any frame size and any maxCorners: a frame with more candidates than the
        LDS selection holds goes through the wide selection path (detect_rois)."""
        c, n = self.detect_rois(image, [(0, 0, image.shape[1], image.shape[0])], stream, mask)
        return c[0, :int(n[0].item())]


def subpix_params(win=(10, 10), zero_zone=(-1, -1), criteria=(3, 20, 0.03)) -> _lib.SubpixParams:
    """tbdk_subpix_params of cv::cornerSubPix's (winSize, zeroZone, TermCriteria(type, maxCount, epsilon))"""
    return _lib.SubpixParams(int(win[0]), int(win[1]), int(zero_zone[0]), int(zero_zone[1]), int(criteria[0]),
                             int(criteria[1]), float(criteria[2]))


def corner_sub_pix_mask(win=(10, 10), zero_zone=(-1, -1)) -> np.ndarray:
    """The (2*win_h+1, 2*win_w+1) float32 window mask corner_sub_pix uses
    (tbdk_corner_sub_pix_mask; host only, needs no GPU)."""
    prm = subpix_params(win, zero_zone)
    out = np.zeros((2 * prm.win_h + 1, 2 * prm.win_w + 1), np.float32)
    if not (1 <= prm.win_w <= 15 and 1 <= prm.win_h <= 15):
        raise _lib.TbdkError("corner_sub_pix_mask: win must be 1..15")
    _lib.check(_lib.load().tbdk_corner_sub_pix_mask(C.byref(prm), out.ctypes.data_as(C.c_void_p)),
               "tbdk_corner_sub_pix_mask")
    return out


def corner_sub_pix(image: torch.Tensor, corners: torch.Tensor, win=(10, 10), zero_zone=(-1, -1),
                   criteria=(3, 20, 0.03), counts: torch.Tensor | None = None, ctx: Context | None = None,
                   stream=None) -> torch.Tensor:
    """cv::cornerSubPix(image, corners, win, zero_zone, TermCriteria(*criteria))
    (imgproc/src/cornersubpix.cpp:44-156; the defaults are samples/cpp/lkdemo.cpp:85's),
    on the device, bit-exact with the CPU function (tbdk_corner_sub_pix).
    image: 2-D uint8, uint16 or float32 device tensor with stride(1) == 1 (uint16:
    the float32 result of the same values).  corners: float32 device tensor (n, 2),
    or (rows, cap, 2) with counts (rows,) int32 as detect_rois returns them: row
    r's first counts[r] points are refined (counts None: all of them).  Returns a
    refined copy; the input is not modified."""
    pix, pitch = _corner_image(image, "corner_sub_pix")
    if not isinstance(corners, torch.Tensor) or corners.dtype != torch.float32 or corners.device != image.device or \
            corners.dim() not in (2, 3) or corners.shape[-1] != 2:
        raise _lib.TbdkError("corner_sub_pix: corners must be a float32 (n, 2) or (rows, cap, 2) tensor on the image's device")
    rows, cap = (1, corners.shape[0]) if corners.dim() == 2 else corners.shape[:2]
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or
                               counts.device != image.device or counts.shape != (rows,) or not counts.is_contiguous()):
        raise _lib.TbdkError("corner_sub_pix: counts must be a contiguous int32 (rows,) tensor on the image's device")
    ctx = ctx or Context.get(image.device.index or 0)
    out = corners.clone(memory_format=torch.contiguous_format)
    prm = subpix_params(win, zero_zone, criteria)
    _lib.check(ctx.lib.tbdk_corner_sub_pix(
        ctx.handle, C.c_void_p(image.data_ptr()), pix, image.shape[1], image.shape[0], pitch,
        C.c_void_p(out.data_ptr()), C.c_void_p(counts.data_ptr()) if counts is not None else None, int(rows),
        int(cap), C.byref(prm), _stream_ptr(stream)), "tbdk_corner_sub_pix")
    return out


def hbm_copy(dst: torch.Tensor, src: torch.Tensor, ctx: Context | None = None, stream=None):
    """dst <- src (contiguous device tensors of equal byte size, a multiple of
    16) through libtbdk's 16-byte-per-lane stream-copy kernel (tbdk_hbm_copy;
    bench.py's HBM copy peak)."""
    nbytes = src.numel() * src.element_size()
    if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()) or \
            dst.numel() * dst.element_size() != nbytes:
        raise ValueError("hbm_copy: contiguous device tensors of equal byte size")
    ctx = ctx or Context.get(src.device.index)
    _lib.check(ctx.lib.tbdk_hbm_copy(ctx.handle, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes,
                                     _stream_ptr(stream)), "tbdk_hbm_copy")
    return dst


def synth_render(seed: int, width: int, height: int, nobj: int, t0: int, nframes: int, device: int = 0,
                 ctx: Context | None = None, stream=None):
    """Render frames [t0, t0+nframes) of the synthetic sequence into HBM.

    Returns (frames uint8 (nframes, H, W) device tensor, gt int32 (nframes, nobj, 5) host tensor)."""
    ctx = ctx or Context.get(device)
    frames = torch.empty((nframes, height, width), dtype=torch.uint8, device=f"cuda:{device}")
    gt = torch.zeros((nframes, max(nobj, 1), 5), dtype=torch.int32)
    _lib.check(ctx.lib.tbdk_synth_render(ctx.handle, seed, width, height, nobj, t0, nframes,
                                         C.c_void_p(frames.data_ptr()), width, C.c_void_p(gt.data_ptr()),
                                         _stream_ptr(stream)), "tbdk_synth_render")
    return frames, gt[:, :nobj]


def mask_circles(mask: torch.Tensor, pts: torch.Tensor, radius: int, value: int = 0,
                 count: torch.Tensor | None = None, ctx: Context | None = None, stream=None) -> torch.Tensor:
    """cv::circle(mask, (int(x), int(y)), radius, value, -1) for every point, in
    place and clipped to the mask (tbdk_mask_circles_u8; imgproc/src/drawing.cpp:1486-1628):
    the disc lk_track.py:77-78 cuts out of its detection mask.  mask: 2-D uint8
    device tensor with stride(1) == 1 (any row stride); pts: float32 (n, 2) device
    tensor; radius 0..64; count: optional int32 device tensor (1,), only the first
    min(count, n) points are drawn.  Centres may lie anywhere; a point that is not
    finite draws nothing.  Returns mask."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() != 2 or not mask.is_cuda or \
            mask.stride(1) != 1:
        raise _lib.TbdkError("mask_circles: mask must be a 2-D uint8 device tensor with stride(1) == 1")
    if not isinstance(pts, torch.Tensor) or pts.dtype != torch.float32 or pts.device != mask.device or \
            pts.dim() != 2 or pts.shape[1] != 2 or not pts.is_contiguous():
        raise _lib.TbdkError("mask_circles: pts must be a contiguous float32 (n, 2) tensor on the mask's device")
    if count is not None and (not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or
                              count.device != mask.device or count.numel() != 1):
        raise _lib.TbdkError("mask_circles: count must be an int32 tensor of one element on the mask's device")
    ctx = ctx or Context.get(mask.device.index or 0)
    _lib.check(ctx.lib.tbdk_mask_circles_u8(
        ctx.handle, C.c_void_p(mask.data_ptr()), mask.shape[1], mask.shape[0], int(mask.stride(0)),
        C.c_void_p(pts.data_ptr()), C.c_void_p(count.data_ptr()) if count is not None else None, int(pts.shape[0]),
        int(radius), int(value), _stream_ptr(stream)), "tbdk_mask_circles_u8")
    return mask


@dataclass
class KltTrackerState:
    """KltTracker.read(): the live tracks in order"""
    ids: np.ndarray       # (n,) int32
    last_pts: np.ndarray  # (n, 2) float32
    lens: np.ndarray      # (n,) int32
    hist: np.ndarray      # (n, track_len, 2) float32, oldest first, zero beyond lens
    stats: dict           # tbdk_klt_tracker_stats of the last step


class KltTracker:
    """The loop of the reference's KLT samples (samples/python/lk_track.py App.run,
    samples/cpp/lkdemo.cpp) as one device-resident object (tbdk_klt_tracker, see
    include/tbdk.h): step(frame) tracks every live point with the forward-backward
    check, drops the lost ones, and every detect_interval frames detects new
    corners away from the live ones; nothing is read back until read().

    KltTracker(cfg=None, ctx=None, **overrides): cfg a _lib.KltTrackerConfig
    (KltTracker.default_config(width, height): lk_track's parameters; without one,
    width= and height= are required), overrides its fields by name (win, max_level, lk_iters, lk_epsilon, min_eig_threshold, back_threshold,
    max_corners, quality_level, min_distance, block_size, use_harris, harris_k,
    detect_interval, track_len, mask_radius, subpix_win, max_tracks).

    Unlike lk_track.py:57-60, which looks only at the distance, a point is kept
    only if both PyrLK passes also report it found (tbdk_lk_sparse_fb)."""

    def __init__(self, cfg: _lib.KltTrackerConfig | None = None, ctx: Context | None = None, device: int = 0,
                 **overrides):
        self.handle = None
        self.ctx = ctx or Context.get(device)
        if cfg is None:
            if "width" not in overrides or "height" not in overrides:
                raise _lib.TbdkError("KltTracker: a configuration, or width= and height=")
            cfg = self.default_config(overrides["width"], overrides["height"])
        self.cfg = cfg
        names = {f[0] for f in _lib.KltTrackerConfig._fields_}
        for k, v in overrides.items():
            if k not in names:
                raise _lib.TbdkError(f"KltTracker: unknown configuration field {k}")
            setattr(self.cfg, k, v)
        h = C.c_void_p()
        _lib.check(self.ctx.lib.tbdk_klt_tracker_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)),
                   "tbdk_klt_tracker_create")
        self.handle = h
        self._keep = None

    @staticmethod
    def default_config(width: int, height: int) -> _lib.KltTrackerConfig:
        cfg = _lib.KltTrackerConfig()
        _lib.check(_lib.load().tbdk_klt_tracker_default_config(int(width), int(height), C.byref(cfg)),
                   "tbdk_klt_tracker_default_config")
        return cfg

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.ctx.lib.tbdk_klt_tracker_destroy(h)
            except Exception:
                pass
            self.handle = None

    def step(self, frame: torch.Tensor, detect_now: bool = False, stream=None) -> None:
        """One frame: a 2-D uint8 device tensor of the tracker's size with
        stride(1) == 1.  Only enqueues work; the tracker keeps a reference to the
        frame until the next step.  Steps, add_points and read belong on one stream."""
        if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() != 2 or \
                not frame.is_cuda or frame.stride(1) != 1 or \
                tuple(frame.shape) != (self.cfg.height, self.cfg.width):
            raise _lib.TbdkError("KltTracker.step expects a 2-D uint8 device tensor of the tracker's size")
        _lib.check(self.ctx.lib.tbdk_klt_tracker_step(self.handle, C.c_void_p(frame.data_ptr()), int(frame.stride(0)),
                                                      _lib.TBDK_KLT_DETECT_NOW if detect_now else 0,
                                                      _stream_ptr(stream)), "tbdk_klt_tracker_step")
        self._keep = frame

    def add_points(self, pts, stream=None) -> None:
        """New tracks at caller-supplied points ((n, 2) float32, a device tensor or
        anything numpy converts), under the capacity rule of detection."""
        if not isinstance(pts, torch.Tensor):
            pts = torch.from_numpy(np.ascontiguousarray(pts, np.float32).reshape(-1, 2)).cuda(self.ctx.device)
        if pts.dtype != torch.float32 or not pts.is_cuda or pts.dim() != 2 or pts.shape[1] != 2:
            raise _lib.TbdkError("KltTracker.add_points expects float32 (n, 2) points")
        pts = pts.contiguous()
        _lib.check(self.ctx.lib.tbdk_klt_tracker_add_points(self.handle, C.c_void_p(pts.data_ptr()), int(pts.shape[0]),
                                                            _stream_ptr(stream)), "tbdk_klt_tracker_add_points")
        self._keep_pts = pts

    def reset(self) -> None:
        _lib.check(self.ctx.lib.tbdk_klt_tracker_reset(self.handle), "tbdk_klt_tracker_reset")

    def read(self) -> KltTrackerState:
        """Host copies of the live tracks and the last step's statistics
        (synchronises the stream of the last step)."""
        n, st = C.c_int(), _lib.KltTrackerStats()
        _lib.check(self.ctx.lib.tbdk_klt_tracker_read(self.handle, None, None, None, None, 0, C.byref(n), C.byref(st)),
                   "tbdk_klt_tracker_read")
        k, L = max(int(n.value), 0), int(self.cfg.track_len)
        ids, lens = np.zeros(k, np.int32), np.zeros(k, np.int32)
        last, hist = np.zeros((k, 2), np.float32), np.zeros((k, L, 2), np.float32)
        if k:
            _lib.check(self.ctx.lib.tbdk_klt_tracker_read(
                self.handle, ids.ctypes.data_as(C.c_void_p), last.ctypes.data_as(C.c_void_p),
                lens.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p), k, C.byref(n), C.byref(st)),
                "tbdk_klt_tracker_read")
        return KltTrackerState(ids, last, lens, hist, {f[0]: int(getattr(st, f[0])) for f in st._fields_})

    def tracks(self) -> dict:
        """{id: (len, 2) float32 positions, oldest first} (lk_track's self.tracks)"""
        s = self.read()
        return {int(i): s.hist[k, :int(s.lens[k])].copy() for k, i in enumerate(s.ids)}

    def device_state(self):
        """(count (1,) int32, ids, last_pts (max_tracks, 2), lens, hist (max_tracks,
        track_len, 2)) as torch views of the tracker's device memory, valid until
        the next step; entries at and beyond count are unspecified."""
        p = [C.c_void_p() for _ in range(5)]
        _lib.check(self.ctx.lib.tbdk_klt_tracker_device_state(self.handle, *[C.byref(x) for x in p]),
                   "tbdk_klt_tracker_device_state")
        M, L = int(self.cfg.max_tracks), int(self.cfg.track_len)
        shapes = [((1,), torch.int32), ((M,), torch.int32), ((M, 2), torch.float32), ((M,), torch.int32),
                  ((M, L, 2), torch.float32)]
        return tuple(_device_view(x.value, sh, dt, self.ctx.device) for x, (sh, dt) in zip(p, shapes))


class _DevMem:
    """__cuda_array_interface__ over library-owned device memory"""

    def __init__(self, ptr: int, shape, typestr: str):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2}


def _device_view(ptr: int, shape, dtype: torch.dtype, device: int) -> torch.Tensor:
    typestr = {torch.int32: "<i4", torch.float32: "<f4", torch.uint8: "|u1"}[dtype]
    return torch.as_tensor(_DevMem(ptr, shape, typestr), device=f"cuda:{device}")
