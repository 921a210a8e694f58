"""Smoothing, thresholding, mask clean-up and blob extraction over libtbdk (HIP, gfx950).

  * gaussian_blur, get_gaussian_kernel_u8 <- cv::GaussianBlur on CV_8UC1 / 8UC3 / 8UC4 (the fixed-point path,
        modules/imgproc/src/smooth.simd.hpp: GaussianBlurFixedPoint), optionally with a threshold fused in
  * threshold <- cv::threshold on 8-bit and CV_32FC1 images, the five plain types and THRESH_OTSU
  * get_structuring_element <- cv::getStructuringElement
  * erode, dilate, morphology_ex <- cv::erode / cv::dilate / cv::morphologyEx (MORPH_ERODE, MORPH_DILATE,
        MORPH_OPEN, MORPH_CLOSE; modules/imgproc/src/morph.dispatch.cpp), cv::cuda::createMorphologyFilter
  * connected_components, connected_components_with_stats <- cv::connectedComponents /
        cv::connectedComponentsWithStats (modules/imgproc/src/connectedcomponents.cpp), CV_32S labels

Results are the CPU implementation's, bit for bit, label numbering included.  Images are uint8 H x W torch
tensors on the HIP device, contiguous or pitched views (unit stride inside a row); everything returned stays on
the device, N included, and no call synchronises with the host.  A structuring element is a host array (numpy,
or anything numpy converts), as get_structuring_element returns it.  Invalid arguments raise TbdkError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .klt import BORDER_CONSTANT, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, Context, _stream_ptr  # noqa: F401

BORDER_WRAP = 3  # cv::BORDER_WRAP (gaussian_blur only)
THRESH_BINARY, THRESH_BINARY_INV, THRESH_TRUNC, THRESH_TOZERO, THRESH_TOZERO_INV = range(5)  # cv::ThresholdTypes
THRESH_OTSU = 8

MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3  # cv::MorphTypes
MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2  # cv::MorphShapes
CCL_WU, CCL_DEFAULT, CCL_GRANA = 0, -1, 1  # cv::ConnectedComponentsAlgorithmsTypes
CC_STAT_LEFT, CC_STAT_TOP, CC_STAT_WIDTH, CC_STAT_HEIGHT, CC_STAT_AREA = range(5)
DEFAULT_BORDER_VALUE = -1  # cv::morphologyDefaultBorderValue()


def get_structuring_element(shape: int, ksize, anchor=(-1, -1)) -> np.ndarray:
    """cv::getStructuringElement(shape, Size(ksize), anchor): a (height, width) uint8 array of 0 / 1"""
    kw, kh = int(ksize[0]), int(ksize[1])
    if kw < 1 or kh < 1:
        raise _lib.TbdkError(f"get_structuring_element: bad size {ksize}")
    out = np.empty((kh, kw), np.uint8)
    _lib.check(_lib.load().tbdk_structuring_element(int(shape), kw, kh, int(anchor[0]), int(anchor[1]),
                                                    out.ctypes.data_as(C.c_void_p)), "tbdk_structuring_element")
    return out


def _mask_layout(t: torch.Tensor, what: str):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or t.numel() == 0:
        raise _lib.TbdkError(f"{what}: a non-empty uint8 H x W tensor (CV_8UC1) expected")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise _lib.TbdkError(f"{what}: rows must be dense (a pitched view is fine)")
    return t.shape[0], t.shape[1], max(t.stride(0), t.shape[1])


def morphology_ex(src: torch.Tensor, op: int, kernel, dst: torch.Tensor | None = None, anchor=(-1, -1),
                  iterations: int = 1, borderType: int = BORDER_CONSTANT, borderValue: int = DEFAULT_BORDER_VALUE,
                  stream=None, ctx: Context | None = None) -> torch.Tensor:
    """cv::morphologyEx(src, dst, op, kernel, anchor, iterations, borderType, borderValue) for the four ops built.
    kernel None is the reference's empty Mat (the 3 x 3 rectangle); borderValue -1 is
    morphologyDefaultBorderValue(), otherwise 0..255.  dst may be src."""
    h, w, spitch = _mask_layout(src, "morphology_ex: src")
    if dst is None:
        dst = torch.empty((h, w), dtype=torch.uint8, device=src.device)
    dh, dw, dpitch = _mask_layout(dst, "morphology_ex: dst")
    if (dh, dw) != (h, w) or dst.device != src.device:
        raise _lib.TbdkError("morphology_ex: dst must have src's size and device")
    ctx = ctx or Context.get(src.device.index or 0)
    if kernel is None:
        kptr, kw, kh = None, 3, 3
    else:
        k = np.ascontiguousarray(np.asarray(kernel.cpu() if isinstance(kernel, torch.Tensor) else kernel) != 0,
                                 dtype=np.uint8)
        if k.ndim != 2 or k.size == 0:
            raise _lib.TbdkError("morphology_ex: kernel must be a non-empty 2-D array")
        kptr, kw, kh = k.ctypes.data_as(C.c_void_p), k.shape[1], k.shape[0]
    _lib.check(ctx.lib.tbdk_morph_u8(ctx.handle, int(op), C.c_void_p(src.data_ptr()), w, h, spitch,
                                     C.c_void_p(dst.data_ptr()), dpitch, kptr, kw, kh, int(anchor[0]), int(anchor[1]),
                                     int(iterations), int(borderType), int(borderValue), _stream_ptr(stream)),
               "tbdk_morph_u8")
    return dst


def erode(src, kernel, dst=None, anchor=(-1, -1), iterations: int = 1, borderType: int = BORDER_CONSTANT,
          borderValue: int = DEFAULT_BORDER_VALUE, stream=None, ctx: Context | None = None) -> torch.Tensor:
    """cv::erode(src, dst, kernel, anchor, iterations, borderType, borderValue)"""
    return morphology_ex(src, MORPH_ERODE, kernel, dst, anchor, iterations, borderType, borderValue, stream, ctx)


def dilate(src, kernel, dst=None, anchor=(-1, -1), iterations: int = 1, borderType: int = BORDER_CONSTANT,
           borderValue: int = DEFAULT_BORDER_VALUE, stream=None, ctx: Context | None = None) -> torch.Tensor:
    """cv::dilate(src, dst, kernel, anchor, iterations, borderType, borderValue)"""
    return morphology_ex(src, MORPH_DILATE, kernel, dst, anchor, iterations, borderType, borderValue, stream, ctx)


def _labels_layout(labels, h, w, device):
    if labels is None:
        labels = torch.empty((h, w), dtype=torch.int32, device=device)
    if labels.dtype != torch.int32 or tuple(labels.shape) != (h, w) or labels.stride(1) != 1 or \
            (h > 1 and labels.stride(0) < w) or labels.device != device:
        raise _lib.TbdkError("connected_components: labels must be an H x W int32 tensor with dense rows on the "
                             "image's device")
    return labels, max(labels.stride(0), w) * 4


def connected_components(image: torch.Tensor, labels: torch.Tensor | None = None, connectivity: int = 8,
                         ccltype: int = CCL_DEFAULT, stream=None, ctx: Context | None = None):
    """cv::connectedComponents(image, labels, connectivity, CV_32S, ccltype): (N as a one-element int32 device
    tensor, labels)"""
    h, w, pitch = _mask_layout(image, "connected_components: image")
    labels, lpitch = _labels_layout(labels, h, w, image.device)
    ctx = ctx or Context.get(image.device.index or 0)
    n = torch.empty(1, dtype=torch.int32, device=image.device)
    _lib.check(ctx.lib.tbdk_connected_components(ctx.handle, C.c_void_p(image.data_ptr()), w, h, pitch,
                                                 C.c_void_p(labels.data_ptr()), lpitch, int(connectivity),
                                                 int(ccltype), None, None, 0, C.c_void_p(n.data_ptr()),
                                                 _stream_ptr(stream)), "tbdk_connected_components")
    return n, labels


def connected_components_with_stats(image: torch.Tensor, labels: torch.Tensor | None = None,
                                    stats: torch.Tensor | None = None, centroids: torch.Tensor | None = None,
                                    connectivity: int = 8, ccltype: int = CCL_DEFAULT, max_labels: int = 1024,
                                    stream=None, ctx: Context | None = None):
    """cv::connectedComponentsWithStats(image, labels, stats, centroids, connectivity, CV_32S, ccltype):
    (N, labels, stats, centroids), all on the device.  stats is (max_labels, 5) int32 (CC_STAT_*), centroids
    (max_labels, 2) float64; rows below min(N, max_labels) are written (row 0 is the background's), the others
    are left as they were (zero in tensors allocated here).  N is the true count even above max_labels."""
    h, w, pitch = _mask_layout(image, "connected_components_with_stats: image")
    labels, lpitch = _labels_layout(labels, h, w, image.device)
    cap = int(max_labels)
    if stats is None:
        stats = torch.zeros((cap, 5), dtype=torch.int32, device=image.device)
    if centroids is None:
        centroids = torch.zeros((cap, 2), dtype=torch.float64, device=image.device)
    if cap < 1 or stats.dtype != torch.int32 or tuple(stats.shape) != (cap, 5) or not stats.is_contiguous() or \
            centroids.dtype != torch.float64 or tuple(centroids.shape) != (cap, 2) or not centroids.is_contiguous():
        raise _lib.TbdkError("connected_components_with_stats: stats must be (max_labels, 5) int32 and centroids "
                             "(max_labels, 2) float64, contiguous, max_labels >= 1")
    ctx = ctx or Context.get(image.device.index or 0)
    n = torch.empty(1, dtype=torch.int32, device=image.device)
    _lib.check(ctx.lib.tbdk_connected_components(ctx.handle, C.c_void_p(image.data_ptr()), w, h, pitch,
                                                 C.c_void_p(labels.data_ptr()), lpitch, int(connectivity),
                                                 int(ccltype), C.c_void_p(stats.data_ptr()),
                                                 C.c_void_p(centroids.data_ptr()), cap, C.c_void_p(n.data_ptr()),
                                                 _stream_ptr(stream)), "tbdk_connected_components")
    return n, labels, stats, centroids


def get_gaussian_kernel_u8(n: int, sigma: float) -> np.ndarray:
    """the n coefficients cv::GaussianBlur uses on 8-bit images, in 1/256 units (uint16); they need not sum to 256"""
    if int(n) < 1:
        raise _lib.TbdkError(f"get_gaussian_kernel_u8: bad size {n}")
    out = np.empty(int(n), np.uint16)
    _lib.check(_lib.load().tbdk_gaussian_kernel_u8(int(n), float(sigma), out.ctypes.data_as(C.c_void_p)),
               "tbdk_gaussian_kernel_u8")
    return out


def _image_layout(t: torch.Tensor, what: str, dtypes=(torch.uint8,)):
    """(height, width, channels, pitch in bytes) of an H x W or H x W x C tensor with dense pixels and rows"""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() not in (2, 3) or t.numel() == 0:
        raise _lib.TbdkError(f"{what}: a non-empty H x W or H x W x C tensor of {dtypes} expected")
    h, w, cn = t.shape[0], t.shape[1], (t.shape[2] if t.dim() == 3 else 1)
    if (t.dim() == 3 and cn > 1 and t.stride(2) != 1) or (w > 1 and t.stride(1) != cn) or \
            (h > 1 and t.stride(0) < w * cn):
        raise _lib.TbdkError(f"{what}: pixels and rows must be dense (a pitched view is fine)")
    return h, w, cn, max(t.stride(0), w * cn) * t.element_size()


def _thresh_params(threshold):
    thresh, maxval, type_ = threshold
    return _lib.ThreshParams(float(thresh), float(maxval), int(type_), 0)


def gaussian_blur(src: torch.Tensor, ksize, sigmaX: float, dst: torch.Tensor | None = None, sigmaY: float = 0,
                  borderType: int = BORDER_REFLECT_101, stream=None, threshold=None,
                  ctx: Context | None = None) -> torch.Tensor:
    """cv::GaussianBlur(src, dst, Size(ksize), sigmaX, sigmaY, borderType | BORDER_ISOLATED) on a uint8 H x W,
    H x W x 3 or H x W x 4 tensor, every byte the reference's.  ksize is (width, height), each odd up to 31, or
    <= 0 for the automatic size from sigma.  threshold (thresh, maxval, type), one of the five plain types, is
    applied to every output byte in the same launch.  dst may be src."""
    h, w, cn, spitch = _image_layout(src, "gaussian_blur: src")
    if dst is None:
        dst = torch.empty_like(src, memory_format=torch.contiguous_format)
    dh, dw, dcn, dpitch = _image_layout(dst, "gaussian_blur: dst")
    if (dh, dw, dcn) != (h, w, cn) or dst.device != src.device:
        raise _lib.TbdkError("gaussian_blur: dst must have src's size, channels and device")
    ctx = ctx or Context.get(src.device.index or 0)
    fused = C.byref(_thresh_params(threshold)) if threshold is not None else None
    _lib.check(ctx.lib.tbdk_gaussian_blur_u8(ctx.handle, C.c_void_p(src.data_ptr()), w, h, cn, spitch,
                                             C.c_void_p(dst.data_ptr()), dpitch, int(ksize[0]), int(ksize[1]),
                                             float(sigmaX), float(sigmaY), int(borderType), fused,
                                             _stream_ptr(stream)), "tbdk_gaussian_blur_u8")
    return dst


def threshold(src: torch.Tensor, thresh: float, maxval: float, type: int, dst: torch.Tensor | None = None,
              stream=None, ctx: Context | None = None):
    """cv::threshold(src, dst, thresh, maxval, type) on a uint8 tensor of any channel count or a float32 one.
    Returns (value, dst): value is the threshold the reference returns, a float; with THRESH_OTSU (uint8 H x W
    only) it is a one-element int32 device tensor, written in stream order.  dst may be src."""
    h, w, cn, spitch = _image_layout(src, "threshold: src", (torch.uint8, torch.float32))
    if dst is None:
        dst = torch.empty_like(src, memory_format=torch.contiguous_format)
    dh, dw, dcn, dpitch = _image_layout(dst, "threshold: dst", (src.dtype,))
    if (dh, dw, dcn) != (h, w, cn) or dst.device != src.device:
        raise _lib.TbdkError("threshold: dst must have src's size, channels and device")
    ctx = ctx or Context.get(src.device.index or 0)
    used = C.c_double(0.0)
    word = torch.empty(1, dtype=torch.int32, device=src.device) if int(type) & THRESH_OTSU else None
    _lib.check(ctx.lib.tbdk_threshold(ctx.handle, C.c_void_p(src.data_ptr()), 0 if src.dtype == torch.uint8 else 2,
                                      w, h, cn, spitch, C.c_void_p(dst.data_ptr()), dpitch, float(thresh),
                                      float(maxval), int(type), C.byref(used),
                                      C.c_void_p(word.data_ptr()) if word is not None else None,
                                      _stream_ptr(stream)), "tbdk_threshold")
    return (word if word is not None else used.value), dst
