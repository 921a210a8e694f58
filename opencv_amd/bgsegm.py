"""Background subtraction over libtbdk (HIP, gfx950).

  * BackgroundSubtractorMOG2 <- cv::BackgroundSubtractorMOG2 / cv::cuda::BackgroundSubtractorMOG2
        (modules/video/include/opencv2/video/background_segm.hpp:90-219,
         impl modules/video/src/bgfg_gaussmix2.cpp)
  * BackgroundSubtractorKNN <- cv::BackgroundSubtractorKNN, the CPU class
        (modules/video/include/opencv2/video/background_segm.hpp:222-300,
         impl modules/video/src/bgfg_KNN.cpp; uint8 frames only)
  * detections_from_stats: the stats rows of imgproc.connected_components_with_stats on a cleaned mask as the
        detections TbdLoop.step takes (samples/cpp/segment_objects.cpp's refineSegments, with boxes out)

Numerics are the CPU implementation's, bit for bit (mask, background image and
model).  Frames are uint8 or float32 torch tensors on the HIP device, H x W or
H x W x 3, contiguous or pitched views (unit stride inside a row); the mask is a
uint8 H x W tensor holding 0, the shadow value or 255, in the form
GoodFeaturesToTrackDetector.detect_rois(mask=) and the KLT tracker take.  The
model lives on the device (tbdk_mog2, include/tbdk.h); it is allocated by the
first apply, when the frame's size and type are known, and they may not change
afterwards (the reference would start a new model; make a new object).  Invalid
arguments raise TbdkError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .klt import Context, _stream_ptr

DEPTH_8U, DEPTH_32F = 0, 5  # TBDK_DEPTH_*


def _image_layout(t: torch.Tensor, what: str):
    """(height, width, channels, depth, pitch in bytes) of a frame-like tensor"""
    if t.dtype not in (torch.uint8, torch.float32):
        raise _lib.TbdkError(f"{what}: uint8 or float32 (CV_8U / CV_32F) expected, got {t.dtype}")
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3):
        raise _lib.TbdkError(f"{what}: H x W or H x W x 3 expected, got {tuple(t.shape)}")
    cn = 1 if t.dim() == 2 else 3
    if t.stride(1) != cn or (cn == 3 and t.stride(2) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * cn):
        raise _lib.TbdkError(f"{what}: rows must be dense (a pitched view is fine)")
    return t.shape[0], t.shape[1], cn, DEPTH_8U if t.dtype == torch.uint8 else DEPTH_32F, t.stride(0) * t.element_size()


class BackgroundSubtractorMOG2:
    """cv::BackgroundSubtractorMOG2 (create / apply / getBackgroundImage / getters / setters)."""

    def __init__(self, history: int = 500, varThreshold: float = 16, detectShadows: bool = True,
                 ctx: Context | None = None):
        self.cfg = _lib.Mog2Config()
        _lib.check(_lib.load().tbdk_mog2_config_default(0, 0, DEPTH_8U, 1, C.byref(self.cfg)),
                   "tbdk_mog2_config_default")
        # the reference's constructor keeps its defaults for non-positive arguments (bgfg_gaussmix2.cpp:157-158)
        if history > 0:
            self.cfg.history = int(history)
        if varThreshold > 0:
            self.cfg.var_threshold = float(varThreshold)
        self.cfg.detect_shadows = int(bool(detectShadows))
        self.ctx = ctx
        self.handle = None
        self._dtype = None

    @staticmethod
    def create(history: int = 500, varThreshold: float = 16, detectShadows: bool = True, ctx: Context | None = None):
        return BackgroundSubtractorMOG2(history, varThreshold, detectShadows, ctx=ctx)

    def __del__(self):
        self._release()

    def _release(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.ctx.lib.tbdk_mog2_destroy(h)
            except Exception:
                pass
        self.handle = None

    def _set(self, name, value):
        old = getattr(self.cfg, name)
        setattr(self.cfg, name, value)
        if self.handle is not None:
            rc = self.ctx.lib.tbdk_mog2_set_params(self.handle, C.byref(self.cfg))
            if rc != _lib.TBDK_OK:
                setattr(self.cfg, name, old)
                _lib.check(rc, f"tbdk_mog2_set_params({name})")

    # getters / setters of background_segm.hpp:100-205
    def getHistory(self): return self.cfg.history
    def setHistory(self, v): self._set("history", int(v))
    def getNMixtures(self): return self.cfg.nmixtures

    def setNMixtures(self, v):
        """before the first apply only: the model is laid out for this many modes"""
        if self.handle is not None and int(v) != self.cfg.nmixtures:
            raise _lib.TbdkError("BackgroundSubtractorMOG2.setNMixtures: the model is already allocated")
        self.cfg.nmixtures = int(v)

    def getBackgroundRatio(self): return self.cfg.background_ratio
    def setBackgroundRatio(self, v): self._set("background_ratio", float(v))
    def getVarThreshold(self): return self.cfg.var_threshold
    def setVarThreshold(self, v): self._set("var_threshold", float(v))
    def getVarThresholdGen(self): return self.cfg.var_threshold_gen
    def setVarThresholdGen(self, v): self._set("var_threshold_gen", float(v))
    def getVarInit(self): return self.cfg.var_init
    def setVarInit(self, v): self._set("var_init", float(v))
    def getVarMin(self): return self.cfg.var_min
    def setVarMin(self, v): self._set("var_min", float(v))
    def getVarMax(self): return self.cfg.var_max
    def setVarMax(self, v): self._set("var_max", float(v))
    def getComplexityReductionThreshold(self): return self.cfg.complexity_reduction
    def setComplexityReductionThreshold(self, v): self._set("complexity_reduction", float(v))
    def getDetectShadows(self): return bool(self.cfg.detect_shadows)
    def setDetectShadows(self, v): self._set("detect_shadows", int(bool(v)))
    def getShadowValue(self): return self.cfg.shadow_value
    def setShadowValue(self, v): self._set("shadow_value", int(v) & 255)  # the reference narrows to uchar
    def getShadowThreshold(self): return self.cfg.shadow_threshold
    def setShadowThreshold(self, v): self._set("shadow_threshold", float(v))

    def frames(self) -> int:
        """frames applied since the model was last cleared"""
        if self.handle is None:
            return 0
        n = C.c_int()
        _lib.check(self.ctx.lib.tbdk_mog2_frames(self.handle, C.byref(n)), "tbdk_mog2_frames")
        return n.value

    def reset(self) -> None:
        """the next apply starts from an empty model"""
        if self.handle is not None:
            _lib.check(self.ctx.lib.tbdk_mog2_reset(self.handle), "tbdk_mog2_reset")

    def _ensure(self, image: torch.Tensor):
        h, w, cn, depth, pitch = _image_layout(image, "BackgroundSubtractorMOG2.apply: image")
        c = self.cfg
        if self.handle is not None and (c.width, c.height, c.depth, c.channels) != (w, h, depth, cn):
            raise _lib.TbdkError("BackgroundSubtractorMOG2.apply: the frame's size and type may not change "
                                 f"(model: {c.width}x{c.height}, {c.channels} channels)")
        if self.handle is None:
            if self.ctx is None:
                self.ctx = Context.get(image.device.index or 0)
            c.width, c.height, c.depth, c.channels = w, h, depth, cn
            hd = C.c_void_p()
            _lib.check(self.ctx.lib.tbdk_mog2_create(self.ctx.handle, C.byref(c), C.byref(hd)), "tbdk_mog2_create")
            self.handle = hd
            self._dtype, self._device = image.dtype, image.device
        return h, w, pitch

    def apply(self, image: torch.Tensor, fgmask: torch.Tensor | None = None, learningRate: float = -1,
              stream=None) -> torch.Tensor:
        h, w, pitch = self._ensure(image)
        if fgmask is None:
            fgmask = torch.empty((h, w), dtype=torch.uint8, device=image.device)
        if fgmask.dtype != torch.uint8 or tuple(fgmask.shape) != (h, w) or fgmask.stride(1) != 1 or \
                (h > 1 and fgmask.stride(0) < w):
            raise _lib.TbdkError("BackgroundSubtractorMOG2.apply: fgmask must be an H x W uint8 tensor with dense rows")
        _lib.check(self.ctx.lib.tbdk_mog2_apply(self.handle, C.c_void_p(image.data_ptr()), pitch,
                                                C.c_void_p(fgmask.data_ptr()), max(fgmask.stride(0), w),
                                                float(learningRate), _stream_ptr(stream)), "tbdk_mog2_apply")
        return fgmask

    def getBackgroundImage(self, backgroundImage: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        if self.handle is None:
            raise _lib.TbdkError("BackgroundSubtractorMOG2.getBackgroundImage: no frame applied yet")
        c = self.cfg
        shape = (c.height, c.width) if c.channels == 1 else (c.height, c.width, 3)
        if backgroundImage is None:
            backgroundImage = torch.empty(shape, dtype=self._dtype, device=self._device)
        h, w, cn, depth, pitch = _image_layout(backgroundImage, "BackgroundSubtractorMOG2.getBackgroundImage")
        if (w, h, depth, cn) != (c.width, c.height, c.depth, c.channels):
            raise _lib.TbdkError("BackgroundSubtractorMOG2.getBackgroundImage: the image must have the frames' size and type")
        _lib.check(self.ctx.lib.tbdk_mog2_get_background(self.handle, C.c_void_p(backgroundImage.data_ptr()), pitch,
                                                         _stream_ptr(stream)), "tbdk_mog2_get_background")
        return backgroundImage

    def model(self, stream=None):
        """(weight (H, W, K), variance (H, W, K), mean (H, W, K, cn) float32, modes_used (H, W) uint8): the
        model in the reference's layout; modes at and above modes_used hold what they last held"""
        if self.handle is None:
            raise _lib.TbdkError("BackgroundSubtractorMOG2.model: no frame applied yet")
        c = self.cfg
        h, w, k, cn = c.height, c.width, c.nmixtures, c.channels
        dev = self._device
        weight = torch.empty((h, w, k), dtype=torch.float32, device=dev)
        variance = torch.empty((h, w, k), dtype=torch.float32, device=dev)
        mean = torch.empty((h, w, k, cn), dtype=torch.float32, device=dev)
        used = torch.empty((h, w), dtype=torch.uint8, device=dev)
        _lib.check(self.ctx.lib.tbdk_mog2_get_model(self.handle, C.c_void_p(weight.data_ptr()),
                                                    C.c_void_p(variance.data_ptr()), C.c_void_p(mean.data_ptr()),
                                                    C.c_void_p(used.data_ptr()), _stream_ptr(stream)),
                   "tbdk_mog2_get_model")
        return weight, variance, mean, used


def createBackgroundSubtractorMOG2(history: int = 500, varThreshold: float = 16, detectShadows: bool = True,
                                   ctx: Context | None = None) -> BackgroundSubtractorMOG2:
    """cv::createBackgroundSubtractorMOG2 (bgfg_gaussmix2.cpp:958-962)"""
    return BackgroundSubtractorMOG2(history, varThreshold, detectShadows, ctx=ctx)


class BackgroundSubtractorKNN:
    """cv::BackgroundSubtractorKNN (create / apply / getBackgroundImage / getters / setters), uint8 frames.
    rngState is cv::theRNG().state of the thread that would run the reference: the three next-update planes
    are redrawn from it on the device, with the reference's sequence and its count of steps."""

    def __init__(self, history: int = 500, dist2Threshold: float = 400.0, detectShadows: bool = True,
                 ctx: Context | None = None, rngState: int = 0xffffffff):
        self.cfg = _lib.KnnConfig()
        _lib.check(_lib.load().tbdk_knn_config_default(0, 0, 1, C.byref(self.cfg)), "tbdk_knn_config_default")
        # the reference's constructor keeps its defaults for non-positive arguments (bgfg_KNN.cpp:108,117)
        if history > 0:
            self.cfg.history = int(history)
        if dist2Threshold > 0:
            self.cfg.dist2_threshold = float(dist2Threshold)
        self.cfg.detect_shadows = int(bool(detectShadows))
        self.cfg.rng_state = int(rngState) & 0xffffffffffffffff
        self.ctx = ctx
        self.handle = None

    @staticmethod
    def create(history: int = 500, dist2Threshold: float = 400.0, detectShadows: bool = True,
               ctx: Context | None = None, rngState: int = 0xffffffff):
        return BackgroundSubtractorKNN(history, dist2Threshold, detectShadows, ctx=ctx, rngState=rngState)

    def __del__(self):
        self._release()

    def _release(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.ctx.lib.tbdk_knn_destroy(h)
            except Exception:
                pass
        self.handle = None

    def _set(self, name, value):
        old = getattr(self.cfg, name)
        setattr(self.cfg, name, value)
        if self.handle is not None:
            rc = self.ctx.lib.tbdk_knn_set_params(self.handle, C.byref(self.cfg))
            if rc != _lib.TBDK_OK:
                setattr(self.cfg, name, old)
                _lib.check(rc, f"tbdk_knn_set_params({name})")

    # getters / setters of background_segm.hpp:230-290
    def getHistory(self): return self.cfg.history
    def setHistory(self, v): self._set("history", int(v))
    def getNSamples(self): return self.cfg.nsamples

    def setNSamples(self, v):
        """before the first apply only: the model is laid out for this many samples a list"""
        if self.handle is not None and int(v) != self.cfg.nsamples:
            raise _lib.TbdkError("BackgroundSubtractorKNN.setNSamples: the model is already allocated")
        self.cfg.nsamples = int(v)

    def getDist2Threshold(self): return self.cfg.dist2_threshold
    def setDist2Threshold(self, v): self._set("dist2_threshold", float(v))
    def getkNNSamples(self): return self.cfg.knn_samples
    def setkNNSamples(self, v): self._set("knn_samples", int(v))
    def getDetectShadows(self): return bool(self.cfg.detect_shadows)
    def setDetectShadows(self, v): self._set("detect_shadows", int(bool(v)))
    def getShadowValue(self): return self.cfg.shadow_value
    def setShadowValue(self, v): self._set("shadow_value", int(v) & 255)  # the reference narrows to uchar
    def getShadowThreshold(self): return self.cfg.shadow_threshold
    def setShadowThreshold(self, v): self._set("shadow_threshold", float(v))

    def frames(self) -> int:
        """frames applied since the model was last cleared"""
        if self.handle is None:
            return 0
        n = C.c_int()
        _lib.check(self.ctx.lib.tbdk_knn_frames(self.handle, C.byref(n)), "tbdk_knn_frames")
        return n.value

    def reset(self) -> None:
        """the next apply starts from an empty model; the RNG state stays"""
        if self.handle is not None:
            _lib.check(self.ctx.lib.tbdk_knn_reset(self.handle), "tbdk_knn_reset")

    def _ensure(self, image: torch.Tensor):
        if image.dtype != torch.uint8:
            raise _lib.TbdkError(f"BackgroundSubtractorKNN.apply: image: uint8 (CV_8U) expected, got {image.dtype}")
        h, w, cn, _, pitch = _image_layout(image, "BackgroundSubtractorKNN.apply: image")
        c = self.cfg
        if self.handle is not None and (c.width, c.height, c.channels) != (w, h, cn):
            raise _lib.TbdkError("BackgroundSubtractorKNN.apply: the frame's size and type may not change "
                                 f"(model: {c.width}x{c.height}, {c.channels} channels)")
        if self.handle is None:
            if self.ctx is None:
                self.ctx = Context.get(image.device.index or 0)
            c.width, c.height, c.channels = w, h, cn
            hd = C.c_void_p()
            _lib.check(self.ctx.lib.tbdk_knn_create(self.ctx.handle, C.byref(c), C.byref(hd)), "tbdk_knn_create")
            self.handle = hd
            self._device = image.device
        return h, w, pitch

    def apply(self, image: torch.Tensor, fgmask: torch.Tensor | None = None, learningRate: float = -1,
              stream=None) -> torch.Tensor:
        h, w, pitch = self._ensure(image)
        if fgmask is None:
            fgmask = torch.empty((h, w), dtype=torch.uint8, device=image.device)
        if fgmask.dtype != torch.uint8 or tuple(fgmask.shape) != (h, w) or fgmask.stride(1) != 1 or \
                (h > 1 and fgmask.stride(0) < w):
            raise _lib.TbdkError("BackgroundSubtractorKNN.apply: fgmask must be an H x W uint8 tensor with dense rows")
        _lib.check(self.ctx.lib.tbdk_knn_apply(self.handle, C.c_void_p(image.data_ptr()), pitch,
                                               C.c_void_p(fgmask.data_ptr()), max(fgmask.stride(0), w),
                                               float(learningRate), _stream_ptr(stream)), "tbdk_knn_apply")
        return fgmask

    def getBackgroundImage(self, backgroundImage: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        if self.handle is None:
            raise _lib.TbdkError("BackgroundSubtractorKNN.getBackgroundImage: no frame applied yet")
        c = self.cfg
        shape = (c.height, c.width) if c.channels == 1 else (c.height, c.width, 3)
        if backgroundImage is None:
            backgroundImage = torch.empty(shape, dtype=torch.uint8, device=self._device)
        h, w, cn, depth, pitch = _image_layout(backgroundImage, "BackgroundSubtractorKNN.getBackgroundImage")
        if (w, h, depth, cn) != (c.width, c.height, DEPTH_8U, c.channels):
            raise _lib.TbdkError("BackgroundSubtractorKNN.getBackgroundImage: the image must have the frames' size and type")
        _lib.check(self.ctx.lib.tbdk_knn_get_background(self.handle, C.c_void_p(backgroundImage.data_ptr()), pitch,
                                                        _stream_ptr(stream)), "tbdk_knn_get_background")
        return backgroundImage

    def model(self, stream=None):
        """(samples (H, W, 3 * nN, cn + 1) uint8, index (3, H, W) uint8, next (3, H, W) uint8, counters (3,) int32,
        rng_state (1,) int64 holding the uint64's bits): the model in the reference's layout, the planes and
        counters in the order short, mid, long, and the RNG state after the last fill; all on the device"""
        if self.handle is None:
            raise _lib.TbdkError("BackgroundSubtractorKNN.model: no frame applied yet")
        c = self.cfg
        h, w, n, cn = c.height, c.width, c.nsamples, c.channels
        dev = self._device
        samples = torch.empty((h, w, 3 * n, cn + 1), dtype=torch.uint8, device=dev)
        index = torch.empty((3, h, w), dtype=torch.uint8, device=dev)
        nxt = torch.empty((3, h, w), dtype=torch.uint8, device=dev)
        counters = torch.empty((3,), dtype=torch.int32, device=dev)
        state = torch.empty((1,), dtype=torch.int64, device=dev)
        _lib.check(self.ctx.lib.tbdk_knn_get_model(self.handle, C.c_void_p(samples.data_ptr()),
                                                   C.c_void_p(index.data_ptr()), C.c_void_p(nxt.data_ptr()),
                                                   C.c_void_p(counters.data_ptr()), C.c_void_p(state.data_ptr()),
                                                   _stream_ptr(stream)), "tbdk_knn_get_model")
        return samples, index, nxt, counters, state


def createBackgroundSubtractorKNN(history: int = 500, dist2Threshold: float = 400.0, detectShadows: bool = True,
                                  ctx: Context | None = None, rngState: int = 0xffffffff) -> BackgroundSubtractorKNN:
    """cv::createBackgroundSubtractorKNN (bgfg_KNN.cpp:873-877)"""
    return BackgroundSubtractorKNN(history, dist2Threshold, detectShadows, ctx=ctx, rngState=rngState)


def detections_from_stats(stats: torch.Tensor, n_labels, min_area: int = 1, max_area: int | None = None) -> np.ndarray:
    """The components of imgproc.connected_components_with_stats as detections for tbd.TbdLoop.step: a
    tbd.DET_DTYPE array with id = label, the box LEFT / TOP / WIDTH / HEIGHT and confidence 1.0, label 0 (the
    background) and the components whose area lies outside min_area..max_area left out.  Copies the
    min(N, rows of stats) stats rows to the host, which waits for the current stream: the one transfer of
    the mask -> boxes chain."""
    from .tbd import DET_DTYPE

    n = int(n_labels.reshape(-1)[0].item()) if isinstance(n_labels, torch.Tensor) else int(n_labels)
    rows = stats[:max(0, min(n, stats.shape[0]))].cpu().numpy()
    rows = rows[1:]
    labels = np.arange(1, len(rows) + 1, dtype=np.int32)
    keep = rows[:, 4] >= min_area
    if max_area is not None:
        keep &= rows[:, 4] <= max_area
    rows, labels = rows[keep], labels[keep]
    out = np.zeros(len(rows), DET_DTYPE)
    out["id"] = labels
    out["x"], out["y"], out["width"], out["height"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    out["confidence"] = 1.0
    return out


def smooth_mask(mask: torch.Tensor, ksize=(11, 11), sigma: float = 3.5, thresh: float = 10, dst: torch.Tensor | None = None,
                stream=None, ctx: Context | None = None) -> torch.Tensor:
    """samples/cpp/bgfg_segm.cpp's smoothMask step, GaussianBlur(mask, mask, Size(11, 11), 3.5, 3.5) followed by
    threshold(mask, mask, 10, 255, THRESH_BINARY), as one launch with no intermediate image; every byte is what
    the two reference calls give.  dst None: a new tensor (pass the mask itself for the sample's in-place form)."""
    from . import imgproc

    return imgproc.gaussian_blur(mask, ksize, sigma, dst, sigma, imgproc.BORDER_REFLECT_101, stream,
                                 (thresh, 255, imgproc.THRESH_BINARY), ctx)
