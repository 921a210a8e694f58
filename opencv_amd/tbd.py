"""Host mirror of the reference's tracking-by-detection loop over libtbdk.

`TbdLoop` is one video stream on one GPU: the tracking section of
samples/gpu/tbd.cpp:624-706 (cv::tbd::Tracker::performTrackingStep,
modules/trackingbydetection/src/tbd.cpp:210-286) with the KLT box
propagation (pyramid, GFTT, PyrLK, similarity fit) feeding Track::motionModel
(tbd.hpp:111).  Everything runs in libtbdk.so: HIP kernels for the image work,
native C++ for the tracker bookkeeping.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .klt import Context, _stream_ptr


def default_config(width: int, height: int, **overrides) -> _lib.TbdConfig:
    lib = _lib.load()
    cfg = _lib.TbdConfig()
    _lib.check(lib.tbdk_tbd_default_config(int(width), int(height), C.byref(cfg)), "tbdk_tbd_default_config")
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise _lib.TbdkError(f"unknown TBD config field {k}")
        setattr(cfg, k, v)
    return cfg


# numpy mirror of tbdk_detection (include/tbdk.h): passed to tbdk_tbd_step without a copy
DET_DTYPE = np.dtype([("id", "<i4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"),
                      ("confidence", "<f8")], align=True)
assert DET_DTYPE.itemsize == C.sizeof(_lib.Detection)


def detections_from_gt(gt_frame) -> np.ndarray:
    """GT rows {valid, x, y, w, h} -> detections (id = object index, confidence 1.0),
    as parseDetections builds them from a ground-truth file (samples/gpu/tbd.cpp:1297-1340).
    Returns a DET_DTYPE array (a list of (id, x, y, w, h, conf) tuples is accepted by step too)."""
    g = np.asarray(gt_frame)
    idx = np.nonzero(g[:, 0])[0]
    out = np.zeros(len(idx), DET_DTYPE)
    out["id"] = idx
    out["x"], out["y"], out["width"], out["height"] = g[idx, 1], g[idx, 2], g[idx, 3], g[idx, 4]
    out["confidence"] = 1.0
    return out


class TbdLoop:
    def __init__(self, cfg: _lib.TbdConfig, device: int = 0, ctx: Context | None = None):
        self.ctx = ctx or Context.get(device)
        self.cfg = cfg
        h = C.c_void_p()
        _lib.check(self.ctx.lib.tbdk_tbd_create(self.ctx.handle, C.byref(cfg), C.byref(h)), "tbdk_tbd_create")
        self.handle = h
        self._dets = (_lib.Detection * 4096)()
        self._corner_mask = None

    def set_corner_mask(self, mask: torch.Tensor | None):
        """A static corner mask for the loop's GFTT (tbdk_tbd_set_corner_mask):
        a 2-D uint8 device tensor of the frame's shape with stride(1) == 1, or
        None to clear it.  Only before the first step.  The loop keeps a
        reference; the caller must not change the tensor while the loop lives."""
        if mask is None:
            _lib.check(self.ctx.lib.tbdk_tbd_set_corner_mask(self.handle, None, 0), "tbdk_tbd_set_corner_mask")
            self._corner_mask = None
            return
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() != 2 or not mask.is_cuda or \
                mask.device.index != self.ctx.device or mask.stride(1) != 1 or \
                tuple(mask.shape) != (self.cfg.height, self.cfg.width):
            raise _lib.TbdkError("corner mask must be a 2-D uint8 device tensor of the loop's frame size")
        _lib.check(self.ctx.lib.tbdk_tbd_set_corner_mask(self.handle, C.c_void_p(mask.data_ptr()),
                                                         int(mask.stride(0))), "tbdk_tbd_set_corner_mask")
        self._corner_mask = mask

    @staticmethod
    def _check_frame(frame):
        if frame.dtype != torch.uint8 or frame.dim() != 2 or not frame.is_cuda or frame.stride(1) != 1:
            raise _lib.TbdkError("frame must be a 2-D uint8 device tensor")

    def step(self, frame: torch.Tensor, frame_id: int, dets, stream=None,
             next_frame: torch.Tensor = None) -> _lib.FrameMetrics:
        """One frame (tbdk_tbd_step).  With next_frame (which the next call must
        pass as its frame, unmodified) the next frame's pyramid and the PyrLK the
        tracker step cannot affect run while this step tracks
        (tbdk_tbd_step_ahead); results are the same."""
        self._check_frame(frame)
        n = len(dets)
        if isinstance(dets, np.ndarray):
            if dets.dtype != DET_DTYPE or not dets.flags.c_contiguous:
                raise _lib.TbdkError("detections must be a contiguous DET_DTYPE array")
            dptr = C.cast(dets.ctypes.data, C.POINTER(_lib.Detection))
        else:
            if n > len(self._dets):
                self._dets = (_lib.Detection * (2 * n))()
            for i, (oid, x, y, w, h, conf) in enumerate(dets):
                d = self._dets[i]
                d.id, d.x, d.y, d.width, d.height, d.confidence = oid, x, y, w, h, conf
            dptr = self._dets
        m = _lib.FrameMetrics()
        if next_frame is None:
            _lib.check(self.ctx.lib.tbdk_tbd_step(self.handle, C.c_void_p(frame.data_ptr()), int(frame.stride(0)),
                                                  int(frame_id), dptr, n, C.byref(m), _stream_ptr(stream)),
                       "tbdk_tbd_step")
        else:
            self._check_frame(next_frame)
            _lib.check(self.ctx.lib.tbdk_tbd_step_ahead(
                self.handle, C.c_void_p(frame.data_ptr()), int(frame.stride(0)), int(frame_id), dptr, n,
                C.c_void_p(next_frame.data_ptr()), int(next_frame.stride(0)), C.byref(m), _stream_ptr(stream)),
                "tbdk_tbd_step_ahead")
        return m

    @staticmethod
    def pack_detections(dets_per_frame):
        """(concatenated DET_DTYPE array, int32 offsets) for run()."""
        arrs = [d if isinstance(d, np.ndarray) else np.array([tuple(x) for x in d], dtype=DET_DTYPE)
                for d in dets_per_frame]
        offs = np.zeros(len(arrs) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(a) for a in arrs])
        cat = np.concatenate(arrs).astype(DET_DTYPE, copy=False) if arrs else np.zeros(0, DET_DTYPE)
        return np.ascontiguousarray(cat), offs

    def run(self, frames, first_frame_id: int, dets, stream=None, packed=None):
        """tbdk_tbd_run: the whole frame loop in native code (tbd.cpp:624-706).
        frames: list of equal-pitch 2-D uint8 device tensors; dets: per-frame
        detections (or packed=pack_detections(...) prepared ahead).  Returns the
        per-frame FrameMetrics array."""
        nf = len(frames)
        for f in frames:
            self._check_frame(f)
        if nf and any(f.stride(0) != frames[0].stride(0) for f in frames):
            raise _lib.TbdkError("frames must share one pitch")
        cat, offs = packed if packed is not None else self.pack_detections(dets)
        if len(offs) != nf + 1:
            raise _lib.TbdkError("one detection list per frame")
        ptrs = (C.c_void_p * max(1, nf))(*[f.data_ptr() for f in frames])
        ms = (_lib.FrameMetrics * max(1, nf))()
        _lib.check(self.ctx.lib.tbdk_tbd_run(
            self.handle, ptrs, int(frames[0].stride(0)) if nf else 0, int(first_frame_id),
            C.cast(cat.ctypes.data, C.POINTER(_lib.Detection)),
            C.cast(offs.ctypes.data, C.POINTER(C.c_int32)), nf, ms, _stream_ptr(stream)), "tbdk_tbd_run")
        return ms[:nf]

    def run_host(self, frames: torch.Tensor, first_frame_id: int, dets, stream=None, packed=None):
        """tbdk_tbd_run_host: the frame loop over frames in host memory, uploaded
        into a device ring two frames ahead of their use (frames: a CPU uint8
        tensor (n, H, W) with unit column stride, ideally pinned).  Returns the
        per-frame FrameMetrics array, identical to run()'s on the same frames."""
        if frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 3 or frames.stride(2) != 1:
            raise _lib.TbdkError("frames must be a (n, H, W) uint8 host tensor")
        nf = frames.shape[0]
        cat, offs = packed if packed is not None else self.pack_detections(dets)
        if len(offs) != nf + 1:
            raise _lib.TbdkError("one detection list per frame")
        base, step = frames.data_ptr(), frames.stride(0)
        ptrs = (C.c_void_p * max(1, nf))(*[base + i * step for i in range(nf)])
        ms = (_lib.FrameMetrics * max(1, nf))()
        _lib.check(self.ctx.lib.tbdk_tbd_run_host(
            self.handle, ptrs, int(frames.stride(1)), int(first_frame_id),
            C.cast(cat.ctypes.data, C.POINTER(_lib.Detection)),
            C.cast(offs.ctypes.data, C.POINTER(C.c_int32)), nf, ms, _stream_ptr(stream)), "tbdk_tbd_run_host")
        return ms[:nf]

    def attach_detector(self, hog, src_size=None, src_cn: int = 3, rgb_order: bool = False, make_gray: bool = True,
                        confidence_mode: int = 0, max_detections: int = 4096):
        """Give the loop its own detector (tbdk_tbd_detector_create): `hog` is an
        opencv_amd.hog.HOG with its SVM detector and detectMultiScale settings;
        src_size = (width, height) of the colour frames step_image takes (None:
        the loop's size; another size is resized to it, the sample's --resize_src).
        confidence_mode 0 gives every detection the sample's -1.0, 1 the HOG weight."""
        if hog.svm.size == 0:
            raise _lib.TbdkError("attach_detector: hog.setSVMDetector first")
        self.detach_detector()
        dc = _lib.TbdDetectConfig()
        _lib.check(self.ctx.lib.tbdk_tbd_detect_default_config(self.cfg.width, self.cfg.height, C.byref(dc)),
                   "tbdk_tbd_detect_default_config")
        sw, sh = (self.cfg.width, self.cfg.height) if src_size is None else (int(src_size[0]), int(src_size[1]))
        dc.src_width, dc.src_height, dc.src_cn = sw, sh, int(src_cn)
        dc.rgb_order, dc.make_gray = int(bool(rgb_order)), int(bool(make_gray))
        dc.resize = int((sw, sh) != (self.cfg.width, self.cfg.height))
        dc.confidence_mode, dc.max_detections = int(confidence_mode), int(max_detections)
        C.memmove(C.byref(dc.hog), C.byref(hog.p), C.sizeof(_lib.HogParams))
        h = C.c_void_p()
        _lib.check(self.ctx.lib.tbdk_tbd_detector_create(self.ctx.handle, self.handle, C.byref(dc),
                                                         hog.svm.ctypes.data_as(C.c_void_p), hog.svm.size, C.byref(h)),
                   "tbdk_tbd_detector_create")
        self._det, self._det_cfg = h, dc
        self._det_out = np.zeros(int(max_detections), DET_DTYPE)

    def detach_detector(self):
        h = getattr(self, "_det", None)
        if h is not None and h.value:
            self.ctx.lib.tbdk_tbd_detector_destroy(h)
        self._det = None

    def step_image(self, frame: torch.Tensor, frame_id: int, stream=None):
        """One colour frame through the sample's whole per-frame path
        (tbdk_tbd_step_image): cvtColor -> resize -> HOG detectMultiScale ->
        the loop.  frame: (H, W, 3|4) uint8 device tensor of the attached source
        size ((H, W) for a gray source).  Returns (metrics, detections), the
        detections (a DET_DTYPE array) in the detector's output order."""
        if getattr(self, "_det", None) is None:
            raise _lib.TbdkError("step_image: attach_detector first")
        dc = self._det_cfg
        shape = (dc.src_height, dc.src_width) if dc.src_cn == 1 else (dc.src_height, dc.src_width, dc.src_cn)
        if (frame.dtype != torch.uint8 or not frame.is_cuda or tuple(frame.shape) != shape or frame.stride(-1) != 1
                or (frame.dim() == 3 and frame.stride(1) != dc.src_cn)):
            raise _lib.TbdkError(f"step_image: frame must be a {shape} uint8 device tensor with packed pixels")
        m = _lib.FrameMetrics()
        n = C.c_int()
        out = self._det_out
        _lib.check(self.ctx.lib.tbdk_tbd_step_image(
            self._det, C.c_void_p(frame.data_ptr()), int(frame.stride(0)), int(frame_id),
            C.cast(out.ctypes.data, C.POINTER(_lib.Detection)), len(out), C.byref(n), C.byref(m),
            _stream_ptr(stream)), "tbdk_tbd_step_image")
        return m, out[:n.value].copy()

    def set_trajectories(self, traj: "Trajectories | None"):
        """Record per-object tracking results of detections with ground-truth ids
        (tbdk_tbd_set_trajectories); keep `traj` alive while attached."""
        self._traj = traj
        _lib.check(self.ctx.lib.tbdk_tbd_set_trajectories(self.handle, traj.handle if traj is not None else None),
                   "tbdk_tbd_set_trajectories")

    def write_tracking_output(self, frame_count: int, path: str | None = None, history_ages=None,
                              log_switches: bool = False) -> dict:
        """The sample's tracking output / MOT metrics for this loop (history age 1 per frame)."""
        ages = list(history_ages) if history_ages is not None else [1] * int(frame_count)
        arr = (C.c_uint32 * max(1, len(ages)))(*ages)
        m = _lib.ScenarioMetrics()
        _lib.check(self.ctx.lib.tbdk_tbd_tracking_write(self.handle, arr, len(ages), int(frame_count),
                                                        str(path).encode() if path else None, int(log_switches),
                                                        C.byref(m)), "tbdk_tbd_tracking_write")
        return {k: getattr(m, k) for k, _ in _lib.ScenarioMetrics._fields_}

    def predictions(self) -> dict:
        """{track id: (cx, cy)} of the KLT predictions the last step gave the tracker."""
        arr = (_lib.Prediction * 4096)()
        n = C.c_int()
        _lib.check(self.ctx.lib.tbdk_tbd_predictions(self.handle, arr, 4096, C.byref(n)), "tbdk_tbd_predictions")
        return {arr[i].track_id: (arr[i].cx, arr[i].cy) for i in range(min(n.value, 4096)) if arr[i].valid}

    def tracks(self):
        cap = 4096
        arr = (_lib.TrackInfo * cap)()
        n = C.c_int()
        _lib.check(self.ctx.lib.tbdk_tbd_tracks(self.handle, arr, cap, C.byref(n)), "tbdk_tbd_tracks")
        keys = [f[0] for f in _lib.TrackInfo._fields_]
        return [{k: getattr(arr[i], k) for k in keys} for i in range(min(n.value, cap))]

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.detach_detector()
                self.ctx.lib.tbdk_tbd_destroy(h)
            except Exception:
                pass
            self.handle = None


class Tracker:
    """cv::tbd::Tracker (modules/trackingbydetection/include/opencv2/tbd.hpp:
    121-177) on the host through tbdk_tracker_*: performTrackingStep(detections,
    frame_id) updates the tracks exactly as the reference does; `predictions`
    ({track id: (cx, cy)}) replace a track's constant-velocity motion model for
    that step (the KLT hook of Track::motionModel, tbd.hpp:111)."""

    def __init__(self, bounds=(0, 1280, 0, 720), cost_of_non_assignment: float = 10.0,
                 time_window_size: int = 16, track_age_threshold: int = 4,
                 track_visibility_threshold: float = 0.3, track_confidence_threshold: float = 0.2):
        self.lib = _lib.load()
        a = _lib.TrackerArgs()
        _lib.check(self.lib.tbdk_tracker_default_args(C.byref(a)), "tbdk_tracker_default_args")
        a.cost_of_non_assignment = cost_of_non_assignment
        a.time_window_size = time_window_size
        a.track_age_threshold = track_age_threshold
        a.track_visibility_threshold = track_visibility_threshold
        a.track_confidence_threshold = track_confidence_threshold
        a.bounds_xmin, a.bounds_xmax, a.bounds_ymin, a.bounds_ymax = bounds
        self.handle = C.c_void_p()
        _lib.check(self.lib.tbdk_tracker_create(C.byref(a), C.byref(self.handle)), "tbdk_tracker_create")

    def performTrackingStep(self, detections, frame_id: int, predictions=None,
                            trajectories: "Trajectories | None" = None) -> _lib.FrameMetrics:
        """detections: DET_DTYPE array or (id, x, y, w, h, confidence) tuples;
        trajectories: the trajectoryMap argument of the reference (ground-truth
        detections record their tracking result there)."""
        d = detections if isinstance(detections, np.ndarray) else \
            np.array([tuple(x) for x in detections], dtype=DET_DTYPE)
        d = np.ascontiguousarray(d, dtype=DET_DTYPE)
        preds = predictions or {}
        pa = (_lib.Prediction * max(1, len(preds)))()
        for i, (tid, (cx, cy)) in enumerate(preds.items()):
            pa[i].track_id, pa[i].valid, pa[i].cx, pa[i].cy = tid, 1, cx, cy
        m = _lib.FrameMetrics()
        _lib.check(self.lib.tbdk_tracker_step_traj(
            self.handle, C.cast(d.ctypes.data, C.POINTER(_lib.Detection)), len(d), int(frame_id), pa, len(preds),
            trajectories.handle if trajectories is not None else None, C.byref(m)), "tbdk_tracker_step_traj")
        return m

    def reset(self):
        _lib.check(self.lib.tbdk_tracker_reset(self.handle), "tbdk_tracker_reset")

    def setRand(self, rng: "CRand | None"):
        """Draw new tracks' colours from rng (the reference's global rand())."""
        self._rng = rng
        _lib.check(self.lib.tbdk_tracker_set_rand(self.handle, rng.handle if rng is not None else None), "tbdk_tracker_set_rand")

    def storeTracks(self, buf: "TrackBuffer", slot: int):
        """buf[slot] = getTracks() (the sample's track output buffer)."""
        _lib.check(self.lib.tbdk_tracker_store_tracks(self.handle, buf.handle, int(slot)), "tbdk_tracker_store_tracks")

    def setTracks(self, buf: "TrackBuffer | None", slot: int = -1):
        """setTracks(buf[slot]); no buffer or slot < 0 sets no tracks (tbd.cpp:187-190)."""
        _lib.check(self.lib.tbdk_tracker_load_tracks(self.handle, buf.handle if buf is not None else None, int(slot)),
                   "tbdk_tracker_load_tracks")

    def getTracks(self):
        """TrackInfo records in the tracker's order (Tracker::getTracks, tbd.hpp:163)."""
        cap = 4096
        out = (_lib.TrackInfo * cap)()
        n = C.c_int()
        _lib.check(self.lib.tbdk_tracker_tracks(self.handle, out, cap, C.byref(n)), "tbdk_tracker_tracks")
        return [out[i] for i in range(min(n.value, cap))]

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.lib.tbdk_tracker_destroy(h)
            except Exception:
                pass
            self.handle = None



class _Handle:
    _destroy = ""

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                getattr(self.lib, self._destroy)(h)
            except Exception:
                pass
            self.handle = None


class CRand(_Handle):
    """glibc rand() with private state (srand(seed)); the sample's rand() is unseeded (seed 1)."""
    _destroy = "tbdk_rand_destroy"

    def __init__(self, seed: int = 1):
        self.lib = _lib.load()
        self.handle = C.c_void_p()
        _lib.check(self.lib.tbdk_rand_create(int(seed), C.byref(self.handle)), "tbdk_rand_create")

    def rand(self) -> int:
        v = C.c_int32()
        _lib.check(self.lib.tbdk_rand_next(self.handle, C.byref(v)), "tbdk_rand_next")
        return v.value

    def history_age(self, dist) -> int:
        """The sample's history-age draw over a normalised distribution."""
        a = (C.c_float * len(dist))(*dist)
        age = C.c_uint32()
        _lib.check(self.lib.tbdk_history_age(self.handle, a, len(dist), C.byref(age)), "tbdk_history_age")
        return age.value


def parse_history_distribution(s: str) -> list:
    """Args::parseHistoryDistribution (samples/gpu/tbd.cpp:258-291)."""
    lib = _lib.load()
    out = (C.c_float * 256)()
    n = C.c_int()
    _lib.check(lib.tbdk_parse_history_distribution(s.encode(), out, 256, C.byref(n)),
               "tbdk_parse_history_distribution")
    return [out[i] for i in range(min(n.value, 256))]


class Trajectories(_Handle):
    """std::map<int, cv::tbd::Trajectory> (tbd.hpp:46-80)."""
    _destroy = "tbdk_trajectories_destroy"

    def __init__(self):
        self.lib = _lib.load()
        self.handle = C.c_void_p()
        _lib.check(self.lib.tbdk_trajectories_create(C.byref(self.handle)), "tbdk_trajectories_create")

    def addPosition(self, obj_id: int, frame: int, x: int, y: int, w: int, h: int):
        _lib.check(self.lib.tbdk_trajectories_add_position(self.handle, obj_id, frame, x, y, w, h),
                   "tbdk_trajectories_add_position")

    def __len__(self):
        n = C.c_int()
        _lib.check(self.lib.tbdk_trajectories_count(self.handle, C.byref(n)), "tbdk_trajectories_count")
        return n.value


class TrackBuffer(_Handle):
    """The sample's per-history-age track output buffers (samples/gpu/tbd.cpp:524-531)."""
    _destroy = "tbdk_track_buffer_destroy"

    def __init__(self, nslots: int):
        self.lib = _lib.load()
        self.handle = C.c_void_p()
        _lib.check(self.lib.tbdk_track_buffer_create(int(nslots), C.byref(self.handle)), "tbdk_track_buffer_create")


PEDESTRIANS, VEHICLES = 0, 1


class Sequence(_Handle):
    """Parsed bbox files (parseBboxFile, samples/gpu/tbd.cpp:1163-1295): per class
    the per-frame rows; camera poses and history choices shared between files."""
    _destroy = "tbdk_sequence_destroy"

    def __init__(self):
        self.lib = _lib.load()
        self.handle = C.c_void_p()
        _lib.check(self.lib.tbdk_sequence_create(C.byref(self.handle)), "tbdk_sequence_create")

    def parseBboxFile(self, path: str, num_frames: int, cls: int = PEDESTRIANS):
        rc = self.lib.tbdk_sequence_parse_bbox_file(self.handle, int(cls), str(path).encode(), int(num_frames))
        if rc != _lib.TBDK_OK:
            raise _lib.TbdkError(f"parseBboxFile: {self.lib.tbdk_sequence_error(self.handle).decode()}")

    def info(self, cls: int = PEDESTRIANS):
        nf, npose, nh = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.tbdk_sequence_info(self.handle, int(cls), C.byref(nf), C.byref(npose), C.byref(nh)),
                   "tbdk_sequence_info")
        return nf.value, npose.value, nh.value

    def history(self) -> list:
        n = C.c_int()
        _lib.check(self.lib.tbdk_sequence_history(self.handle, None, 0, C.byref(n)), "tbdk_sequence_history")
        out = (C.c_uint32 * max(1, n.value))()
        _lib.check(self.lib.tbdk_sequence_history(self.handle, out, n.value, C.byref(n)), "tbdk_sequence_history")
        return list(out[:n.value])

    def cameraPose(self, index: int) -> list:
        out = (C.c_double * 16)()
        n = C.c_int()
        _lib.check(self.lib.tbdk_sequence_camera_pose(self.handle, int(index), out, 16, C.byref(n)),
                   "tbdk_sequence_camera_pose")
        return list(out[:min(n.value, 16)])

    def detections(self, frame: int, cls: int = PEDESTRIANS, trajectories: Trajectories | None = None) -> np.ndarray:
        """parseDetections (samples/gpu/tbd.cpp:1297-1340) -> DET_DTYPE array."""
        n = C.c_int()
        tr = trajectories.handle if trajectories is not None else None
        _lib.check(self.lib.tbdk_sequence_detections(self.handle, int(cls), int(frame), None, None, 0, C.byref(n)),
                   "tbdk_sequence_detections")
        out = np.zeros(n.value, DET_DTYPE)
        _lib.check(self.lib.tbdk_sequence_detections(self.handle, int(cls), int(frame), tr,
                                                      C.cast(out.ctypes.data, C.POINTER(_lib.Detection)), n.value,
                                                      C.byref(n)), "tbdk_sequence_detections")
        return out


def write_tracking_output(tracker: Tracker, history_ages, trajectories: Trajectories, frame_count: int,
                          path: str | None = None, log_switches: bool = False) -> dict:
    """App::writeTrackingOutputToFile (samples/gpu/tbd.cpp:946-1120): appends the
    sample's output to path (if given); returns the scenario metrics."""
    lib = _lib.load()
    ages = (C.c_uint32 * max(1, len(history_ages)))(*history_ages)
    m = _lib.ScenarioMetrics()
    _lib.check(lib.tbdk_tracking_write(tracker.handle, ages, len(history_ages), int(frame_count), trajectories.handle,
                                       str(path).encode() if path else None, int(log_switches), C.byref(m)),
               "tbdk_tracking_write")
    return {k: getattr(m, k) for k, _ in _lib.ScenarioMetrics._fields_}


def run_app(pedestrian_bbox_filename=None, vehicle_bbox_filename=None, pedestrian_tracking_filepath=None,
            vehicle_tracking_filepath=None, history_distribution=None, write_tracking=True, num_tracking_iters=1,
            num_tracking_frames=100, seed=1, verbose=False, **tracker_args):
    """The sample's tracking loop over bbox files (tbdk_app_run; CLI: opencv_amd/bin/tbdk_tbd_app).
    Returns {"frames", "detections", "scenario": [pedestrians, vehicles]}."""
    lib = _lib.load()
    a = _lib.AppArgs()
    _lib.check(lib.tbdk_app_default_args(C.byref(a)), "tbdk_app_default_args")
    enc = lambda v: str(v).encode() if v else None  # noqa: E731
    a.pedestrian_bbox_filename = enc(pedestrian_bbox_filename)
    a.vehicle_bbox_filename = enc(vehicle_bbox_filename)
    a.pedestrian_tracking_filepath = enc(pedestrian_tracking_filepath)
    a.vehicle_tracking_filepath = enc(vehicle_tracking_filepath)
    a.history_distribution = enc(history_distribution)
    a.write_tracking = int(bool(write_tracking))
    a.num_tracking_iters = int(num_tracking_iters)
    a.num_tracking_frames = int(num_tracking_frames)
    a.rand_seed = int(seed)
    a.verbose = int(bool(verbose))
    for k, v in tracker_args.items():
        setattr(a.tracker, k, v)
    r = _lib.AppResult()
    _lib.check(lib.tbdk_app_run(C.byref(a), C.byref(r)), "tbdk_app_run")
    sc = [{k: getattr(r.scenario[c], k) for k, _ in _lib.ScenarioMetrics._fields_} for c in range(2)]
    return {"frames": r.frames, "detections": r.detections, "scenario": sc}


def run_app_images(image_list_filename, hog, tracking_filepath=None, num_tracking_frames=100, make_gray=True,
                   resize_src=False, width=640, height=480, confidence_mode=0, device=0, verbose=False,
                   **tracker_args):
    """The sample's loop over an image sequence with no bbox file (tbdk_app_run_images):
    image_list_filename lists binary PNM frames (P6 colour, RGB order, or P5 gray;
    maxval 255), one path per line; `hog` is an opencv_amd.hog.HOG with its SVM
    detector and settings.  Writes the sample's history|object|frame|scenario
    output to tracking_filepath.  Returns {"frames", "detections", "scenario"}."""
    lib = _lib.load()
    if hog.svm.size == 0:
        raise _lib.TbdkError("run_app_images: hog.setSVMDetector first")
    a = _lib.AppImageArgs()
    _lib.check(lib.tbdk_app_image_default_args(C.byref(a)), "tbdk_app_image_default_args")
    a.image_list_filename = str(image_list_filename).encode()
    a.tracking_filepath = str(tracking_filepath).encode() if tracking_filepath else None
    a.num_tracking_frames = int(num_tracking_frames)
    a.make_gray, a.resize_src = int(bool(make_gray)), int(bool(resize_src))
    a.width, a.height = int(width), int(height)
    a.confidence_mode, a.device, a.verbose = int(confidence_mode), int(device), int(bool(verbose))
    C.memmove(C.byref(a.hog), C.byref(hog.p), C.sizeof(_lib.HogParams))
    svm = np.ascontiguousarray(hog.svm, dtype=np.float32)
    a.svm = svm.ctypes.data_as(C.POINTER(C.c_float))
    a.svm_len = svm.size
    for k, v in tracker_args.items():
        if not hasattr(a.tracker, k):
            raise _lib.TbdkError(f"unknown tracker argument {k}")
        setattr(a.tracker, k, v)
    r = _lib.AppImageResult()
    _lib.check(lib.tbdk_app_run_images(C.byref(a), C.byref(r)), "tbdk_app_run_images")
    return {"frames": r.frames, "detections": r.detections,
            "scenario": {k: getattr(r.scenario, k) for k, _ in _lib.ScenarioMetrics._fields_}}
