"""Face stage around the RetinaFace network ("next" row f4): detections -> tracks -> u8 tiles.

Mirrors, with the reference's names and argument meaning:
  * `PriorBox(cfg_re50, image_size).forward()`            retina_face/prior_box.py:16-33        -> prior_boxes
  * `RetinaFacePredictor.__call__` after `self.net(image)`  retina_face_predictor.py:70-108      -> FaceDetections
  * `py_cpu_nms`                                          retina_face/py_cpu_nms.py:11-39        -> nms
  * `SimpleFaceTracker`                                   utils/simple_face_tracker.py:10-90     -> SimpleFaceTracker
  * `VideoPredictor.process`                              data/get_face_images.py:38-63          -> VideoTiler.process

What runs where: box / landmark decoding, the confidence filter + NMS + top-k + final threshold (one launch per batch
of frames, only the kept rows return to the host) and the crop + NEAREST resize into the u8 tile buffer are HIP kernels
(`avcer_face_decode`, `avcer_face_nms`, `avcer_crop_tiles`); the IoU/Hungarian tracker acts on a handful of boxes per
frame, is sequential in time and stays on the host, as in the reference (scipy there too).  The RetinaFace-R50
network runs on the same implicit-GEMM kernel as the recognition models (`avcer_face_forward`, mirror
`RetinaFacePredictor` below).  Tiles go straight to `avcer_static_forward`; the reference's JPEG file round trip
(cv2.imwrite -> PIL.Image.open) is gone, which is the only intended difference -- and with `via_jpeg=True`
(`VideoTiler.process`; `faces_via_jpeg` of run_inference and run_dataset) that difference is gone as well: every tile is then what
reading the crop's JPEG file back gives (quality 95, 4:2:0, libjpeg-turbo's arithmetic on both sides, bit for bit what PIL writes
and reads; cv2 is not among this project's dependencies, the claim about it ends at the shared libjpeg defaults), computed on the
device without the file (jpeg.roundtrip_tiles).  Video decoding is not part of this build.
"""
from __future__ import annotations

import math
import os
from functools import lru_cache
from typing import List, Optional, Sequence

import numpy as np
import torch

from scipy.optimize import linear_sum_assignment

from . import packing
from .engine import MODE_DEFAULT

# retina_face/config.py:22-39 (cfg_re50)
CFG_RE50 = {"min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32], "variance": [0.1, 0.2], "clip": False}


@lru_cache(maxsize=8)
def _prior_boxes(h: int, w: int) -> np.ndarray:
    levels = []
    for sizes, step in zip(CFG_RE50["min_sizes"], CFG_RE50["steps"]):
        fh, fw = math.ceil(h / step), math.ceil(w / step)
        cy = ((np.arange(fh, dtype=np.float64) + 0.5) * step / h)[:, None, None]
        cx = ((np.arange(fw, dtype=np.float64) + 0.5) * step / w)[None, :, None]
        sz = np.asarray(sizes, dtype=np.float64)[None, None, :]
        lvl = np.stack(np.broadcast_arrays(cx, cy, sz / w, sz / h), axis=-1)  # [fh, fw, sizes, 4]
        levels.append(lvl.reshape(-1, 4))
    out = np.concatenate(levels).astype(np.float32)
    if CFG_RE50["clip"]:
        out = np.clip(out, 0.0, 1.0)
    out.setflags(write=False)
    return out


def prior_boxes(image_size) -> np.ndarray:
    """Anchors (cx, cy, w, h) as fractions of the image for an image of (height, width)."""
    return _prior_boxes(int(image_size[0]), int(image_size[1]))


class FaceDetections:
    """The post-network half of `RetinaFacePredictor`: same constructor thresholds, same [k,15] float32 result."""

    def __init__(self, engine, threshold: float = 0.8, top_k: int = 750, conf_thresh: float = 0.02,
                 nms_thresh: float = 0.4, nms_top_k: int = 5000):
        self.engine = engine
        self.threshold = threshold
        self.top_k, self.conf_thresh, self.nms_thresh, self.nms_top_k = top_k, conf_thresh, nms_thresh, nms_top_k
        self._priors_dev = {}

    def __call__(self, loc, conf, landms, image_size) -> np.ndarray:
        """loc [P,4], conf [P,2] (softmaxed), landms [P,10] as the network's test phase returns them (batch dim
        squeezed), for an image of (height, width)."""
        key = (int(image_size[0]), int(image_size[1]))
        if key not in self._priors_dev:
            self._priors_dev[key] = torch.from_numpy(np.array(prior_boxes(key))).to(self.engine.device)
        dets = self.engine.face_decode(loc, conf, landms, self._priors_dev[key], key, CFG_RE50["variance"])
        # confidence floor, NMS (py_cpu_nms order), top-k and the final threshold run on the device: only the kept rows
        # and their count come back to the host
        rows, cnt = self.engine.face_nms(dets[None], self.conf_thresh, self.nms_thresh, self.nms_top_k, self.top_k, self.threshold)
        k = int(cnt[0])
        return rows[0, :k].cpu().numpy() if k else np.empty((0, 15), dtype=np.float32)


    def batch(self, loc, conf, landms, image_size) -> List[np.ndarray]:
        """[T,P,*] network outputs of T frames -> one [k,15] array per frame: ONE decode launch, ONE order + NMS launch pair and
        ONE device-to-host copy for the whole batch."""
        key = (int(image_size[0]), int(image_size[1]))
        if key not in self._priors_dev:
            self._priors_dev[key] = torch.from_numpy(np.array(prior_boxes(key))).to(self.engine.device)
        dets = self.engine.face_decode_batch(loc, conf, landms, self._priors_dev[key], key, CFG_RE50["variance"])
        rows, cnt = self.engine.face_nms(dets, self.conf_thresh, self.nms_thresh, self.nms_top_k, self.top_k, self.threshold)
        cnt = cnt.cpu().numpy()
        most = int(cnt.max()) if len(cnt) else 0
        if not most:
            return [np.empty((0, 15), dtype=np.float32) for _ in range(len(cnt))]
        # only the rows some frame kept cross to the host, through a page-locked buffer (torch's host allocator caches the block from
        # call to call; a pageable copy of the worst case -- 750 frames x 750 rows, 34 MB -- is 5 ms with the GPU idle behind it,
        # pinned ~1.4 ms).  The per-frame arrays are VIEWS of that buffer, which they keep alive: no second copy on the host.
        host = torch.empty((int(rows.shape[0]), most, 15), dtype=torch.float32, pin_memory=True)
        host.copy_(rows[:, :most], non_blocking=True)
        torch.cuda.current_stream(rows.device).synchronize()
        rows = host.numpy()
        return [rows[t, :int(cnt[t])] if cnt[t] else np.empty((0, 15), dtype=np.float32) for t in range(len(cnt))]


class RetinaFacePredictor:
    """`RetinaFacePredictor(threshold, device, model)` (retina_face_predictor.py:17-108) on the HIP path: the network,
    box decoding and the device-side filter / NMS / top-k (`FaceDetections`).  `state_dict` = RetinaFace(cfg_re50).state_dict() (the file
    `Resnet50_Final.pth`, with or without the `module.` prefix) or RetinaFace(cfg_mnet).state_dict() (`mobilenet0.25_Final.pth`:
    `get_model("mobilenet0.25")`, retina_face_predictor.py:40-52); the two configurations share the priors and the variances, so
    everything behind the network is the same.  `kind`: 1 = ResNet-50, 2 = MobileNet-0.25 (modes FP32 and F16X3 only)."""

    # algorithmic GFLOP of the network per 640 x 360 frame, what dist.video_cost prices a detector at
    GFLOP_PER_FRAME = {1: 50.7, 2: 1.116}

    def __init__(self, engine, state_dict, threshold: float = 0.8, mode: int = MODE_DEFAULT):
        self.engine, self.mode = engine, mode
        engine.load_face(state_dict)
        self.kind = packing.face_kind(state_dict)
        self.gflop_per_frame = self.GFLOP_PER_FRAME[self.kind]
        self.post = FaceDetections(engine, threshold=threshold)

    def __call__(self, image, rgb: bool = True) -> np.ndarray:
        """image u8 [H,W,3] -> detections [k,15] = x0, y0, x1, y1, score, 5 landmarks (float32)."""
        img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        loc, conf, lm = self.engine.face_forward(img[None], self.mode, rgb=rgb)
        return self.post(loc[0], conf[0], lm[0], (int(img.shape[0]), int(img.shape[1])))

    def batch(self, frames, rgb: bool = False) -> List[np.ndarray]:
        """frames u8 [T,H,W,3] -> one detection array per frame; the network runs once over the whole batch (the
        reference calls it frame by frame, get_face_images.py:49)."""
        x = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        loc, conf, lm = self.engine.face_forward(x, self.mode, rgb=rgb)
        size = (int(x.shape[1]), int(x.shape[2]))
        return self.post.batch(loc, conf, lm, size)


# s3fd_predictor.py:27-42: get_model("s3fd").config and create_config()'s defaults
CFG_S3FD = {"min_sizes": (16, 32, 64, 128, 256, 512), "steps": (4, 8, 16, 32, 64, 128), "variance": (0.1, 0.2), "clip": False,
            "top_k": 750, "conf_thresh": 0.05, "nms_thresh": 0.3, "nms_top_k": 5000}


def s3fd_feature_maps(h: int, w: int):
    """(rows, columns) of the six head inputs of S3FDNet for an h x w frame: two floor pools, the ceil_mode pool (vgg.16), two more
    floor pools, then the two stride-2 extras (3x3, padding 1).  The rule of `avcer_s3fd_num_priors`."""
    def ext(v):
        f = [v // 2 // 2]
        f.append(-(-f[0] // 2))
        f.append(f[1] // 2)
        f.append(f[2] // 2)
        f.append((f[3] - 1) // 2 + 1)
        f.append((f[4] - 1) // 2 + 1)
        return f
    return list(zip(ext(int(h)), ext(int(w))))


@lru_cache(maxsize=8)
def _s3fd_prior_boxes(h: int, w: int) -> np.ndarray:
    levels = []
    for (fh, fw), size, step in zip(s3fd_feature_maps(h, w), CFG_S3FD["min_sizes"], CFG_S3FD["steps"]):
        # utils.py:189-199 in the same Python-float operations: (j + 0.5) / (imw / step), size / imw
        cx = ((np.arange(fw, dtype=np.float64) + 0.5) / (w / step))[None, :]
        cy = ((np.arange(fh, dtype=np.float64) + 0.5) / (h / step))[:, None]
        lvl = np.stack(np.broadcast_arrays(cx, cy, np.float64(size / w), np.float64(size / h)), axis=-1)
        levels.append(lvl.reshape(-1, 4))
    out = np.concatenate(levels).astype(np.float32)
    if CFG_S3FD["clip"]:
        out = np.clip(out, 0.0, 1.0)
    out.setflags(write=False)
    return out


def s3fd_prior_boxes(image_size) -> np.ndarray:
    """`PriorBox(size, feature_maps, config).forward()` of S3FD (s3fd/utils.py:174-206) for an image of (height, width): one anchor
    (cx, cy, w, h) per position of the six levels, computed in Python floats and stored as float32 like the reference's."""
    return _s3fd_prior_boxes(int(image_size[0]), int(image_size[1]))


class S3FDPredictor:
    """`S3FDPredictor(threshold, device, model, config)` (s3fd/s3fd_predictor.py:12-68) on the HIP path: the network
    (`avcer_face_forward`, detector kind 3) and `Detect` plus the predictor's threshold loop in one device-side call
    (`avcer_s3fd_detect`).  `state_dict` = S3FDNet.state_dict() (`s3fd_weights.pth`, with or without a `module.` prefix).
    Results are float32 [k,5] = x0, y0, x1, y1 in pixels, score.  Modes FP32 and F16X3 only.

    When `top_k` boxes all pass the threshold, the reference's loop reads one row past its [top_k, 5] array and raises
    (s3fd_predictor.py:59); this mirror returns those `top_k` rows."""

    kind = packing.FACE_KIND_S3FD
    gflop_per_frame = 144.27   # algorithmic GFLOP per 640 x 360 frame: what dist.video_cost prices it at

    def __init__(self, engine, state_dict, threshold: float = 0.8, mode: int = MODE_DEFAULT, top_k: int = CFG_S3FD["top_k"],
                 conf_thresh: float = CFG_S3FD["conf_thresh"], nms_thresh: float = CFG_S3FD["nms_thresh"],
                 nms_top_k: int = CFG_S3FD["nms_top_k"]):
        if packing.face_kind(state_dict) != packing.FACE_KIND_S3FD:
            raise ValueError("S3FDPredictor: not an S3FDNet state dict")
        self.engine, self.mode, self.threshold = engine, mode, threshold
        self.top_k, self.conf_thresh, self.nms_thresh, self.nms_top_k = top_k, conf_thresh, nms_thresh, nms_top_k
        engine.load_face(state_dict)
        self._priors_dev = {}

    def _rows(self, x, rgb):
        size = (int(x.shape[1]), int(x.shape[2]))
        if size not in self._priors_dev:
            self._priors_dev[size] = torch.from_numpy(np.array(s3fd_prior_boxes(size))).to(self.engine.device)
        # the x3 mode's range contract: a pass that left fp16's range is repeated in f32 (Engine.guarded)
        loc, conf, _ = self.engine.guarded(self.mode, lambda m: self.engine.face_forward(x, m, rgb=rgb))
        return self.engine.s3fd_detect(loc, conf, self._priors_dev[size], size, CFG_S3FD["variance"], self.conf_thresh, self.nms_thresh,
                                       self.nms_top_k, self.top_k, self.threshold)

    def __call__(self, image, rgb: bool = True) -> np.ndarray:
        """image u8 [H,W,3] -> detections [k,5] (float32)."""
        img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        rows, cnt = self._rows(img[None], rgb)
        k = int(cnt[0])
        return rows[0, :k].cpu().numpy() if k else np.empty((0, 5), dtype=np.float32)

    def batch(self, frames, rgb: bool = False) -> List[np.ndarray]:
        """frames u8 [T,H,W,3] -> one [k,5] array per frame; the network and the post-processing run once over the batch, and only
        the kept rows cross to the host, through a page-locked buffer (as in FaceDetections.batch)."""
        x = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        rows, cnt = self._rows(x, rgb)
        cnt = cnt.cpu().numpy()
        most = int(cnt.max()) if len(cnt) else 0
        if not most:
            return [np.empty((0, 5), dtype=np.float32) for _ in range(len(cnt))]
        host = torch.empty((int(rows.shape[0]), most, 5), dtype=torch.float32, pin_memory=True)
        host.copy_(rows[:, :most], non_blocking=True)
        torch.cuda.current_stream(rows.device).synchronize()
        rows = host.numpy()
        return [rows[t, :int(cnt[t])] if cnt[t] else np.empty((0, 5), dtype=np.float32) for t in range(len(cnt))]


_X_COLS, _Y_COLS = (0, 2, 5, 7, 9, 11, 13), (1, 3, 6, 8, 10, 12, 14)  # box corners, then the five landmarks of a [k,15] row


def check_detect_size(detect_size, detect_filter="bilinear", detector=None, detections=None, frame_size=None):
    """The `detect_size` / `detect_filter` options of run_inference, run_inference_file and run_dataset, checked before any work:
    None, (height, width) or an int (the longest side) -- anything else is a ValueError, as are a filter other than resize.FILTERS, a
    `detect_size` beside given `detections` with no detector (nothing would use it), and, once the frame size is known
    (`frame_size` = (H, W)), a target larger than the frames on either side."""
    from .resize import check_filter, target_size

    check_filter(detect_filter)
    if detect_size is None:
        return
    target_size(1, 1, detect_size)  # the value's form alone
    if detector is None and detections is not None:
        raise ValueError("detect_size is given with detections= and no detector: nothing would use it")
    if frame_size is not None:
        ScaledDetector.plan(int(frame_size[0]), int(frame_size[1]), detect_size)


def scaled_detector(detector, detect_size, detect_filter="bilinear"):
    """`detector` as the entry points use it: itself for detect_size=None (no wrapper is constructed) or without a detector."""
    return detector if detect_size is None or detector is None else ScaledDetector(detector, detect_size, detect_filter)


class ScaledDetector:
    """A detector run on a smaller copy of the frames: `ScaledDetector(detector, size, filter="bilinear")` wraps a
    RetinaFacePredictor (either network) or an S3FDPredictor and offers what the call sites use -- `batch`, `__call__`, `kind`,
    `gflop_per_frame`.  The batch is resized on the device (resize.resize_frames: PIL's Image.resize, bit for bit), the inner
    detector runs on the copy, and every row is mapped back to source pixels, so tracker, crop rectangles and crops work on
    full-resolution coordinates and the crops come from the full-resolution frames.  This departs from the reference on purpose
    (data/get_face_images.py:50 detects on whole frames) and is off unless asked for.

    `size`: (height, width), or an int n = the longest side: h2 = max(1, int(H * n / max(H, W) + 0.5)), likewise w2.  A target that
    shrinks neither side -- the frames' own size, an int >= their longest side -- passes the frames straight to the inner detector:
    the identical call, the identical arrays.  A target larger than the frames on one side and not equal on the other is refused
    with ValueError: upscaling for detection is not offered.
    Mapping: sx = float32(W) / float32(w2), sy = float32(H) / float32(h2); columns 0, 2 (and 5, 7, 9, 11, 13 of a [k,15] row) are
    multiplied by sx, columns 1, 3 (and 6, 8, 10, 12, 14) by sy, in float32; the score is untouched.
    `kind` is 0 (a wrapper; `inner.kind` is the network's), so run_dataset prices it by `gflop_per_frame`: the inner detector's
    figure times (h2 * w2) / (H * W) of the last frame size seen (`gflop_at(H, W)` for any other), which dist.video_cost multiplies
    by H * W / (640 * 360) again."""

    kind = 0

    def __init__(self, detector, size, filter: str = "bilinear"):
        from .resize import check_filter, target_size

        target_size(1, 1, size)
        self.inner, self.size, self.filter = detector, size, check_filter(filter)
        self.engine = detector.engine
        self._last = None  # (H, W) of the last frames seen

    @staticmethod
    def plan(height: int, width: int, size):
        """(h2, w2) for frames of height x width, or None where the frames pass straight through; ValueError for an upscale."""
        from .resize import target_size

        h2, w2 = target_size(height, width, size)
        if h2 >= height and w2 >= width and (isinstance(size, (int, np.integer)) or (h2, w2) == (height, width)):
            return None
        if h2 > height or w2 > width:
            raise ValueError(f"detect size {h2} x {w2} (height x width) is larger than the {height} x {width} frames: upscaling for "
                             "detection is not offered")
        return h2, w2

    def gflop_at(self, height: int, width: int) -> float:
        """The wrapper's price per frame of height x width in dist.video_cost's unit (GFLOP per 640 x 360 frame of the SOURCE)."""
        t = self.plan(int(height), int(width), self.size)
        g = float(self.inner.gflop_per_frame)
        return g if t is None else g * (t[0] * t[1]) / (int(height) * int(width))

    @property
    def gflop_per_frame(self) -> float:
        return float(self.inner.gflop_per_frame) if self._last is None else self.gflop_at(*self._last)

    def _map(self, rows: np.ndarray, h: int, w: int, h2: int, w2: int) -> np.ndarray:
        rows = np.array(rows, dtype=np.float32)  # a copy: the inner arrays may be views of a shared host buffer
        sx, sy = np.float32(w) / np.float32(w2), np.float32(h) / np.float32(h2)
        nx = [c for c in _X_COLS if c < rows.shape[1]]
        ny = [c for c in _Y_COLS if c < rows.shape[1]]
        rows[:, nx] *= sx
        rows[:, ny] *= sy
        return rows

    def batch(self, frames, rgb: bool = False):
        """frames u8 [T,H,W,3] -> one array per frame, of the inner detector's width, in source pixels."""
        x = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        h, w = int(x.shape[1]), int(x.shape[2])
        t = self.plan(h, w, self.size)
        self._last = (h, w)
        if t is None:
            return self.inner.batch(frames, rgb=rgb)
        small = self.engine.resize_frames(x.to(self.engine.device).contiguous(), t, self.filter)
        return [self._map(r, h, w, *t) for r in self.inner.batch(small, rgb=rgb)]

    def __call__(self, image, rgb: bool = True):
        """image u8 [H,W,3] -> the inner detector's array, in source pixels."""
        img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        h, w = int(img.shape[0]), int(img.shape[1])
        t = self.plan(h, w, self.size)
        self._last = (h, w)
        if t is None:
            return self.inner(image, rgb=rgb)
        small = self.engine.resize_frames(img[None].to(self.engine.device).contiguous(), t, self.filter)
        return self._map(self.inner(small[0], rgb=rgb), h, w, *t)


class SimpleFaceTracker:
    """IoU + Hungarian face tracker; ids start at 1, a frame without faces drops every tracklet."""

    def __init__(self, iou_threshold: float = 0.4, minimum_face_size: float = 0.0) -> None:
        self.iou_threshold = iou_threshold
        self.minimum_face_size = minimum_face_size
        self.reset()

    def reset(self, reset_tracklet_counter: bool = True) -> None:
        self._boxes = np.zeros((0, 4), dtype=np.float32)
        self._areas = np.zeros((0,), dtype=np.float32)
        self._ids: List[int] = []
        if reset_tracklet_counter:
            self._counter = 0

    def __call__(self, face_boxes: np.ndarray) -> List[Optional[int]]:
        if face_boxes.size <= 0:
            self.reset(False)
            return []
        fb = face_boxes[:, :4]
        areas = np.abs((fb[:, 2] - fb[:, 0]) * (fb[:, 3] - fb[:, 1]))
        thr = float(np.clip(1.0 - self.iou_threshold, 0.0, 1.0))
        big = areas >= max(self.minimum_face_size ** 2, np.finfo(float).eps)
        n, m = len(fb), len(self._ids)
        dist = np.full((n, m), 2.0 * min(n, m), dtype=float)
        if m:
            tb = self._boxes
            xl = np.maximum(np.minimum(fb[:, 0], fb[:, 2])[:, None], np.minimum(tb[:, 0], tb[:, 2])[None])
            yt = np.maximum(np.minimum(fb[:, 1], fb[:, 3])[:, None], np.minimum(tb[:, 1], tb[:, 3])[None])
            xr = np.minimum(np.maximum(fb[:, 0], fb[:, 2])[:, None], np.maximum(tb[:, 0], tb[:, 2])[None])
            yb = np.minimum(np.maximum(fb[:, 1], fb[:, 3])[:, None], np.maximum(tb[:, 1], tb[:, 3])[None])
            inter = (xr - xl) * (yb - yt)                                    # dtype of the boxes, like the scalars there
            union = (areas[:, None] + self._areas[None]) - inter
            # evaluated in the boxes' dtype: `1.0 - f32 / float(f32)` is float32 under NumPy >= 2 (weak Python scalars);
            # NumPy 1.x made the last two operations float64, a < 1e-7 difference that only matters for exact ties
            with np.errstate(divide="ignore", invalid="ignore"):
                d = (1.0 - inter / union).astype(float)
            d = np.where((xr <= xl) | (yb <= yt), 1.0, d)
            ok = (d <= thr) & big[:, None]
            dist[ok] = d[ok]
        ids: List[Optional[int]] = [None] * n
        tracked = np.zeros(m, dtype=bool)
        boxes, tareas = self._boxes.copy(), self._areas.copy()
        for r, c in zip(*linear_sum_assignment(dist)):
            if dist[r, c] <= thr:
                ids[r] = self._ids[c]
                boxes[c], tareas[c], tracked[c] = fb[r], areas[r], True
        new = [r for r in range(n) if big[r] and ids[r] is None]
        for r in new:
            self._counter += 1
            ids[r] = self._counter
        self._boxes = np.concatenate([boxes[tracked], fb[new].astype(boxes.dtype)]) if m or new else boxes
        self._areas = np.concatenate([tareas[tracked], areas[new].astype(tareas.dtype)])
        self._ids = [i for i, t in zip(self._ids, tracked) if t] + [ids[r] for r in new]
        return ids


def crop_rects(dets: np.ndarray, w: int, h: int) -> np.ndarray:
    """Box corners -> the half-open pixel rectangle `fr[y0:y1, x0:x1]` the reference crops (truncate toward zero, clamp
    the start to 0 and the end to size-1, then numpy's slice rules).  [k,>=4] float -> [k,4] int (x0, y0, x1, y1)."""
    b = np.asarray(dets)[:, :4].astype(int)
    out = np.empty((len(b), 4), dtype=np.int64)
    for k, (sx, sy, ex, ey) in enumerate(b):
        x0, x1, _ = slice(max(0, int(sx)), min(w - 1, int(ex))).indices(w)
        y0, y1, _ = slice(max(0, int(sy)), min(h - 1, int(ey))).indices(h)
        out[k] = (x0, y0, max(x0, x1), max(y0, y1))
    return out


class VideoTiler:
    """`VideoPredictor.process` with the decoded frames and the per-frame detections already in memory: tracks the
    faces and cuts every detection into a 224x224 RGB tile on the GPU.  Returns per write, in the reference's order:
    records int64 [n,6] = frame index, track directory (tid-1), x0, y0, x1, y1; and the tiles u8 [n,224,224,3] (device)."""

    def __init__(self, engine):
        self.engine = engine
        self.face_tracker = SimpleFaceTracker(iou_threshold=0.4, minimum_face_size=0.0)

    def process(self, frames_bgr, dets_per_frame: Sequence[np.ndarray], save_path: Optional[str] = None, video_name: Optional[str] = None,
                entropy: str = "host", via_jpeg: bool = False):
        """`save_path` and `video_name` given: the crops are also written as the reference's face folders (write_face_crops, which
        takes `entropy`).
        `via_jpeg`: the tiles are what stage 1 of the reference reads back from those files (jpeg.roundtrip_tiles on the same
        half-open rectangles, BGR in, quality 95, 4:2:0) instead of the raw crops; files asked for in the same call are packed
        from that pass's coefficients.  Anything but a bool raises ValueError before any work."""
        check_via_jpeg(via_jpeg)
        if (save_path is None) != (video_name is None):
            raise ValueError("give both save_path and video_name, or neither")
        frames = frames_bgr if torch.is_tensor(frames_bgr) else torch.from_numpy(np.ascontiguousarray(frames_bgr))
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError("frames must be uint8 [T,H,W,3] (BGR, as cv2 decodes them)")
        t_total, h, w = (int(v) for v in frames.shape[:3])
        if len(dets_per_frame) != t_total:
            raise ValueError("one detection array per frame")
        # tracker + crop rectangles of the whole video in ONE native host call (csrc/track.hip: the arithmetic of SimpleFaceTracker
        # above and of crop_rects, scipy's assignment algorithm): the 750 Python iterations this replaces took 25-30 ms per 30 s
        # video, with the visual branch's stream idle behind them
        records = self.engine.track_faces(dets_per_frame, w, h, self.face_tracker.iou_threshold, self.face_tracker.minimum_face_size)
        if not len(records):
            return records, torch.zeros((0, 224, 224, 3), dtype=torch.uint8, device=self.engine.device)
        if via_jpeg:
            return records, roundtrip_face_tiles(self.engine, frames, records, save_path, video_name, entropy=entropy)[0]
        rects = torch.from_numpy(records[:, [0, 2, 3, 4, 5]].astype(np.int32))
        if save_path is not None:
            frames = frames.to(self.engine.device)  # one copy for both consumers
            write_face_crops(self.engine, frames, records, save_path, video_name, entropy=entropy)
        return records, self.engine.crop_tiles(frames, rects, bgr=True)


def check_via_jpeg(value) -> None:
    """The `via_jpeg` / `faces_via_jpeg` option is a bool; anything else is a ValueError (before any work, at every entry point)."""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"faces_via_jpeg / via_jpeg must be True or False, not {value!r}")


def check_tracks(tracks, flag_heatmaps: bool = False):
    """The `tracks` option of run_inference / run_inference_file / annotate.write_result_video -> None, "all" or a tuple of ints.
    None: track directory 00 alone, the reference's walk (get_prob_video.py:79-94).  "all": every track directory stage 0 writes.
    A list / tuple / array of distinct non-negative ints: those track directories (tid - 1, the folder numbers), in that order.
    Anything else -- another string, an empty list, a bool, a float, a negative, a repeat -- is a ValueError before any work, and so
    is `flag_heatmaps` beside it: heat maps are drawn for track 00 alone."""
    if tracks is None:
        return None
    if flag_heatmaps:
        raise ValueError("flag_heatmaps and tracks cannot be combined: heat maps are made for track 00 only (tracks=None)")
    if isinstance(tracks, str):
        if tracks != "all":
            raise ValueError(f'tracks must be None, "all" or a list of track numbers, not {tracks!r}')
        return "all"
    if not isinstance(tracks, (list, tuple, np.ndarray)) or np.ndim(tracks) != 1 or len(tracks) == 0:
        raise ValueError(f'tracks must be None, "all" or a non-empty list of track numbers, not {tracks!r}')
    for k in tracks:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"tracks: {k!r} is not a track number (an int >= 0)")
    out = tuple(int(k) for k in tracks)
    if len(set(out)) != len(out):
        raise ValueError(f"tracks: a track is named twice in {list(out)}")
    return out


def select_tracks(records: np.ndarray, tracks):
    """`tracks` as check_tracks returns it -> the tuple of track directories it means for these records: "all" = every distinct
    records[:, 1], ascending.  A named track without a record, or "all" without any record, is the FileNotFoundError the reference's
    os.listdir of that folder raises (get_prob_video.py:79)."""
    have = sorted({int(t) for t in np.asarray(records).reshape(-1, 6)[:, 1]})
    if isinstance(tracks, str):
        if not have:
            raise FileNotFoundError("no face track (os.listdir(<faces>/00) fails in the reference, get_prob_video.py:79)")
        return tuple(have)
    for k in tracks:
        if k not in have:
            raise FileNotFoundError(f"no face track {k:02d} (os.listdir(<faces>/{k:02d}) fails, as in get_prob_video.py:79); the tracks are "
                                    f"{', '.join('%02d' % t for t in have) or 'none'}")
    return tuple(tracks)


def face_crop_paths(records: np.ndarray, save_path: str, video_name: str) -> List[str]:
    """get_face_images.py:58-60: `<save_path>/<video_name>/<track:02d>/<frame:06d>.jpg` of every record, in record order."""
    return [os.path.join(save_path, video_name, str(int(t)).zfill(2), str(int(f)).zfill(6) + ".jpg") for f, t in records[:, :2]]


def _write_files(paths: List[str], blobs) -> None:
    for folder in sorted({os.path.dirname(p) for p in paths}):
        os.makedirs(folder, exist_ok=True)
    for p, blob in zip(paths, blobs):
        with open(p, "wb") as f:
            f.write(blob)


def write_face_crops(engine, frames_bgr, records: np.ndarray, save_path: str, video_name: str, quality: int = 95,
                     entropy: str = "host", frame_base: int = 0) -> List[str]:
    """Stage 0's face folders (`VideoPredictor.process`, get_face_images.py:52-63): for every record of `VideoTiler.process` the
    half-open crop `fr[y0:y1, x0:x1]` of its frame, written where the reference's cv2.imwrite writes it (JPEG quality 95, 4:2:0:
    cv2's defaults).  The crops are encoded straight out of the BGR frames on the device (jpeg.encode_images); no crop and no
    frame is copied to the host.  `entropy`: where the Huffman coding runs, "host" or "device" (jpeg.encode_images; the files are the
    same).  `frame_base`: `frames_bgr` is one pass of a longer video and holds its frames from that index on; the records (and the
    file names) keep the video's own frame index.  Returns the paths in record order."""
    from . import jpeg

    records = np.asarray(records).reshape(-1, 6)
    paths = face_crop_paths(records, save_path, video_name)
    if not paths:
        return paths
    blobs = jpeg.encode_images(engine, frames_bgr, pass_rects(records, frame_base), bgr=True, quality=quality, subsampling=2, entropy=entropy)
    _write_files(paths, blobs)
    return paths


def pass_rects(records: np.ndarray, frame_base: int = 0) -> np.ndarray:
    """records [n,6] -> the kernels' rectangles int64 [n,5] = (frame - frame_base, x0, y0, x1, y1): the frame index rebased to a pass
    that starts at frame `frame_base` of the video."""
    rects = np.asarray(records).reshape(-1, 6)[:, [0, 2, 3, 4, 5]].copy()
    rects[:, 0] -= int(frame_base)
    return rects


def track_pass(tracker, frames, frame_base: int, width: int, height: int, detector=None, detections=None) -> np.ndarray:
    """Stage 0 of one frame pass, stated once for run._run and for dataset's streamed jobs: the detector on the pass's frames (or the
    pass's slice of the video's given `detections`) -> the resumable tracker (Engine.tracker) -> the pass's records, their frame
    index counted over the whole video.  `frame_base`: the video's frame the pass starts at."""
    dets = detections[frame_base:frame_base + int(frames.shape[0])] if detections is not None else detector.batch(frames, rgb=False)
    return tracker.push(dets, width, height)


def pass_tiles(engine, frames_bgr, records: np.ndarray, frame_base: int = 0, via_jpeg: bool = False):
    """The tiles of `records` cut from the frames of the pass that starts at frame `frame_base`: u8 [n,224,224,3] RGB on the device, in
    record order -- the raw crops, or with `via_jpeg` what reading stage 0's files back gives (roundtrip_face_tiles, no file written)."""
    if via_jpeg:
        return roundtrip_face_tiles(engine, frames_bgr, records, frame_base=frame_base)[0]
    return engine.crop_tiles(frames_bgr, torch.from_numpy(pass_rects(records, frame_base).astype(np.int32)), bgr=True)


def roundtrip_face_tiles(engine, frames_bgr, records: np.ndarray, save_path: Optional[str] = None, video_name: Optional[str] = None,
                         quality: int = 95, entropy: str = "host", frame_base: int = 0):
    """The tiles of `records` as the reference's stage 1 reads them back from stage 0's files (jpeg.roundtrip_tiles: the rectangles
    of write_face_crops, BGR in, 4:2:0) -> (tiles u8 [n,224,224,3] RGB on the device, the paths written or None).  With `save_path`
    and `video_name` the files of write_face_crops are written too, packed from the coefficients of the same pass: no second forward
    pass runs.  `frame_base`: as in write_face_crops."""
    from . import jpeg

    jpeg._check_entropy(entropy)
    records = np.asarray(records).reshape(-1, 6)
    rects = pass_rects(records, frame_base)
    if save_path is None or not len(records):
        return jpeg.roundtrip_tiles(engine, frames_bgr, rects, bgr=True, quality=quality, subsampling=2), None
    tiles, coeffs, d_dev, desc = jpeg.roundtrip_tiles(engine, frames_bgr, rects, bgr=True, quality=quality, subsampling=2, keep_coeffs=True)
    paths = face_crop_paths(records, save_path, video_name)
    _write_files(paths, jpeg.files_from_coeffs(engine, coeffs, d_dev, desc, entropy=entropy))
    return tiles, paths


def track_clip(records: np.ndarray, tiles: torch.Tensor, track: int, total_frames: int):
    """One track directory as `video_pipeline.visual_forward(frames, present, fps)` consumes it: frames u8
    [total_frames,224,224,3] with the track's tiles at their frame indices (other frames zero, never read) and the
    present mask -- the listing `preprocess_video_and_predict` walks, get_prob_video.py:79-90."""
    rows = np.where(records[:, 1] == track)[0]
    present = np.zeros(total_frames, dtype=bool)
    present[records[rows, 0]] = True
    frames = torch.zeros((total_frames, 224, 224, 3), dtype=torch.uint8, device=tiles.device)
    if len(rows):
        frames[torch.from_numpy(records[rows, 0]).to(tiles.device)] = tiles[torch.from_numpy(rows).to(tiles.device)]
    return frames, present
