"""Thin object wrapper over the C ABI: one Engine = one avcer_ctx on one GPU.

torch is used for device memory (tensor.data_ptr()) and the current HIP stream only; every arithmetic step of
the hot path runs inside libavcer_hip.so.  All methods raise AvcerError on a non-zero return code.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib, packing
from ._lib import SPLIT_TRAILER, AvcerError, ConvDesc
from .jpeg import DESC as _JPEG_DESC

MODE_FP32 = 0    # exact f32 FMA chains on the f32 MFMA: the reference's own arithmetic, a third of the speed
MODE_BF16 = 1    # plain bf16 operands: throughput only, misses the 1e-4 parity gate
MODE_F16X3 = 2   # fp16 hi/lo operand pairs, 3 MFMAs per product: f32-grade results (include/avcer_hip.h)
# What every host mirror runs unless told otherwise.  Both parity-grade modes sit at the same distance from the reference's
# CPU path (worst |dprob| 1.6e-5 / 1.5e-5 at 8 x the synthetic logit scale, tests/test_gpu_parity_breadth.py); the fast one
# is the default, MODE_FP32 stays for checkpoints whose activations leave fp16's range (|x| >= 65504 -> NaN outputs).
MODE_DEFAULT = MODE_F16X3
PAD_MODES = {"mean": 0, "constant": 1, "repeat": 2}
_JPEG_DESC_BYTES = _JPEG_DESC.itemsize  # sizeof(struct avcer_jpeg_desc): jpeg.DESC is its one statement on this side


EVAL_MAX_ROWS = 1 << 28  # include/avcer_hip.h AVCER_EVAL_MAX_ROWS


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pack_detections(dets_per_frame):
    """Per-frame detection arrays [k, >= 4] -> (boxes f32 [max(total, 1), 4] back to back, counts i32 [frames], an int64 record
    buffer [max(total, 1), 6]): the host arguments of avcer_track_faces / avcer_tracker_push."""
    counts = np.fromiter((len(d) for d in dets_per_frame), dtype=np.int32, count=len(dets_per_frame))
    total = int(counts.sum())
    boxes = np.zeros((max(total, 1), 4), dtype=np.float32)
    if total:
        np.concatenate([np.asarray(d, dtype=np.float32).reshape(len(d), -1)[:, :4] for d in dets_per_frame if len(d)], out=boxes[:total])
    return boxes, counts, np.empty((max(total, 1), 6), dtype=np.int64)


class FaceTracker:
    """The face tracker behind a handle (include/avcer_hip.h avcer_tracker_*; host code, no device): the live tracklets, the
    tracklet counter and the effect of an empty frame are carried from one `push` to the next, so a video pushed in pieces of any
    size gives the records of `Engine.track_faces` on the whole.  `lib`: the loaded library (Engine.tracker() passes its own).
    `frames`: how many frames have been pushed, the index the next push starts at."""

    def __init__(self, lib, iou_threshold: float = 0.4, minimum_face_size: float = 0.0):
        self.lib, self.frames = lib, 0
        self._h = lib.avcer_tracker_create(float(iou_threshold), float(minimum_face_size))
        if not self._h:
            raise MemoryError("avcer_tracker_create failed")

    def push(self, dets_per_frame, frame_w: int, frame_h: int) -> np.ndarray:
        """The next len(dets_per_frame) frames -> their records int64 [n, 6] = frame (of the whole video), track directory, x0, y0,
        x1, y1.  ValueError naming the frame where the reference raises (zero-area detection, empty crop); the tracker takes no
        push after that."""
        if not self._h:
            raise ValueError("the tracker is closed")
        boxes, counts, rec = _pack_detections(dets_per_frame)
        n = C.c_int64(0)
        rc = self.lib.avcer_tracker_push(self._h, boxes.ctypes.data_as(C.c_void_p), 4, counts.ctypes.data_as(C.c_void_p), len(counts),
                                         self.frames, int(frame_w), int(frame_h), rec.ctypes.data_as(C.c_void_p), C.byref(n))
        if rc != 0:
            raise ValueError(self.lib.avcer_tracker_last_error(self._h).decode("utf-8", "replace"))
        self.frames += len(counts)
        return rec[:int(n.value)]

    def close(self):
        if getattr(self, "_h", None):
            self.lib.avcer_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SideBranch:
    """What Engine.side_branch hands out: the side stream, and the tensors named as its results."""

    def __init__(self, stream):
        self.stream, self.named = stream, []

    def results(self, *tensors):
        self.named.extend(tensors)


_LIVE = {}  # device index -> weak references to the engines created for it, oldest first (Engine.live)


class Engine:
    @staticmethod
    def live(device: int | None = None):
        """The youngest engine of `device` (default: torch's current device) that is still alive, for code that is called without
        one (a dataset.VideoJob's load); RuntimeError when there is none."""
        device = torch.cuda.current_device() if device is None else int(device)
        refs = _LIVE.get(device, [])
        refs[:] = [r for r in refs if r() is not None]
        if not refs:
            raise RuntimeError(f"no Engine is alive for device {device}")
        return refs[-1]()

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("avcer_amd needs a ROCm GPU (gfx950); there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)  # make sure the primary context exists before the library uses it
        ctx = _lib.c_ctx()
        rc = self.lib.avcer_ctx_create(device, C.byref(ctx))
        if rc != 0:
            raise AvcerError(rc, "avcer_ctx_create failed")
        self.ctx = ctx
        _LIVE.setdefault(int(device), []).append(weakref.ref(self))
        self.audio_classes = 0
        self.x3_fallbacks = 0  # calls `guarded` had to repeat in MODE_FP32 (the x3 range contract was broken)
        self._resample_cache = {}  # (orig_freq, new_freq) -> (plan, taps [span, n] and first [n] on the device): Engine.resample
        self._side_stream = None   # Engine.side_branch creates it on first use
        self._resize_cache = {}    # (in, out, filter) -> (plan, its packed table on the host and on the device): Engine.resize_frames

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.avcer_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _check(self, rc: int):
        if rc != 0:
            raise AvcerError(rc, self.lib.avcer_last_error(self.ctx).decode("utf-8", "replace"))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t, dtype):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------ x3 range contract
    def x3_overflow_count(self, reset: bool = True) -> int:
        """How many GPU threads have turned a finite activation of magnitude >= 65520 into an infinite fp16 half since the
        last reset (include/avcer_hip.h avcer_x3_overflow_count).  Waits for the current stream."""
        n = C.c_int64(0)
        self._check(self.lib.avcer_x3_overflow_count(self.ctx, int(reset), C.byref(n), self._stream()))
        return int(n.value)

    def x3_overflow_clear(self):
        """Asynchronous reset of the range-contract counter, in stream order on the current stream (no wait)."""
        self._check(self.lib.avcer_x3_overflow_count(self.ctx, 1, None, self._stream()))

    def guarded(self, mode: int, call):
        """`call(mode)` with the x3 mode's range contract enforced.  `guarded` OWNS the counter for the duration of the call: in
        MODE_F16X3 it is cleared in stream order in front of the call (counts left behind by earlier unguarded kernel-level
        calls, by a call that raised or by abandoned side-stream work are not charged to this one), read ONCE behind it -- the
        read waits for the current stream, so `call` must have joined any side stream it used -- and, when an activation left
        fp16's range, the same call is repeated in MODE_FP32 (no range limit; a fresh call on the same context).  What comes
        back is then what the reference's fp32 path computes -- NaN only where the input was NaN (the empty audio window).
        Other modes pass through.  Cost: one host synchronisation per guarded call."""
        if mode != MODE_F16X3:
            return call(mode)
        self.x3_overflow_clear()
        out = call(mode)
        if self.x3_overflow_count(reset=True):
            self.x3_fallbacks += 1
            out = call(MODE_FP32)
        return out

    # ------------------------------------------------------------------ the audio branch beside the visual one
    @contextlib.contextmanager
    def side_branch(self, *inputs):
        """Work beside the current stream, on the engine's ONE side stream (created here, on first use): the audio branch depends on
        nothing of the visual one and runs there while the caller's stream (and the host: tracker, plans) goes on.
            with engine.side_branch(wav) as side:
                with torch.cuda.stream(side.stream):
                    logits = ...          # queued on the side stream
                side.results(logits)      # what the caller's stream reads behind the join
                ...                       # the visual branch, on the caller's stream
            # joined
        Entry forks the side stream from the current one; `inputs`, tensors allocated on the current stream, are record_stream'ed on
        the side stream (the allocator must not hand them out while it still reads them).  EVERY exit, an exception included, joins
        the side stream back and record_stream's the named results on the caller's stream: no launch queued here outlives the block
        -- the workspace and the range-contract counter belong to the next call (`guarded` reads the counter behind the join)."""
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(self.device)
        main, branch = torch.cuda.current_stream(self.device), _SideBranch(self._side_stream)
        branch.stream.wait_stream(main)
        for t in inputs:
            if torch.is_tensor(t) and t.is_cuda:  # a host input is copied by the kernel wrapper, on the stream that reads it
                t.record_stream(branch.stream)
        try:
            yield branch
        finally:
            main.wait_stream(branch.stream)
            for t in branch.named:
                t.record_stream(main)

    # ------------------------------------------------------------------ weights
    def _load(self, fn, tensors):
        blob = packing.to_blob(tensors)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._check(fn(self.ctx, C.cast(buf, C.c_void_p), len(blob)))

    def load_static(self, state_dict):
        self._load(self.lib.avcer_load_static, packing.pack_static(state_dict))

    def load_dynamic(self, state_dict):
        self._load(self.lib.avcer_load_dynamic, packing.pack_dynamic(state_dict))

    def load_audio(self, state_dict, max_tokens: int = packing.PE_ROWS):
        """`max_tokens`: the longest window this model will be asked for, in wav2vec2 tokens (one per 20 ms: 256 = 5.1 s, the
        default, up to 5000 = 100 s, the reference's own limit): that many rows of `pe` are packed, and the forward accepts
        windows up to it (avcer_set_audio_max_tokens).  Windows of at most 256 tokens give the same bits whatever it is."""
        self._load(self.lib.avcer_load_audio, packing.pack_audio(state_dict, pe_rows=max_tokens))
        self._check(self.lib.avcer_set_audio_max_tokens(self.ctx, int(max_tokens)))
        self.audio_classes = self.lib.avcer_audio_num_classes(self.ctx)

    @property
    def audio_max_tokens(self) -> int:
        """The longest audio window the loaded model accepts, in tokens (load_audio's max_tokens)."""
        return int(self.lib.avcer_audio_max_tokens(self.ctx))

    @property
    def audio_head_kind(self) -> int:
        """Head of the loaded audio model: 0 none, 1 the GRU of ExprModelV1, 3 the TransformerLayers of ExprModelV2 / V3."""
        return int(self.lib.avcer_audio_head_kind(self.ctx))

    def load_face(self, state_dict):
        """Any of the three detectors: RetinaFace(cfg_re50).state_dict(), RetinaFace(cfg_mnet).state_dict() or S3FDNet.state_dict()
        (packing.pack_face tells them apart)."""
        self._load(self.lib.avcer_load_face, packing.pack_face(state_dict))

    def face_kind(self) -> int:
        """The loaded detector: 0 none, 1 RetinaFace-R50, 2 RetinaFace-MobileNet-0.25, 3 S3FD."""
        return int(self.lib.avcer_face_kind(self.ctx))

    def face_forward(self, frames_u8, mode: int = MODE_DEFAULT, rgb: bool = False):
        """frames u8 [N,H,W,3] (BGR unless rgb) -> (loc [N,P,4], conf [N,P,2] softmaxed, landms [N,P,10]).  With the S3FD
        detector loaded (face_kind 3) P = avcer_s3fd_num_priors(h, w) and there are no landmarks: (loc, conf, None)."""
        x = self._dev(frames_u8, torch.uint8)
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"frames must be [N,H,W,3] uint8, got {tuple(x.shape)}")
        n, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        if self.face_kind() == 3:
            p = int(self.lib.avcer_s3fd_num_priors(h, w))
            loc, conf = self._new(n, p, 4), self._new(n, p, 2)
            self._check(self.lib.avcer_face_forward(self.ctx, _ptr(x), n, h, w, 1 if rgb else 0, mode, _ptr(loc), _ptr(conf), None,
                                                    self._stream()))
            return loc, conf, None
        p = int(self.lib.avcer_face_num_priors(h, w))
        loc, conf, lm = self._new(n, p, 4), self._new(n, p, 2), self._new(n, p, 10)
        self._check(self.lib.avcer_face_forward(self.ctx, _ptr(x), n, h, w, 1 if rgb else 0, mode, _ptr(loc), _ptr(conf),
                                                _ptr(lm), self._stream()))
        return loc, conf, lm

    def set_static_batch(self, frames: int, back: int | None = None):
        """Frames per front pass of the static CNN (1..1024) and, optionally, per back pass (1..2048; 0 = two front passes)."""
        self._check(self.lib.avcer_set_static_batch(self.ctx, int(frames)))
        if back is not None:
            self._check(self.lib.avcer_set_static_back_batch(self.ctx, int(back)))

    def set_static_lanes(self, lanes: int, min_frames: int | None = None, max_frames: int | None = None):
        """2 (default): mid-sized static-CNN calls run as two half-batches on two streams; 1: always serial.  min / max frames:
        the call sizes that take the two-lane schedule."""
        self._check(self.lib.avcer_set_static_lanes(self.ctx, int(lanes)))
        if min_frames is not None or max_frames is not None:
            self._check(self.lib.avcer_set_static_lane_range(self.ctx, int(min_frames or 128), int(max_frames or 512)))

    def set_skip_unread_rows(self, on: bool = True):
        """True (default): in the x3 mode the block in front of a strided last block of the recognition CNN stores only the output rows
        that block reads; False: every row.  Results are bit-identical either way."""
        self._check(self.lib.avcer_set_skip_unread_rows(self.ctx, 1 if on else 0))

    # ------------------------------------------------------------------ forward passes
    def static_forward(self, frames_u8, mode: int = MODE_DEFAULT):
        """frames u8 [N,H,W,3] RGB -> (logits [N,7], probs [N,7], feats [N,512] pre-ReLU)."""
        x = self._dev(frames_u8, torch.uint8)
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"frames must be [N,H,W,3] uint8, got {tuple(x.shape)}")
        n, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        logits, probs, feats = self._new(n, 7), self._new(n, 7), self._new(n, 512)
        self._check(self.lib.avcer_static_forward(self.ctx, _ptr(x), n, h, w, mode, _ptr(logits), _ptr(probs),
                                                  _ptr(feats), self._stream()))
        return logits, probs, feats

    def static_forward_cam(self, frames_u8, mode: int = MODE_DEFAULT):
        """`static_forward` plus the Grad-CAM maps of layer 4 for all 7 classes: (logits, probs, feats, cam [N,7,7,7]); cam is the
        raw map mean_c g_k[c] * A[c,y,x] before ReLU and normalisation (include/avcer_hip.h avcer_static_forward_cam)."""
        x = self._dev(frames_u8, torch.uint8)
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"frames must be [N,H,W,3] uint8, got {tuple(x.shape)}")
        n, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        logits, probs, feats, cam = self._new(n, 7), self._new(n, 7), self._new(n, 512), self._new(n, 7, 7, 7)
        self._check(self.lib.avcer_static_forward_cam(self.ctx, _ptr(x), n, h, w, mode, _ptr(logits), _ptr(probs), _ptr(feats),
                                                      _ptr(cam), self._stream()))
        return logits, probs, feats, cam

    def static_forward_nchw(self, x, mode: int = MODE_DEFAULT):
        x = self._dev(x, torch.float32)
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224):
            raise ValueError(f"input must be [N,3,224,224] float32, got {tuple(x.shape)}")
        n = int(x.shape[0])
        logits, probs, feats = self._new(n, 7), self._new(n, 7), self._new(n, 512)
        self._check(self.lib.avcer_static_forward_nchw(self.ctx, _ptr(x), n, mode, _ptr(logits), _ptr(probs),
                                                       _ptr(feats), self._stream()))
        return logits, probs, feats

    def gather_windows(self, feats, idx, validated: bool = False):
        """`validated=True`: the caller built idx on the host and already checked its range (no device sync here)."""
        feats = self._dev(feats, torch.float32)
        if not validated and not (isinstance(idx, torch.Tensor) and idx.is_cuda):
            a = np.asarray(idx)
            if a.size and (a.min() < 0 or a.max() >= feats.shape[0]):
                raise ValueError("gather_windows: index out of range")
            validated = True
        idx = self._dev(idx, torch.int32)
        if idx.dim() != 2 or idx.shape[1] != 10 or feats.dim() != 2 or feats.shape[1] != 512:
            raise ValueError("gather_windows: feats [*,512], idx [nwin,10]")
        if not validated and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= feats.shape[0]):
            raise ValueError("gather_windows: index out of range")
        out = self._new(idx.shape[0], 10, 512)
        self._check(self.lib.avcer_gather_windows(self.ctx, _ptr(feats), _ptr(idx), int(idx.shape[0]), _ptr(out),
                                                  self._stream()))
        return out

    def dynamic_forward(self, windows, mode: int = MODE_DEFAULT):
        x = self._dev(windows, torch.float32)
        if x.dim() != 3 or tuple(x.shape[1:]) != (10, 512):
            raise ValueError(f"windows must be [N,10,512], got {tuple(x.shape)}")
        out = self._new(x.shape[0], 7)
        self._check(self.lib.avcer_dynamic_forward_mode(self.ctx, _ptr(x), int(x.shape[0]), int(mode), _ptr(out),
                                                        self._stream()))
        return out

    def audio_forward(self, wav, normalize: bool = True, mode: int = MODE_DEFAULT, return_features: bool = False):
        """wav [N,T] -> logits [N,C]; return_features: (logits, the pooled head activations [N, 256 (ExprModelV1) or 1024])."""
        x = self._dev(wav, torch.float32)
        if x.dim() != 2:
            raise ValueError(f"wav must be [N,T], got {tuple(x.shape)}")
        out = self._new(x.shape[0], self.audio_classes)
        if not return_features:
            self._check(self.lib.avcer_audio_forward(self.ctx, _ptr(x), int(x.shape[0]), int(x.shape[1]), int(normalize),
                                                     mode, _ptr(out), self._stream()))
            return out
        feats = self._new(x.shape[0], 256 if self.audio_head_kind == 1 else 1024)
        self._check(self.lib.avcer_audio_forward_features(self.ctx, _ptr(x), int(x.shape[0]), int(x.shape[1]), int(normalize),
                                                          mode, _ptr(out), _ptr(feats), self._stream()))
        return out, feats

    def gru_layer(self, xp, w_hh, b_hh, mode: int = MODE_DEFAULT):
        """One GRU layer's recurrence (avcer_gru_layer): xp [N,S,768] = x W_ih^T + b_ih, w_hh [768,256], b_hh [768] -> h [N,S,256]."""
        xp, w_hh, b_hh = self._dev(xp, torch.float32), self._dev(w_hh, torch.float32), self._dev(b_hh, torch.float32)
        if xp.dim() != 3 or xp.shape[2] != 768 or tuple(w_hh.shape) != (768, 256) or tuple(b_hh.shape) != (768,):
            raise ValueError("gru_layer: xp [N,S,768], w_hh [768,256], b_hh [768]")
        out = self._new(xp.shape[0], xp.shape[1], 256)
        self._check(self.lib.avcer_gru_layer(self.ctx, _ptr(xp), _ptr(w_hh), _ptr(b_hh), int(xp.shape[0]), int(xp.shape[1]), 256,
                                             int(mode), _ptr(out), self._stream()))
        return out

    def audio_chunks(self, wav, starts, ends, window: int, padding: str = "mean"):
        wav = self._dev(wav, torch.float32)
        # the ranges are validated on the HOST when they come from the host (chunk_spans builds them there): a device-side
        # `int(starts.min())` is a synchronisation in front of every launch of the audio branch
        if not (torch.is_tensor(starts) and starts.is_cuda) and not (torch.is_tensor(ends) and ends.is_cuda):
            hs = np.asarray(starts.cpu() if torch.is_tensor(starts) else starts).reshape(-1).astype(np.int64)
            he = np.asarray(ends.cpu() if torch.is_tensor(ends) else ends).reshape(-1).astype(np.int64)
            n = int(hs.size)
            if wav.dim() != 1 or he.size != n:
                raise ValueError("audio_chunks: wav [L], starts/ends [n]")
            if n and (hs.min() < 0 or he.max() > wav.numel() or (he < hs).any() or (he - hs).max() > window):
                raise ValueError("audio_chunks: sample ranges out of bounds")
            if padding == "repeat" and n and (he - hs).min() == 0:
                raise ZeroDivisionError("integer division or modulo by zero")  # data/utils.py:66 on an empty chunk
            starts = torch.from_numpy(hs.astype(np.int32)).to(self.device, non_blocking=True)
            ends = torch.from_numpy(he.astype(np.int32)).to(self.device, non_blocking=True)
        else:
            starts = self._dev(starts, torch.int32)
            ends = self._dev(ends, torch.int32)
            n = int(starts.numel())
            if wav.dim() != 1 or ends.numel() != n:
                raise ValueError("audio_chunks: wav [L], starts/ends [n]")
            if n and (int(starts.min()) < 0 or int(ends.max()) > wav.numel() or bool((ends < starts).any())
                      or int((ends - starts).max()) > window):
                raise ValueError("audio_chunks: sample ranges out of bounds")
            if padding == "repeat" and n and int((ends - starts).min()) == 0:
                raise ZeroDivisionError("integer division or modulo by zero")  # data/utils.py:66 on an empty chunk
        out = self._new(n, window)
        self._check(self.lib.avcer_audio_chunks(self.ctx, _ptr(wav), _ptr(starts), _ptr(ends), n, int(window),
                                                PAD_MODES[padding], _ptr(out), self._stream()))
        return out

    def resample(self, src, orig_freq: int, new_freq: int):
        """Source audio at `orig_freq` -> mono float32 [n_out] at `new_freq` on the device, n_out = ceil(L * new / orig) -- what
        data/utils.py:50-57 makes of a WAV file (int16 / 32768, channel mean, torchaudio's Resample), in one launch
        (include/avcer_hip.h avcer_resample).  src: int16 [L] or [L, C] (interleaved frames, as they lie in the file) or float32
        [L] or [C, L] (as torchaudio.load returns them), C <= 8; anything else raises ValueError, as do rates the kernel does
        not cover (audio_pipeline.resample_plan).  Equal rates: conversion and downmix alone (float32 mono comes back as it is).
        The tap table of a rate pair is built once per engine and stays on the device.  No host synchronisation."""
        from .audio_pipeline import resample_out_len, resample_plan

        if not isinstance(src, torch.Tensor):
            src = torch.as_tensor(np.asarray(src))
        if src.dtype == torch.int16 and src.dim() in (1, 2):
            kind, length, ch = 0, int(src.shape[0]), int(src.shape[1]) if src.dim() == 2 else 1
        elif src.dtype == torch.float32 and src.dim() in (1, 2):
            kind, length, ch = 1, int(src.shape[-1]), int(src.shape[0]) if src.dim() == 2 else 1
        else:
            raise ValueError(f"resample: source must be int16 [L] / [L, C] or float32 [L] / [C, L], got {src.dtype} {tuple(src.shape)}")
        if not 1 <= ch <= 8:
            raise ValueError(f"resample: {ch} channels (1..8)")
        if length > 2 ** 31 - 1:
            raise ValueError(f"resample: {length} samples per channel (the kernel takes 2^31 - 1)")
        if orig_freq == new_freq:
            resample_plan(orig_freq, new_freq)  # validates the rate
            if kind == 1 and ch == 1:
                return self._dev(src, torch.float32).reshape(-1)
            taps = first = None
            o = n = 1
            span = width = 0
        else:
            cache = self._resample_cache
            key = (int(orig_freq), int(new_freq))
            if key not in cache:
                plan = resample_plan(*key)
                cache[key] = (plan, self._dev(np.ascontiguousarray(plan.taps.T), torch.float32), self._dev(plan.first.copy(), torch.int32))
            plan, taps, first = cache[key]
            o, n, span, width = plan.o, plan.n, plan.span, plan.width
        n_out = resample_out_len(length, o, n)
        x = self._dev(src, src.dtype)
        out = self._new(n_out)
        if length:
            self._check(self.lib.avcer_resample(self.ctx, _ptr(x), kind, length, ch, _ptr(taps), _ptr(first), o, n, span, width,
                                                _ptr(out), n_out, self._stream()))
        return out

    def _resize_tables(self, in_size: int, out_size: int, filter: str):
        from .resize import resize_plan

        key = (int(in_size), int(out_size), filter)
        if key not in self._resize_cache:
            plan = resize_plan(*key)
            host = plan.packed()
            self._resize_cache[key] = (plan, host, torch.from_numpy(host).to(self.device))
        return self._resize_cache[key]

    def resize_form(self, in_h: int, out_h: int, filter: str = "bilinear") -> int:
        """The form avcer_resize_frames chooses for a vertical axis in_h -> out_h (resize.FORM_FUSED / FORM_TWO_PASS), from the
        table alone: nothing is launched."""
        _, host, _ = self._resize_tables(in_h, out_h, filter)
        rc = self.lib.avcer_resize_form(host.ctypes.data_as(C.c_void_p), int(out_h))
        if rc < 0:
            raise AvcerError(rc, "avcer_resize_form: bad table")
        return rc

    def resize_frames(self, frames, size, filter: str = "bilinear", form: int = 0, out=None):
        """frames u8 [n,H,W,3] on the device, contiguous -> u8 [n,h2,w2,3], size = (h2, w2): PIL's Image.resize((w2, h2), filter) of
        every frame, bit for bit, for "box", "bilinear", "bicubic" and "lanczos" (include/avcer_hip.h avcer_resize_frames; the CPU
        statement is resize.resize_numpy).  Sides 1..8192.  The tables of an axis are built once per engine and stay on the device.
        A batch that already has the size is returned as it is, with no launch (unless `out` is given, which is then filled).
        `form`: resize.FORM_CHOOSE, or FORM_FUSED / FORM_TWO_PASS by name (tests; the bits are the same).  `out`: a contiguous uint8
        [n,h2,w2,3] on the device to write into.  A wrong dtype, shape, device or layout, a side out of range and an unknown filter
        raise ValueError before any launch.  No host synchronisation."""
        from .resize import _check_size, check_filter

        check_filter(filter)
        h2, w2 = _check_size(size)
        if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3):
            raise ValueError("resize_frames: frames must be uint8 [n,H,W,3]")
        if not frames.is_cuda or frames.device != self.device:
            raise ValueError(f"resize_frames: frames must be on {self.device}")
        if not frames.is_contiguous():
            raise ValueError("resize_frames: frames must be contiguous")
        n, h, w = (int(v) for v in frames.shape[:3])
        _check_size((h, w))
        if form not in (0, 1, 2):
            raise ValueError(f"resize_frames: form {form!r}")
        if out is None:
            if (h, w) == (h2, w2):
                return frames
            out = self._new(n, h2, w2, 3, dtype=torch.uint8)
        elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and tuple(out.shape) == (n, h2, w2, 3) and out.is_contiguous() and
                  out.device == self.device):
            raise ValueError("resize_frames: out must be a contiguous uint8 [n,h2,w2,3] on the device")
        if n == 0:
            return out
        xp, xh, xd = self._resize_tables(w, w2, filter)
        yp, yh, yd = self._resize_tables(h, h2, filter)
        self._check(self.lib.avcer_resize_frames(self.ctx, _ptr(frames), n, h, w, _ptr(out), h2, w2, xh.ctypes.data_as(C.c_void_p), _ptr(xd),
                                                 xp.ksize, yh.ctypes.data_as(C.c_void_p), _ptr(yd), yp.ksize, int(form), self._stream()))
        return out

    def chart_path(self, T: int, pw: int) -> int:
        """How avcer_chart_series' envelope treats a chart of T frames on pw columns (chart.PATH_REDUCE / PATH_SEGMENT): nothing is
        launched."""
        rc = self.lib.avcer_chart_path(int(T), int(pw))
        if rc < 0:
            raise AvcerError(rc, f"avcer_chart_path: {T} frames on {pw} columns")
        return rc

    def chart_series(self, preds, plans, out, colours=None):
        """The traces of a batch of prediction charts (include/avcer_hip.h avcer_chart_series; the CPU statement is
        chart.series_numpy): preds int32 / int64 [S, sum T] on the device, contiguous, S <= 4 -- the class tables of the charts back
        to back --, plans: one chart.ChartPlan per chart, in that order (their T are the lengths); out uint8 [V, height, width, 3] on
        the device, contiguous, already holding the background: painted IN PLACE and returned.  colours: S RGB triples
        (chart.COLOURS).  A wrong dtype, shape, device or layout, and plans that do not fill the table, raise ValueError before any
        launch; the class values are the caller's to check (chart.render does; the kernel clamps).  No host synchronisation."""
        from . import chart as ch

        if not (torch.is_tensor(preds) and preds.dim() == 2 and preds.dtype in (torch.int32, torch.int64) and preds.is_contiguous() and
                preds.device == self.device):
            raise ValueError(f"chart_series: preds must be a contiguous int32 or int64 [S, sum T] on {self.device}")
        series, total = (int(v) for v in preds.shape)
        plans = list(plans)
        if not 1 <= series <= ch.MAX_SERIES:
            raise ValueError(f"chart_series: {series} series (1..{ch.MAX_SERIES})")
        if sum(p.T for p in plans) != total:
            raise ValueError(f"chart_series: plans of {[p.T for p in plans]} frames over a table of {total} columns")
        if not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.dim() == 4 and int(out.shape[0]) == len(plans) and
                out.shape[-1] == 3 and out.is_contiguous() and out.device == self.device):
            raise ValueError(f"chart_series: out must be a contiguous uint8 [{len(plans)},height,width,3] on {self.device}")
        h, w = int(out.shape[1]), int(out.shape[2])
        if any((p.height, p.width) != (h, w) for p in plans):
            raise ValueError(f"chart_series: a plan of another picture size than out's {w} x {h}")
        ink = np.ascontiguousarray(ch.COLOURS[:series] if colours is None else colours, dtype=np.uint8).reshape(-1)
        if ink.size != 3 * series:
            raise ValueError(f"chart_series: {series} RGB colours are needed")
        if not plans:
            return out
        offsets = np.cumsum([0] + [p.T for p in plans[:-1]])
        host = np.concatenate([p.record(int(o)) for p, o in zip(plans, offsets)])
        dev = torch.from_numpy(host.view(np.uint8)).to(self.device, non_blocking=True)
        self._check(self.lib.avcer_chart_series(self.ctx, _ptr(preds), preds.element_size(), series, total, host.ctypes.data_as(C.c_void_p),
                                                _ptr(dev), len(plans), _ptr(out), h, w, ink.ctypes.data_as(C.c_void_p), self._stream()))
        return out

    def weight_search_counts(self, preds, labels, weights):
        """Per-candidate argmax counts of the fusion weight search in one launch (include/avcer_hip.h
        avcer_weight_search_counts; data/utils.py:151-154, :176, :200).  preds [M, N, C] probability tables, labels [N],
        weights [W, M, C]; returns (tp, pred), int32 [W, C] on the device: how often candidate k's weighted sum picks class j
        and is right / picks class j.  Inputs are converted to float64 / int32 first -- numpy promotes a float32 table times a
        float64 weight the same way, so float32 tables give the reference's bits.  Shapes outside 1 <= M <= 4, 2 <= C <= 8,
        1 <= N < 2^31, 1 <= W <= 2^24 raise ValueError.  No host synchronisation."""
        p = self._dev(preds, torch.float64)
        wt = self._dev(weights, torch.float64)
        lab = self._dev(labels, torch.int32)
        if p.dim() != 3 or wt.dim() != 3 or lab.dim() != 1:
            raise ValueError(f"weight search: preds [M, N, C], labels [N], weights [W, M, C] expected, got {tuple(p.shape)}, "
                             f"{tuple(lab.shape)}, {tuple(wt.shape)}")
        m, n, c = (int(s) for s in p.shape)
        w = int(wt.shape[0])
        if tuple(wt.shape[1:]) != (m, c) or int(lab.shape[0]) != n:
            raise ValueError(f"weight search: preds {tuple(p.shape)}, labels {tuple(lab.shape)} and weights {tuple(wt.shape)} disagree")
        if not (1 <= m <= 4 and 2 <= c <= 8 and 1 <= n <= 2 ** 31 - 1 and 1 <= w <= 2 ** 24):
            raise ValueError(f"weight search: {m} models (1..4), {c} classes (2..8), {n} frames (1..2^31-1), {w} candidates (1..2^24)")
        tp = self._new(w, c, dtype=torch.int32)
        pred = self._new(w, c, dtype=torch.int32)
        self._check(self.lib.avcer_weight_search_counts(self.ctx, _ptr(p), _ptr(lab), n, m, c, _ptr(wt), w, _ptr(tp), _ptr(pred),
                                                        self._stream()))
        return tp, pred

    def eval_tables(self, rows, row_counts, need, need_counts, out_counts, softmax: bool, video_level: bool = False, keys=None,
                    key_lo=None, key_spans=None, out=None):
        """One model's tables of a whole file list (include/avcer_hip.h avcer_eval_tables; get_pred_av.py:77-195).  rows [R, c]
        (7 <= c <= 8): the videos' raw rows one behind the other; keys [R] (optional): each row's `frames` number, with key_lo /
        key_spans [V]: the first key value and the number of key values of each video's range; row_counts, need_counts,
        out_counts [V]: HOST integer arrays, the rows, kept positions and output rows per video; need: the videos' ascending
        kept positions one behind the other.  video_level: one output row per video (out_counts and need are ignored).
        Returns float64 [sum(out_counts), 7] on the device (`out`: write into this tensor instead).  Limits are the library's:
        AvcerError with code AVCER_EINVAL.  No host synchronisation."""
        x = self._dev(rows, torch.float64)
        if x.dim() != 2:
            raise ValueError(f"eval_tables: rows [R, c] expected, got {tuple(x.shape)}")
        counts = [np.asarray(row_counts, dtype=np.int64).reshape(-1)]
        nv = int(counts[0].shape[0])
        if video_level:
            counts += [np.zeros(nv, dtype=np.int64), np.ones(nv, dtype=np.int64)]
        else:
            counts += [np.asarray(a, dtype=np.int64).reshape(-1) for a in (need_counts, out_counts)]
        if any(a.shape[0] != nv for a in counts) or any((a < 0).any() for a in counts):
            raise ValueError("eval_tables: row_counts, need_counts and out_counts are one non-negative count per video")
        n_rows, n_need, n_out = (int(a.sum()) for a in counts)
        if n_rows != int(x.shape[0]):
            raise ValueError(f"eval_tables: {int(x.shape[0])} rows, row_counts sum to {n_rows}")
        nd = np.asarray([] if video_level else need, dtype=np.int64).reshape(-1)
        if nd.shape[0] != n_need:
            raise ValueError(f"eval_tables: {nd.shape[0]} kept positions, need_counts sum to {n_need}")
        n_slots = 0
        spans = np.zeros(nv, dtype=np.int64)
        if keys is not None:
            spans = np.asarray(key_spans, dtype=np.int64).reshape(-1)
            lo = np.asarray(key_lo, dtype=np.int64).reshape(-1)
            if spans.shape[0] != nv or lo.shape[0] != nv or (spans < 0).any():
                raise ValueError("eval_tables: key_lo and key_spans are one value per video")
            n_slots = int(spans.sum())
        sizes = (n_rows, n_need, n_out, n_slots)
        fits = max(sizes) <= EVAL_MAX_ROWS  # beyond it the library refuses the sizes themselves: nothing is read or allocated for them
        if fits:
            offs = np.zeros((4, nv + 1), dtype=np.int32)
            for i, a in enumerate(counts + [spans]):
                offs[i, 1:] = np.cumsum(a)
            packed = np.concatenate([offs.reshape(-1), (lo if keys is not None else spans).astype(np.int32), nd.astype(np.int32)])
        else:
            packed = np.zeros(5 * nv + 4, dtype=np.int32)
        dev = torch.from_numpy(packed).to(self.device, non_blocking=True)
        row_off, need_off, out_off, key_off = (dev[i * (nv + 1):(i + 1) * (nv + 1)] for i in range(4))
        klo, nd_dev = dev[4 * (nv + 1):5 * nv + 4], dev[5 * nv + 4:]
        k = None
        ws, ws_bytes = None, 0
        if keys is not None:
            k = self._dev(keys, torch.int32)
            if k.dim() != 1 or int(k.shape[0]) != n_rows:
                raise ValueError(f"eval_tables: {n_rows} rows, keys {tuple(k.shape)}")
            ws_bytes = int(self.lib.avcer_eval_tables_workspace(n_slots)) if fits else 0
            ws = self._new(max(ws_bytes, 8), dtype=torch.uint8)
        if out is None:
            out = self._new(n_out if fits else 0, 7, dtype=torch.float64)
        elif out.dtype != torch.float64 or tuple(out.shape) != (n_out, 7) or not out.is_contiguous():
            raise ValueError(f"eval_tables: out must be a contiguous float64 [{n_out}, 7]")
        self._check(self.lib.avcer_eval_tables(self.ctx, _ptr(x), _ptr(k), n_rows, int(x.shape[1]), _ptr(row_off), _ptr(klo), _ptr(key_off),
                                               n_slots, _ptr(nd_dev), n_need, _ptr(need_off), _ptr(out_off), nv, n_out, int(bool(softmax)),
                                               int(bool(video_level)), _ptr(out), _ptr(ws), ws_bytes, self._stream()))
        return out

    def eval_confusion(self, tables, labels=None, weights_1=None, weights_2=None, compound: int = 0, want_pred: bool = True,
                       want_cm: bool = True, pred=None, cm=None):
        """The prediction of a model or a fusion and its confusion matrix (include/avcer_hip.h avcer_eval_confusion;
        get_pred_av.py:35-45).  tables [m, N, 7], labels [N]; weights_1 [m, 7] and weights_2 [m] optional (ones).  compound: 0, or
        EVAL_COMPOUND with EVAL_CE_WEIGHTS / EVAL_CE_MASK for the compound-expression rule in front of the argmax.  Returns
        (pred int32 [N] or None, cm int64 [7, 7] or None) on the device.  No host synchronisation."""
        t = self._dev(tables, torch.float64)
        if t.dim() != 3 or t.shape[2] != 7:
            raise ValueError(f"eval_confusion: tables [m, N, 7] expected, got {tuple(t.shape)}")
        m, n = int(t.shape[0]), int(t.shape[1])
        lab = None
        if labels is not None:
            lab = self._dev(labels, torch.int32)
            if lab.dim() != 1 or int(lab.shape[0]) != n:
                raise ValueError(f"eval_confusion: {n} rows, labels {tuple(lab.shape)}")
        w1 = w2 = None
        if weights_1 is not None:
            w1 = np.ascontiguousarray(np.asarray(weights_1, dtype=np.float64))
            if w1.shape != (m, 7):
                raise ValueError(f"eval_confusion: weights_1 [{m}, 7] expected, got {w1.shape}")
        if weights_2 is not None:
            w2 = np.ascontiguousarray(np.asarray(weights_2, dtype=np.float64))
            if w2.shape != (m,):
                raise ValueError(f"eval_confusion: weights_2 [{m}] expected, got {w2.shape}")
        if pred is None and want_pred:
            pred = self._new(n, dtype=torch.int32)
        if cm is None and want_cm and lab is not None:
            cm = self._new(7, 7, dtype=torch.int64)
        self._check(self.lib.avcer_eval_confusion(self.ctx, _ptr(t), _ptr(lab), n, m, None if w1 is None else w1.ctypes.data_as(C.c_void_p),
                                                  None if w2 is None else w2.ctypes.data_as(C.c_void_p), int(compound), _ptr(pred), _ptr(cm),
                                                  self._stream()))
        return pred, cm

    def audio_frame_mean(self, win_logits, frame_lo, frame_hi, n_frames: int):
        x = self._dev(win_logits, torch.float32)
        lo, hi = self._dev(frame_lo, torch.int32), self._dev(frame_hi, torch.int32)
        out = self._new(n_frames, x.shape[1])
        cnt = self._new(n_frames, dtype=torch.int32)
        self._check(self.lib.avcer_audio_frame_mean(self.ctx, _ptr(x), _ptr(lo), _ptr(hi), int(x.shape[0]),
                                                    int(x.shape[1]), int(n_frames), _ptr(out), _ptr(cnt), self._stream()))
        return out, cnt

    def window_votes(self, logits, targets, file_off, out=None):
        """Softmax, argmax and the per-file majority vote of a corpus's window logits in one launch (include/avcer_hip.h
        avcer_window_votes; common_utils.py:74-108).  logits [n, c] (2 <= c <= 8), targets [n], file_off [F + 1]: a HOST integer
        array, the prefix offsets of the files' windows (0 first, ascending, n last).  Returns (probs f32 [n, c], pred i32 [n],
        file_pred i32 [F], file_target i32 [F], file_onehot i32 [F, c]) on the device (`out`: write into these five tensors instead).
        Shapes that disagree raise ValueError; limits are the library's (AvcerError).  No host synchronisation."""
        x = self._dev(logits, torch.float32)
        t = self._dev(targets, torch.int32)
        off = np.asarray(file_off, dtype=np.int64).reshape(-1)
        if x.dim() != 2 or t.dim() != 1 or int(t.shape[0]) != int(x.shape[0]):
            raise ValueError(f"window_votes: logits [n, c] and targets [n] expected, got {tuple(x.shape)} and {tuple(t.shape)}")
        n, c, nf = int(x.shape[0]), int(x.shape[1]), int(off.shape[0]) - 1
        if nf < 1 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
            raise ValueError(f"window_votes: file_off must ascend from 0 to {n} over at least one file")
        shapes = ((n, c), (n,), (nf,), (nf,), (nf, c))
        dtypes = (torch.float32,) + (torch.int32,) * 4
        if out is None:
            out = tuple(self._new(*s, dtype=d) for s, d in zip(shapes, dtypes))
        elif len(out) != 5 or any(tuple(o.shape) != s or o.dtype != d or not o.is_contiguous() for o, s, d in zip(out, shapes, dtypes)):
            raise ValueError(f"window_votes: out must be five contiguous tensors of shapes {shapes}")
        dev_off = torch.from_numpy(off.astype(np.int32)).to(self.device, non_blocking=True)
        self._check(self.lib.avcer_window_votes(self.ctx, _ptr(x), _ptr(t), _ptr(dev_off), n, c, nf, *(_ptr(o) for o in out),
                                                self._stream()))
        return tuple(out)

    def window_losses(self, logits, targets, weights=None, kind: int = 0, label_smoothing: float = 0.2, gamma: float = 0.0,
                      batch_size: int = 64):
        """The losses of a corpus's window logits, batched as a DataLoader batches them, in one launch (include/avcer_hip.h
        avcer_window_losses; net_trainer.py:391-465).  logits [n, c] (2 <= c <= 16), targets [n] in [0, c), weights [c] or None
        (ones); kind 0: cross entropy with `label_smoothing`, 1: soft focal loss with `gamma`.  Returns (row_loss f64 [n],
        batch_loss f64 [ceil(n / batch_size)], epoch f64 [2]: the reference's epoch loss and the row-weighted mean) on the device.
        Shapes that disagree raise ValueError; limits are the library's (AvcerError).  No host synchronisation."""
        x = self._dev(logits, torch.float32)
        t = self._dev(targets, torch.int32)
        if x.dim() != 2 or t.dim() != 1 or int(t.shape[0]) != int(x.shape[0]):
            raise ValueError(f"window_losses: logits [n, c] and targets [n] expected, got {tuple(x.shape)} and {tuple(t.shape)}")
        n, c, bsz = int(x.shape[0]), int(x.shape[1]), int(batch_size)
        w = None
        if weights is not None:
            w = self._dev(weights, torch.float32)
            if tuple(w.shape) != (c,):
                raise ValueError(f"window_losses: weights [{c}] expected, got {tuple(w.shape)}")
        n_batches = -(-n // bsz) if n > 0 and bsz > 0 else 0
        row, batch, epoch = (self._new(k, dtype=torch.float64) for k in (n, n_batches, 2))
        ticket = self._new(1, dtype=torch.int32)
        self._check(self.lib.avcer_window_losses(self.ctx, _ptr(x), _ptr(t), _ptr(w), n, c, int(kind), float(label_smoothing), float(gamma),
                                                 bsz, _ptr(row), _ptr(batch), _ptr(epoch), _ptr(ticket), self._stream()))
        return row, batch, epoch

    def wave_augment(self, chunks, recs, min_snr: float = 1e-4, max_snr: float = 5e-3, noise=None, return_std: bool = False):
        """The reference's waveform augmentations on padded windows, IN PLACE (include/avcer_hip.h avcer_wave_augment;
        wave_augmentation.py:8-108): chunks f32 [n, win], a contiguous device tensor as Engine.audio_chunks(padding="constant")
        returns it; recs: a HOST array of augment.REC records [n] (kind, ratio, u, key; augment.draw_plan makes them); noise f32
        [n, win] or None: added to the windows of kind 2 in place of the generated noise.  Returns chunks, and with `return_std` also
        the f32 [n] standard deviations the kernel took for its kind-2 windows (NaN elsewhere).  Shapes that disagree raise
        ValueError; limits are the library's (AvcerError).  No host synchronisation behind the upload of the records."""
        from .augment import REC

        if not (isinstance(chunks, torch.Tensor) and chunks.is_cuda and chunks.dtype == torch.float32 and chunks.dim() == 2
                and chunks.is_contiguous()):
            raise ValueError("wave_augment: chunks must be a contiguous float32 device tensor [n, win] (it is changed in place)")
        n, win = int(chunks.shape[0]), int(chunks.shape[1])
        rc = np.ascontiguousarray(recs)
        if rc.dtype != REC or rc.shape != (n,):
            raise ValueError(f"wave_augment: {n} records of augment.REC expected, got {rc.dtype} {rc.shape}")
        nz = None
        if noise is not None:
            nz = self._dev(noise, torch.float32)
            if tuple(nz.shape) != (n, win):
                raise ValueError(f"wave_augment: noise [{n}, {win}] expected, got {tuple(nz.shape)}")
        std = torch.full((n,), float("nan"), device=self.device) if return_std else None
        if n:
            recs_dev = self._new(n * REC.itemsize, dtype=torch.uint8)
            part_len = 4096 * -(-win // (1 << 20))             # include/avcer_hip.h: CH and P of avcer_wave_augment
            used = nz is None and bool((rc["kind"] == 2).any())  # only kind 2 with the generated noise takes a std
            parts = self._new(n * -(-win // part_len) * 2 if used else 1, dtype=torch.float64)
            self._check(self.lib.avcer_wave_augment(self.ctx, _ptr(chunks), n, win, rc.ctypes.data_as(C.c_void_p), _ptr(recs_dev),
                                                    float(min_snr), float(max_snr), _ptr(nz), _ptr(parts), _ptr(std), self._stream()))
        return (chunks, std) if return_std else chunks

    def head_fit(self, feats, targets, hyper, class_w, w0, b0, order, mix_lam=None, mix_index=None, epochs: int = 1,
                 batch_size: int = 64, view=None):
        """K runs of fitting the classifier head, all epochs, in one launch (include/avcer_hip.h avcer_head_fit;
        net_trainer.py:357-467, 574-604).  feats f32 [n, F] (a device tensor stays where it is), targets [n] in [0, C); hyper: a
        HOST float64 [K, 12] table (kind, label_smoothing, gamma, lr, beta1, beta2, eps, t0, eta_min, mixup, first_epoch, 0);
        class_w [K, C], w0 [K, C, F], b0 [K, C], order int32 [K, epochs, n], mix_lam [K, epochs, n_batches] and mix_index int32
        [K, epochs, n] or both None.  head_fit.fit_heads builds and validates these tables: this call checks shapes only, and the
        kernel turns a row number, position or target out of range into NaN.  Returns (w_hist f32 [K, epochs, C, F], b_hist f32
        [K, epochs, C], batch_loss f32 [K, epochs, n_batches], epoch_loss f64 [K, epochs]) on the device.  Shapes that disagree
        raise ValueError; limits are the library's (AvcerError).  No host synchronisation behind the upload of the tables.
        feats f32 [V, n, F] with view int32 [K, epochs]: epoch e of run r takes its rows from feats[view[r, e]] (avcer_head_fit_views;
        a view out of range turns its epoch into NaN)."""
        x = self._dev(feats, torch.float32)
        t = self._dev(targets, torch.int32)
        hy = np.ascontiguousarray(np.asarray(hyper, dtype=np.float64))
        views = None
        if x.dim() == 3 and x.shape[0] >= 1:
            views, x = int(x.shape[0]), x.reshape(-1, x.shape[2])
        elif view is not None:
            raise ValueError("head_fit: view comes with feats [V, n, F]")
        if x.dim() != 2 or t.dim() != 1 or int(t.shape[0]) * (views or 1) != int(x.shape[0]) or hy.ndim != 2 or hy.shape[1] != 12:
            raise ValueError(f"head_fit: feats [n, F] or [V, n, F], targets [n] and hyper [K, 12] expected, got {tuple(np.shape(feats))}, "
                             f"{tuple(t.shape)}, {hy.shape}")
        n, f, k, ep, bsz = int(t.shape[0]), int(x.shape[1]), int(hy.shape[0]), int(epochs), int(batch_size)
        vw = None
        if views is not None:
            vw = self._dev(np.zeros((k, ep), np.int32) if view is None else view, torch.int32)
            if tuple(vw.shape) != (k, ep):
                raise ValueError(f"head_fit: view [{k}, {ep}] expected, got {tuple(vw.shape)}")
        w = self._dev(w0, torch.float32)
        if w.dim() != 3 or int(w.shape[0]) != k or int(w.shape[2]) != f:
            raise ValueError(f"head_fit: w0 [{k}, C, {f}] expected, got {tuple(w.shape)}")
        c = int(w.shape[1])
        n_batches = -(-n // bsz) if n > 0 and bsz > 0 else 0
        cw, b, od = self._dev(class_w, torch.float32), self._dev(b0, torch.float32), self._dev(order, torch.int32)
        if tuple(cw.shape) != (k, c) or tuple(b.shape) != (k, c) or tuple(od.shape) != (k, ep, n):
            raise ValueError(f"head_fit: class_w and b0 [{k}, {c}] and order [{k}, {ep}, {n}] expected, got {tuple(cw.shape)}, "
                             f"{tuple(b.shape)}, {tuple(od.shape)}")
        if (mix_lam is None) != (mix_index is None):
            raise ValueError("head_fit: mix_lam and mix_index come together")
        lam = idx = None
        if mix_lam is not None:
            lam, idx = self._dev(mix_lam, torch.float32), self._dev(mix_index, torch.int32)
            if tuple(lam.shape) != (k, ep, n_batches) or tuple(idx.shape) != (k, ep, n):
                raise ValueError(f"head_fit: mix_lam [{k}, {ep}, {n_batches}] and mix_index [{k}, {ep}, {n}] expected, got "
                                 f"{tuple(lam.shape)}, {tuple(idx.shape)}")
        w_hist, b_hist, batch_loss = self._new(k, ep, c, f), self._new(k, ep, c), self._new(k, ep, n_batches)
        epoch_loss, hy_dev = self._new(k, ep, dtype=torch.float64), self._new(k, 12, dtype=torch.float64)
        tail = (n, f, c, k, ep, bsz, hy.ctypes.data_as(C.c_void_p), _ptr(hy_dev), _ptr(cw), _ptr(w), _ptr(b), _ptr(od), _ptr(lam), _ptr(idx),
                _ptr(w_hist), _ptr(b_hist), _ptr(batch_loss), _ptr(epoch_loss), self._stream())
        if views is None:
            self._check(self.lib.avcer_head_fit(self.ctx, _ptr(x), _ptr(t), *tail))
        else:
            self._check(self.lib.avcer_head_fit_views(self.ctx, _ptr(x), views, _ptr(vw), _ptr(t), *tail))
        return w_hist, b_hist, batch_loss, epoch_loss

    def head_apply(self, feats, w, b, out=None):
        """The logits of a feature table under many heads in one launch (include/avcer_hip.h avcer_head_apply): feats f32 [m, F],
        w f32 [H, C, F], b f32 [H, C] -> f32 [H, m, C] on the device (`out`: write into this contiguous tensor).  A head alone
        gives the bits it gives among many.  Shapes that disagree raise ValueError; limits are the library's (AvcerError)."""
        x, ww, bb = self._dev(feats, torch.float32), self._dev(w, torch.float32), self._dev(b, torch.float32)
        if x.dim() != 2 or ww.dim() != 3 or int(ww.shape[2]) != int(x.shape[1]) or tuple(bb.shape) != tuple(ww.shape[:2]):
            raise ValueError(f"head_apply: feats [m, F], w [H, C, F] and b [H, C] expected, got {tuple(x.shape)}, {tuple(ww.shape)}, "
                             f"{tuple(bb.shape)}")
        m, f, h, c = int(x.shape[0]), int(x.shape[1]), int(ww.shape[0]), int(ww.shape[1])
        if out is None:
            out = self._new(h, m, c)
        elif tuple(out.shape) != (h, m, c) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"head_apply: out must be a contiguous float32 tensor of shape {(h, m, c)}")
        self._check(self.lib.avcer_head_apply(self.ctx, _ptr(x), _ptr(ww), _ptr(bb), m, f, c, h, _ptr(out), self._stream()))
        return out

    def ccc(self, targets, predicts):
        """The concordance correlation coefficient of two series (include/avcer_hip.h avcer_ccc; accuracy_utils.ccc_score):
        tensors or arrays of equal element counts, read as float64; a one-dimensional strided view of a device float64 tensor (a
        column of an [n, t, 2] table) is read where it lies.  Returns a float64 [1] tensor on the device.  No host synchronisation."""
        def series(v):
            if isinstance(v, torch.Tensor) and v.dtype == torch.float64 and v.device == torch.device(self.device) and v.dim() == 1 \
                    and (v.numel() < 2 or v.stride(0) >= 1):
                return v, int(v.stride(0)) if v.numel() > 1 else 1
            return self._dev(v, torch.float64).reshape(-1), 1

        (a, sa), (b, sb) = series(targets), series(predicts)
        if a.numel() != b.numel():
            raise ValueError(f"ccc: {a.numel()} targets and {b.numel()} predictions")
        if sa != sb:
            a, b, sa = a.contiguous(), b.contiguous(), 1
        out = self._new(1, dtype=torch.float64)
        self._check(self.lib.avcer_ccc(self.ctx, _ptr(a), _ptr(b), int(a.numel()), sa, _ptr(out), self._stream()))
        return out

    def face_decode(self, loc, conf, landms, priors, image_size, variance=(0.1, 0.2)):
        """RetinaFace head outputs [P,4], [P,2], [P,10] + priors [P,4] -> dets [P,15] in pixels (before filtering)."""
        loc, conf = self._dev(loc, torch.float32), self._dev(conf, torch.float32)
        landms, priors = self._dev(landms, torch.float32), self._dev(priors, torch.float32)
        p = int(priors.shape[0])
        if tuple(loc.shape) != (p, 4) or tuple(conf.shape) != (p, 2) or tuple(landms.shape) != (p, 10) or priors.shape[1] != 4:
            raise ValueError("face_decode: loc [P,4], conf [P,2], landms [P,10], priors [P,4]")
        dets = self._new(p, 15)
        self._check(self.lib.avcer_face_decode(self.ctx, _ptr(loc), _ptr(conf), _ptr(landms), _ptr(priors), p,
                                               int(image_size[0]), int(image_size[1]), float(variance[0]),
                                               float(variance[1]), _ptr(dets), self._stream()))
        return dets

    def face_decode_batch(self, loc, conf, landms, priors, image_size, variance=(0.1, 0.2)):
        """The same for T frames in one launch: loc [T,P,4], conf [T,P,2], landms [T,P,10] + priors [P,4] -> dets [T,P,15]."""
        loc, conf = self._dev(loc, torch.float32), self._dev(conf, torch.float32)
        landms, priors = self._dev(landms, torch.float32), self._dev(priors, torch.float32)
        t, p = int(loc.shape[0]), int(priors.shape[0])
        if tuple(loc.shape) != (t, p, 4) or tuple(conf.shape) != (t, p, 2) or tuple(landms.shape) != (t, p, 10) or priors.shape[1] != 4:
            raise ValueError("face_decode_batch: loc [T,P,4], conf [T,P,2], landms [T,P,10], priors [P,4]")
        dets = self._new(t, p, 15)
        self._check(self.lib.avcer_face_decode_batch(self.ctx, _ptr(loc), _ptr(conf), _ptr(landms), _ptr(priors), t, p,
                                                     int(image_size[0]), int(image_size[1]), float(variance[0]),
                                                     float(variance[1]), _ptr(dets), self._stream()))
        return dets

    def face_nms(self, dets, conf_thresh: float = 0.02, nms_thresh: float = 0.4, nms_top_k: int = 5000, top_k: int = 750,
                 threshold: float = 0.8):
        """dets [T,P,15] (face_decode output per frame) -> (rows [T,top_k,15], counts [T]) after the reference's confidence
        floor, NMS, top-k and final threshold; only counts[t] rows of frame t are meaningful."""
        d = self._dev(dets, torch.float32)
        if d.dim() == 2:
            d = d[None]
        if d.dim() != 3 or d.shape[2] != 15:
            raise ValueError("face_nms: dets [T,P,15]")
        t, p = int(d.shape[0]), int(d.shape[1])
        out = self._new(t, top_k, 15)
        cnt = self._new(t, dtype=torch.int32)
        self._check(self.lib.avcer_face_nms(self.ctx, _ptr(d), t, p, float(conf_thresh), float(nms_thresh), int(nms_top_k),
                                            int(top_k), float(threshold), _ptr(out), _ptr(cnt), self._stream()))
        return out, cnt

    def s3fd_detect(self, loc, conf, priors, image_size, variance=(0.1, 0.2), conf_thresh: float = 0.05, nms_thresh: float = 0.3,
                    nms_top_k: int = 5000, top_k: int = 750, threshold: float = 0.8):
        """S3FD's `Detect` and the predictor's threshold loop for T frames (avcer_s3fd_detect): loc [T,P,4], conf [T,P,2] softmaxed,
        priors [P,4] -> (rows [T,top_k,5] = x0, y0, x1, y1 in pixels, score; counts [T]); only counts[t] rows of frame t are meaningful."""
        loc, conf, priors = self._dev(loc, torch.float32), self._dev(conf, torch.float32), self._dev(priors, torch.float32)
        if loc.dim() == 2:
            loc, conf = loc[None], conf[None]
        t, p = int(loc.shape[0]), int(priors.shape[0])
        if tuple(loc.shape) != (t, p, 4) or tuple(conf.shape) != (t, p, 2) or tuple(priors.shape) != (p, 4):
            raise ValueError("s3fd_detect: loc [T,P,4], conf [T,P,2], priors [P,4]")
        out = self._new(t, top_k, 5)
        cnt = self._new(t, dtype=torch.int32)
        self._check(self.lib.avcer_s3fd_detect(self.ctx, _ptr(loc), _ptr(conf), _ptr(priors), t, p, int(image_size[0]), int(image_size[1]),
                                               float(variance[0]), float(variance[1]), float(conf_thresh), float(nms_thresh),
                                               int(nms_top_k), int(top_k), float(threshold), _ptr(out), _ptr(cnt), self._stream()))
        return out, cnt

    def track_faces(self, dets_per_frame, frame_w: int, frame_h: int, iou_threshold: float = 0.4, minimum_face_size: float = 0.0):
        """The tracker + crop-rectangle loop of `VideoPredictor.process` for a whole video in one native HOST call
        (csrc/track.hip): per-frame detection arrays [k, >= 4] -> records int64 [n, 6] = frame, track directory, x0, y0, x1, y1.
        Raises ValueError where the reference raises (zero-area detection, empty crop)."""
        boxes, counts, rec = _pack_detections(dets_per_frame)
        n = C.c_int64(0)
        rc = self.lib.avcer_track_faces(self.ctx, boxes.ctypes.data_as(C.c_void_p), 4, counts.ctypes.data_as(C.c_void_p), len(counts),
                                        int(frame_w), int(frame_h), float(iou_threshold), float(minimum_face_size),
                                        rec.ctypes.data_as(C.c_void_p), C.byref(n))
        if rc == -1:
            raise ValueError(self.lib.avcer_last_error(self.ctx).decode("utf-8", "replace"))
        self._check(rc)
        return rec[:int(n.value)]

    def tracker(self, iou_threshold: float = 0.4, minimum_face_size: float = 0.0) -> "FaceTracker":
        """`track_faces` for a video that arrives in passes: a `FaceTracker` whose `.push(dets_per_frame, w, h)` takes the next
        frames and returns their records, with the frame index counted over the whole video.  All pushes together give what one
        track_faces call on the whole gives."""
        return FaceTracker(self.lib, iou_threshold, minimum_face_size)

    def crop_tiles(self, frames_u8, rects, bgr: bool = True):
        """frames u8 [T,H,W,3] + rects i32 [n,5] (frame, x0, y0, x1, y1; validated by the caller) -> RGB tiles [n,224,224,3]."""
        x = self._dev(frames_u8, torch.uint8)
        r = self._dev(rects, torch.int32)
        if x.dim() != 4 or x.shape[-1] != 3 or r.dim() != 2 or r.shape[1] != 5:
            raise ValueError("crop_tiles: frames [T,H,W,3] uint8, rects [n,5] int32")
        n = int(r.shape[0])
        tiles = self._new(n, 224, 224, 3, dtype=torch.uint8)
        self._check(self.lib.avcer_crop_tiles(self.ctx, _ptr(x), int(x.shape[0]), int(x.shape[1]), int(x.shape[2]),
                                              _ptr(r), n, 1 if bgr else 0, _ptr(tiles), self._stream()))
        return tiles

    def jpeg_tiles(self, coeffs, desc, n: int, n_blocks: int, out=None):
        """Coefficients int16 [>= 64 * n_blocks] and descriptors (n records of struct avcer_jpeg_desc as bytes), both on the device
        as avcer_jpeg_entropy_batch wrote them (avcer_amd/jpeg.py) -> (RGB tiles u8 [n,224,224,3], flags i32 [n] on the device); a tile is zero for a file not decoded: status not OK, or flag 1
        (the inverse DCT left the range inside which the decode is defined, include/avcer_hip.h)."""
        if coeffs.dtype != torch.int16 or coeffs.numel() < 64 * n_blocks or desc.dtype != torch.uint8 or desc.numel() < _JPEG_DESC_BYTES * n or \
                not coeffs.is_cuda or not desc.is_cuda:
            raise ValueError("jpeg_tiles: coeffs int16 [64 * n_blocks], desc uint8 [sizeof(avcer_jpeg_desc) * n], both on the device")
        tiles = self._new(n, 224, 224, 3, dtype=torch.uint8) if out is None else out
        if tuple(tiles.shape) != (n, 224, 224, 3) or tiles.dtype != torch.uint8 or not tiles.is_contiguous():
            raise ValueError("jpeg_tiles: out must be a contiguous uint8 [n,224,224,3]")
        flags = self._new(n, dtype=torch.int32)
        self._check(self.lib.avcer_jpeg_tiles(self.ctx, _ptr(coeffs), int(n_blocks), _ptr(desc), int(n), _ptr(flags), _ptr(tiles),
                                              self._stream()))
        return tiles, flags

    def jpeg_forward(self, src, rects, desc, n: int, n_blocks: int, bgr: bool = False, out=None):
        """The forward half of the JPEG encoder (avcer_jpeg_forward): image i is the half-open rectangle rects[i] = (slot, x0, y0, x1, y1)
        (int32 [n,5] on the device) of src u8 [N,H,W,3] (RGB, or BGR with `bgr`); desc = n records of struct avcer_jpeg_desc as bytes on
        the device, as avcer_jpeg_plan wrote them -> quantised coefficients int16 [64 * n_blocks] in the layout the decoder reads."""
        if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3 or not src.is_cuda or not src.is_contiguous():
            raise ValueError("jpeg_forward: src must be a contiguous uint8 [N,H,W,3] on the device")
        if rects.dtype != torch.int32 or tuple(rects.shape) != (n, 5) or not rects.is_cuda or not rects.is_contiguous():
            raise ValueError("jpeg_forward: rects must be a contiguous int32 [n,5] on the device")
        if desc.dtype != torch.uint8 or desc.numel() < _JPEG_DESC_BYTES * n or not desc.is_cuda:
            raise ValueError("jpeg_forward: desc uint8 [sizeof(avcer_jpeg_desc) * n] on the device")
        coeffs = self._new(64 * int(n_blocks), dtype=torch.int16) if out is None else out
        if coeffs.dtype != torch.int16 or coeffs.numel() < 64 * n_blocks or not coeffs.is_cuda or not coeffs.is_contiguous():
            raise ValueError("jpeg_forward: out must be a contiguous int16 [>= 64 * n_blocks] on the device")
        self._check(self.lib.avcer_jpeg_forward(self.ctx, _ptr(src), int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), _ptr(rects),
                                                _ptr(desc), int(n), 1 if bgr else 0, _ptr(coeffs), int(n_blocks), self._stream()))
        return coeffs

    def _jpeg_roundtrip_args(self, what, src, rects, desc, n, n_blocks, keep_coeffs):
        if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3 or not src.is_cuda or not src.is_contiguous():
            raise ValueError(f"{what}: src must be a contiguous uint8 [N,H,W,3] on the device")
        if rects.dtype != torch.int32 or tuple(rects.shape) != (n, 5) or not rects.is_cuda or not rects.is_contiguous():
            raise ValueError(f"{what}: rects must be a contiguous int32 [n,5] on the device")
        if desc.dtype != torch.uint8 or desc.numel() < _JPEG_DESC_BYTES * n or not desc.is_cuda or n <= 0 or n_blocks <= 0:
            raise ValueError(f"{what}: desc uint8 [sizeof(avcer_jpeg_desc) * n] on the device, n and n_blocks positive")
        return (self._new(64 * int(n_blocks), dtype=torch.int16) if keep_coeffs else None), self._new(int(n), dtype=torch.int32)

    def jpeg_roundtrip_tiles(self, src, rects, desc, n: int, n_blocks: int, bgr: bool = False, keep_coeffs: bool = False):
        """The crops as the JPEG files of them would read back, without the files (avcer_jpeg_roundtrip_tiles): arguments as
        jpeg_forward takes them -> (RGB tiles u8 [n,224,224,3] as jpeg_tiles gives them for the files jpeg.encode_images writes,
        flags i32 [n], the quantised coefficients int16 [64 * n_blocks] of jpeg_forward when `keep_coeffs`, else None)."""
        coeffs, flags = self._jpeg_roundtrip_args("jpeg_roundtrip_tiles", src, rects, desc, n, n_blocks, keep_coeffs)
        tiles = self._new(int(n), 224, 224, 3, dtype=torch.uint8)
        self._check(self.lib.avcer_jpeg_roundtrip_tiles(self.ctx, _ptr(src), int(src.shape[0]), int(src.shape[1]), int(src.shape[2]),
                                                        _ptr(rects), _ptr(desc), int(n), 1 if bgr else 0,
                                                        _ptr(coeffs) if keep_coeffs else None, int(n_blocks), _ptr(flags), _ptr(tiles),
                                                        self._stream()))
        return tiles, flags, coeffs

    def jpeg_roundtrip_rgb(self, src, rects, desc, n: int, n_blocks: int, hmax: int, wmax: int, bgr: bool = False,
                           keep_coeffs: bool = False):
        """The same round trip at full size (avcer_jpeg_roundtrip_rgb) -> (canvas u8 [n,hmax,wmax,3] RGB as jpeg_rgb gives it, flags,
        coefficients or None)."""
        coeffs, flags = self._jpeg_roundtrip_args("jpeg_roundtrip_rgb", src, rects, desc, n, n_blocks, keep_coeffs)
        if hmax <= 0 or wmax <= 0:
            raise ValueError("jpeg_roundtrip_rgb: canvas sizes positive")
        canvas = self._new(int(n), int(hmax), int(wmax), 3, dtype=torch.uint8)
        self._check(self.lib.avcer_jpeg_roundtrip_rgb(self.ctx, _ptr(src), int(src.shape[0]), int(src.shape[1]), int(src.shape[2]),
                                                      _ptr(rects), _ptr(desc), int(n), 1 if bgr else 0,
                                                      _ptr(coeffs) if keep_coeffs else None, int(n_blocks), _ptr(flags), _ptr(canvas),
                                                      int(hmax), int(wmax), self._stream()))
        return canvas, flags, coeffs

    def jpeg_pack(self, coeffs, desc, n: int, blocks: int, cap_bytes: int):
        """The entropy-coding half of the JPEG encoder on the device (avcer_jpeg_pack): coefficients int16 [>= 64 * blocks] as
        jpeg_forward leaves them and desc = n records of struct avcer_jpeg_desc as bytes, both on the device -> (out u8 [cap_bytes]:
        the files back to back, offsets i64 [n + 1], status i32 [n]: 0 or the reason a file has no bytes, bytes_needed i64 [1]), all on
        the device.  Byte-identical to avcer_jpeg_write_batch on the same arrays."""
        if coeffs.dtype != torch.int16 or coeffs.numel() < 64 * blocks or desc.dtype != torch.uint8 or desc.numel() < _JPEG_DESC_BYTES * n or \
                not coeffs.is_cuda or not desc.is_cuda or not coeffs.is_contiguous() or not desc.is_contiguous():
            raise ValueError("jpeg_pack: coeffs int16 [64 * blocks], desc uint8 [sizeof(avcer_jpeg_desc) * n], both contiguous on the device")
        out = self._new(int(cap_bytes), dtype=torch.uint8)
        offsets = self._new(int(n) + 1, dtype=torch.int64)
        status = self._new(int(n), dtype=torch.int32)
        need = self._new(1, dtype=torch.int64)
        self._check(self.lib.avcer_jpeg_pack(self.ctx, _ptr(coeffs), int(blocks), _ptr(desc), int(n), _ptr(out) if cap_bytes else None,
                                             int(cap_bytes), _ptr(offsets), _ptr(status), _ptr(need), self._stream()))
        return out, offsets, status, need

    def jpeg_unpack(self, data, scan, tabs, n_tabs: int, desc, n: int, n_blocks: int, sub_bits: int = 0, out=None):
        """The Huffman decode of the JPEG reader on the device (avcer_jpeg_unpack): data u8 = the entropy-coded bytes, scan and tabs
        = n records of struct avcer_jpeg_scan and n_tabs of struct avcer_jpeg_tab as bytes, desc = n records of struct avcer_jpeg_desc
        as bytes, all on the device as avcer_jpeg_scan_batch wrote them (avcer_amd/jpeg.py) -> (coefficients int16 [64 * n_blocks],
        status i32 [n]), both on the device; status and reason of `desc` are updated in place.  Exactly what
        avcer_jpeg_entropy_batch computes from the same files.  sub_bits: bits per subsequence, 0 = the library's default, else a
        multiple of 32 of at least 128; the result does not depend on it."""
        from .jpeg import SCAN as _SCAN, TAB as _TAB

        for name, x, size in (("data", data, 1), ("scan", scan, _SCAN.itemsize * n), ("tabs", tabs, _TAB.itemsize * n_tabs),
                              ("desc", desc, _JPEG_DESC_BYTES * n)):
            if x.dtype != torch.uint8 or x.numel() < size or not x.is_cuda or not x.is_contiguous():
                raise ValueError(f"jpeg_unpack: {name} must be a contiguous uint8 tensor of at least {size} bytes on the device")
        if n <= 0 or n_tabs <= 0 or n_blocks <= 0 or sub_bits < 0 or (sub_bits and (sub_bits < 128 or sub_bits % 32)):
            raise ValueError("jpeg_unpack: n, n_tabs and n_blocks positive; sub_bits 0 or a multiple of 32 of at least 128")
        coeffs = self._new(64 * int(n_blocks), dtype=torch.int16) if out is None else out
        if coeffs.dtype != torch.int16 or coeffs.numel() < 64 * n_blocks or not coeffs.is_cuda or not coeffs.is_contiguous():
            raise ValueError("jpeg_unpack: out must be a contiguous int16 [>= 64 * n_blocks] on the device")
        status = self._new(int(n), dtype=torch.int32)
        self._check(self.lib.avcer_jpeg_unpack(self.ctx, _ptr(data), int(data.numel()), _ptr(scan), _ptr(tabs), int(n_tabs), _ptr(desc),
                                               int(n), _ptr(coeffs), int(n_blocks), _ptr(status), int(sub_bits), self._stream()))
        return coeffs, status

    def jpeg_rgb(self, coeffs, desc, n: int, n_blocks: int, hmax: int, wmax: int):
        """The same files at full size -> (canvas u8 [n,hmax,wmax,3] RGB: image i in the top left corner of slot i, zeros around it;
        flags i32 [n] as jpeg_tiles returns them)."""
        if coeffs.dtype != torch.int16 or coeffs.numel() < 64 * n_blocks or desc.dtype != torch.uint8 or desc.numel() < _JPEG_DESC_BYTES * n or \
                not coeffs.is_cuda or not desc.is_cuda:
            raise ValueError("jpeg_rgb: coeffs int16 [64 * n_blocks], desc uint8 [sizeof(avcer_jpeg_desc) * n], both on the device")
        canvas = self._new(n, int(hmax), int(wmax), 3, dtype=torch.uint8)
        flags = self._new(n, dtype=torch.int32)
        self._check(self.lib.avcer_jpeg_rgb(self.ctx, _ptr(coeffs), int(n_blocks), _ptr(desc), int(n), _ptr(flags), _ptr(canvas), int(hmax),
                                            int(wmax), self._stream()))
        return canvas, flags

    def jpeg_frames(self, coeffs, desc, n: int, n_blocks: int, height: int, width: int, bgr: bool = True, out=None):
        """The same files as video frames (avcer_jpeg_frames) -> (frames u8 [n,height,width,3] in BGR order, or RGB with bgr=False;
        flags i32 [n]: 1 as jpeg_tiles returns it, 2 for a decoded file of another size than width x height; such a frame is zero)."""
        if coeffs.dtype != torch.int16 or coeffs.numel() < 64 * n_blocks or desc.dtype != torch.uint8 or desc.numel() < _JPEG_DESC_BYTES * n or \
                not coeffs.is_cuda or not desc.is_cuda:
            raise ValueError("jpeg_frames: coeffs int16 [64 * n_blocks], desc uint8 [sizeof(avcer_jpeg_desc) * n], both on the device")
        frames = self._new(n, int(height), int(width), 3, dtype=torch.uint8) if out is None else out
        if tuple(frames.shape) != (n, int(height), int(width), 3) or frames.dtype != torch.uint8 or not frames.is_contiguous() or \
                not frames.is_cuda:
            raise ValueError("jpeg_frames: out must be a contiguous uint8 [n,height,width,3] on the device")
        flags = self._new(n, dtype=torch.int32)
        self._check(self.lib.avcer_jpeg_frames(self.ctx, _ptr(coeffs), int(n_blocks), _ptr(desc), int(n), _ptr(flags), _ptr(frames),
                                               int(height), int(width), 1 if bgr else 0, self._stream()))
        return frames, flags

    def dib_frames(self, span, offsets, n: int, height: int, width: int, bits: int, bottom_up: bool, bgr: bool = True, out=None):
        """Uncompressed video frames (avcer_dib_frames): span u8 [bytes] and offsets i64 [n] on the device (the first byte of each
        frame's chunk data in `span`, any alignment) -> frames u8 [n,height,width,3] in BGR order, or RGB with bgr=False.  A frame
        is `height` rows of (width * bits / 8 + 3) & ~3 bytes, bits 24 or 32, the last row first when bottom_up."""
        if span.dtype != torch.uint8 or span.dim() != 1 or not span.is_cuda or span.stride(0) != 1:
            raise ValueError("dib_frames: span must be a uint8 vector on the device")
        if offsets.dtype != torch.int64 or offsets.numel() < n or not offsets.is_cuda or not offsets.is_contiguous():
            raise ValueError("dib_frames: offsets int64 [n] on the device")
        if int(bits) not in (24, 32):
            raise ValueError(f"dib_frames: {bits} bits a pixel (24 or 32)")
        frames = self._new(n, int(height), int(width), 3, dtype=torch.uint8) if out is None else out
        if tuple(frames.shape) != (n, int(height), int(width), 3) or frames.dtype != torch.uint8 or not frames.is_contiguous() or \
                not frames.is_cuda:
            raise ValueError("dib_frames: out must be a contiguous uint8 [n,height,width,3] on the device")
        self._check(self.lib.avcer_dib_frames(self.ctx, _ptr(span), int(span.numel()), _ptr(offsets), int(n), _ptr(frames), int(height),
                                              int(width), int(bits), 1 if bottom_up else 0, 1 if bgr else 0, self._stream()))
        return frames

    def crop_resize_linear(self, frames_u8, rects, swap_rb: bool = False, out_h: int = 224, out_w: int = 224):
        """frames u8 [T,H,W,3] + rects i32 [n,5] (frame, x0, y0, x1, y1) -> u8 [n,out_h,out_w,3]: cv2.resize of each crop with
        INTER_LINEAR, first and last channel swapped when `swap_rb`."""
        x = self._dev(frames_u8, torch.uint8)
        r = self._dev(rects, torch.int32)
        if x.dim() != 4 or x.shape[-1] != 3 or r.dim() != 2 or r.shape[1] != 5:
            raise ValueError("crop_resize_linear: frames [T,H,W,3] uint8, rects [n,5] int32")
        n = int(r.shape[0])
        out = self._new(n, out_h, out_w, 3, dtype=torch.uint8)
        if n:
            self._check(self.lib.avcer_crop_resize_linear(self.ctx, _ptr(x), int(x.shape[0]), int(x.shape[1]), int(x.shape[2]),
                                                          _ptr(r), n, 1 if swap_rb else 0, int(out_h), int(out_w), _ptr(out),
                                                          self._stream()))
        return out

    def cam_render(self, cam, rows, cls, base_rgb, lut_bgr, image_weight: float = 0.8):
        """Grad-CAM overlays: cam f32 [M,7,7,7] (static_forward_cam), rows [n] (map rows, checked here), cls [n] (classes 0..6),
        base_rgb u8 [n,224,224,3], lut_bgr u8 [256,3] -> u8 [n,224,224,3] BGR as show_cam_on_image returns it."""
        cam = self._dev(cam, torch.float32)
        rows_h = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows, dtype=np.int64).reshape(-1)
        if cam.dim() != 4 or tuple(cam.shape[1:]) != (7, 7, 7):
            raise ValueError(f"cam must be [M,7,7,7] float32, got {tuple(cam.shape)}")
        if len(rows_h) and (rows_h.min() < 0 or rows_h.max() >= cam.shape[0]):
            raise ValueError("cam_render: a row outside the maps")
        r = self._dev(rows_h.astype(np.int32), torch.int32)
        c = self._dev(cls, torch.int32).reshape(-1)
        b = self._dev(base_rgb, torch.uint8)
        lut = self._dev(lut_bgr, torch.uint8)
        n = len(rows_h)
        if c.numel() != n or tuple(b.shape) != (n, 224, 224, 3) or tuple(lut.shape) != (256, 3):
            raise ValueError("cam_render: cls [n], base_rgb [n,224,224,3] uint8, lut_bgr [256,3] uint8")
        if not 0.0 <= float(image_weight) <= 1.0:
            raise ValueError(f"image_weight should be in the range [0, 1], got {image_weight}")
        out = self._new(n, 224, 224, 3, dtype=torch.uint8)
        if n:
            self._check(self.lib.avcer_cam_render(self.ctx, _ptr(cam), _ptr(r), _ptr(c), _ptr(b), n, _ptr(lut), float(image_weight),
                                                  _ptr(out), self._stream()))
        return out

    def annotate(self, frames, items, masks, table):
        """The result video's drawing (avcer_annotate_frames): `items` -- annotate.ITEM records sorted by frame, or a list of
        annotate.outline / fill / mask records -- drawn IN PLACE into frames u8 [n,H,W,3] on the device, one after another per frame,
        exactly as annotate.draw_numpy draws them; masks u8 [bytes] (the coverage masks back to back; moved to the device if they are
        not there) and table int [k,3] = offset, width, height per mask (annotate.pack_masks).  Every item is checked on the host
        first: a frame outside [0, n), x1 < x0 or y1 < y0, a width below 1, a coverage outside 1..255, a mask index or scale out of
        range raise ValueError naming the item, before any launch.  Returns `frames`."""
        from . import annotate as an

        if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and
                frames.shape[-1] == 3 and frames.is_contiguous()):
            raise ValueError("annotate: frames must be a contiguous uint8 [n,H,W,3] on the device")
        n, h, w = (int(v) for v in frames.shape[:3])
        items = an.as_items(items)
        table = np.ascontiguousarray(np.asarray(table.cpu() if torch.is_tensor(table) else table, dtype=np.int32).reshape(-1, 3))
        m_dev = self._dev(masks, torch.uint8).reshape(-1)
        an.check_items(items, n, table, int(m_dev.numel()))
        if n == 0 or h == 0 or w == 0:
            return frames
        work, n_tiles = an.work_table(items, table, n, h, w)
        if not len(items) or not n_tiles:
            return frames
        n_i, n_w = 12 * len(items), work.size
        ints = np.concatenate([items.view(np.int32).reshape(-1), work.reshape(-1), table.reshape(-1)])
        d = torch.from_numpy(ints).to(self.device, non_blocking=True)  # one copy for items, launch plan and mask table
        self._check(self.lib.avcer_annotate_frames(self.ctx, _ptr(frames), n, h, w, _ptr(d), len(items), _ptr(m_dev) if m_dev.numel() else None,
                                                   int(m_dev.numel()), _ptr(d[n_i + n_w:]) if len(table) else None, len(table),
                                                   _ptr(d[n_i:]), len(work), int(n_tiles), self._stream()))
        return frames

    def fuse(self, stat, dyn_logits, aud_mean, n_aud: int, weights_1=None, weights_2=(1, 1, 1),
             ce_weights_type: bool = False, ce_mask: bool = True):
        stat = self._dev(stat, torch.float32)
        dyn = self._dev(dyn_logits, torch.float32)
        aud = self._dev(aud_mean, torch.float32)
        n = int(stat.shape[0])
        if tuple(stat.shape) != (n, 7) or tuple(dyn.shape) != (n, 7) or aud.dim() != 2 or aud.shape[1] < 7:
            raise ValueError("fuse: stat/dyn [n,7], aud [n_aud,>=7]")
        if not (1 <= n_aud <= aud.shape[0]):
            raise ValueError("fuse: n_aud out of range")
        w1 = (C.c_double * 21)(*np.asarray(weights_1, dtype=np.float64).reshape(21)) if weights_1 else None
        w2 = (C.c_double * 3)(*[float(v) for v in weights_2])
        prob = self._new(4, n, 7, dtype=torch.float64)
        am = self._new(4, n, dtype=torch.int32)
        self._check(self.lib.avcer_fuse(self.ctx, _ptr(stat), _ptr(dyn), _ptr(aud), n, int(n_aud), int(aud.shape[1]),
                                        w1, w2, int(bool(ce_weights_type)), int(bool(ce_mask)), _ptr(prob), _ptr(am),
                                        self._stream()))
        return prob, am

    def fuse_videos(self, stat, dyn_logits, win_logits, frame_lo, frame_hi, frame_counts, win_counts, weights_1=None,
                    weights_2=(1, 1, 1), ce_weights_type: bool = False, ce_mask: bool = True, names=None, with_mean: bool = True):
        """`audio_frame_mean` + `fuse` for a set of videos in ONE launch (include/avcer_hip.h avcer_fuse_videos).  stat, dyn_logits
        [N,7]: the videos' frames one behind the other; win_logits [W,c]: their audio windows one behind the other; frame_lo /
        frame_hi: HOST integer arrays [W], each window's span in its own video's frame numbering (audio_pipeline.chunk_spans per
        video, concatenated); frame_counts / win_counts: frames and windows per video.  The covered prefix of every video
        (fusion.covered_frames) is settled on the host first: a video no window covers raises IndexError, one whose covered frames
        are not a prefix ValueError -- what `fusion.fuse` raises for it, with the video's name (`names`, default its index) in
        front -- before anything is launched.  Returns (comp_prob f64 [4,N,7], comp_argmax i32 [4,N], aud_mean f32 [N,c], count
        i32 [N]); the last two are None unless `with_mean`.  A video's slices equal what the two calls give for it alone, bit for
        bit.  No host synchronisation."""
        from .fusion import covered_frames

        stat = self._dev(stat, torch.float32)
        dyn = self._dev(dyn_logits, torch.float32)
        win = self._dev(win_logits, torch.float32)
        lo = np.asarray(frame_lo.cpu() if torch.is_tensor(frame_lo) else frame_lo).reshape(-1).astype(np.int64)
        hi = np.asarray(frame_hi.cpu() if torch.is_tensor(frame_hi) else frame_hi).reshape(-1).astype(np.int64)
        fc = np.asarray(frame_counts, dtype=np.int64).reshape(-1)
        wc = np.asarray(win_counts, dtype=np.int64).reshape(-1)
        nv, n, w = int(fc.size), int(fc.sum()), int(wc.sum())
        if nv < 1 or wc.size != nv or (fc < 0).any() or (wc < 0).any():
            raise ValueError("fuse_videos: frame_counts / win_counts [V] >= 0, V >= 1")
        if tuple(stat.shape) != (n, 7) or tuple(dyn.shape) != (n, 7) or win.dim() != 2 or int(win.shape[0]) != w or lo.size != w or hi.size != w:
            raise ValueError("fuse_videos: stat/dyn [sum(frame_counts),7], win_logits [sum(win_counts),c], frame_lo/hi [sum(win_counts)]")
        c = int(win.shape[1])
        if not 7 <= c <= 8:
            raise ValueError(f"fuse_videos: {c} audio classes (7..8)")
        if not (1 <= n <= 2 ** 31 - 1 and 1 <= w <= 2 ** 31 - 1):
            raise ValueError(f"fuse_videos: {n} frames and {w} windows (1..2^31-1 each)")
        f_off = np.concatenate([[0], np.cumsum(fc)])
        w_off = np.concatenate([[0], np.cumsum(wc)])
        if len(lo) and (min(lo.min(), hi.min()) < -2 ** 31 or max(lo.max(), hi.max()) > 2 ** 31 - 1):
            raise ValueError("fuse_videos: a frame span outside int32")
        n_aud = np.zeros(nv, dtype=np.int32)
        for v in range(nv):
            a, b = int(w_off[v]), int(w_off[v + 1])
            if (np.diff(lo[a:b]) < 0).any() or (np.diff(hi[a:b]) < 0).any():
                raise ValueError(f"fuse_videos: video {names[v] if names is not None else v}: frame spans must not decrease")
            try:
                n_aud[v] = covered_frames(lo[a:b], hi[a:b], int(fc[v])) if fc[v] else 1
            except (IndexError, ValueError) as e:
                raise type(e)(f"video {names[v] if names is not None else v}: {e}") from None
        idx = np.concatenate([lo, hi, f_off, w_off, n_aud]).astype(np.int32)
        idx_d = torch.from_numpy(idx).to(self.device, non_blocking=True)  # one copy for the five index arrays
        lo_d, hi_d = idx_d[:w], idx_d[w:2 * w]
        fo_d, wo_d, na_d = idx_d[2 * w:2 * w + nv + 1], idx_d[2 * w + nv + 1:2 * w + 2 * nv + 2], idx_d[2 * w + 2 * nv + 2:]
        w1 = (C.c_double * 21)(*np.asarray(weights_1, dtype=np.float64).reshape(21)) if weights_1 else None
        w2 = (C.c_double * 3)(*[float(x) for x in weights_2])
        prob = self._new(4, n, 7, dtype=torch.float64)
        am = self._new(4, n, dtype=torch.int32)
        mean = self._new(n, c) if with_mean else None
        cnt = self._new(n, dtype=torch.int32) if with_mean else None
        self._check(self.lib.avcer_fuse_videos(self.ctx, _ptr(stat), _ptr(dyn), _ptr(win), _ptr(lo_d), _ptr(hi_d), _ptr(fo_d),
                                               _ptr(wo_d), _ptr(na_d), nv, n, w, c, w1, w2, int(bool(ce_weights_type)),
                                               int(bool(ce_mask)), _ptr(mean), _ptr(cnt), _ptr(prob), _ptr(am), self._stream()))
        return prob, am, mean, cnt

    def conv_gemm(self, desc: ConvDesc, dtype: int, x, w, scale, bias, residual, y):
        self._check(self.lib.avcer_conv_gemm(self.ctx, C.byref(desc), dtype, _ptr(x), _ptr(w), _ptr(scale), _ptr(bias),
                                             _ptr(residual), _ptr(y), self._stream()))

    def profile_enable(self, on: bool = True):
        self._check(self.lib.avcer_profile_enable(self.ctx, int(on)))

    def profile_read(self):
        """(summed conv_gemm kernel time in ms, number of launches) since the last read; synchronises."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        self._check(self.lib.avcer_profile_read(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    FAMILIES = ("conv_gemm_kernel", "conv_gemm_wd_kernel", "bneck_kernel", "bneck_tail2_kernel", "stem_pool_kernel",
                "conv_gemm_skinny_kernel", "gru_layer_kernel")  # AVCER_FAM_*

    def profile_read_families(self):
        """Per kernel family since profile_enable / the last read: {name: (event ms, launches, algorithmic FLOPs, compulsory
        HBM bytes)}; synchronises.  Use instead of profile_read."""
        n = len(self.FAMILIES)
        ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
        la = (C.c_int64 * n)()
        self._check(self.lib.avcer_profile_read_families(self.ctx, n, ms, la, fl, by))
        return {name: (ms[i], int(la[i]), fl[i], by[i]) for i, name in enumerate(self.FAMILIES)}

    def profile_read_launches(self, max_n: int = 8192):
        """Launch by launch since profile_enable / the last read: list of dicts {family, ms, flops, bytes, m, n, k} in launch
        order; synchronises.  Use instead of profile_read / profile_read_families."""
        fam = np.zeros(max_n, np.int32)
        ms, fl, by = np.zeros(max_n), np.zeros(max_n), np.zeros(max_n)
        mnk = np.zeros((max_n, 3), np.int64)
        n = C.c_int64(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._check(self.lib.avcer_profile_read_launches(self.ctx, max_n, vp(fam), vp(ms), vp(fl), vp(by), vp(mnk), C.byref(n)))
        k = min(int(n.value), max_n)
        return [dict(family=self.FAMILIES[fam[i]], ms=float(ms[i]), flops=float(fl[i]), bytes=float(by[i]), m=int(mnk[i, 0]),
                     n=int(mnk[i, 1]), k=int(mnk[i, 2])) for i in range(k)]

    def debug_tap(self, name: str, numel: int, dtype=torch.float32):
        """Arm a one-shot tap; returns the destination tensor (filled by the next forward pass)."""
        dst = torch.zeros(numel, dtype=dtype, device=self.device)
        self._tap_keepalive = dst
        self._check(self.lib.avcer_debug_tap(self.ctx, name.encode(), _ptr(dst), dst.numel() * dst.element_size()))
        return dst

    def debug_tap_copied(self) -> int:
        return int(self.lib.avcer_debug_tap_copied(self.ctx))

    def split_weights(self, w):
        """f32 tensor (numel a multiple of 32) -> sp32 ACTIVATION layout (hi / lo fp16 per group of 32; int16 tensor of
        2 * numel entries): the A operand of conv_gemm dtypes 5 / 6.  Not valid for weights: use split_weight_rows."""
        w = self._dev(w, torch.float32)
        out = torch.empty(w.numel() * 2, dtype=torch.int16, device=self.device)
        self._check(self.lib.avcer_split_weights(self.ctx, _ptr(w), _ptr(out), w.numel(), self._stream()))
        return out

    def split_weight_rows(self, w):
        """f32 [N,K] weight matrix -> the split-fp16, row-permuted layout of conv_gemm dtypes 3-6 and the fused kernels
        (int16 tensor of 2*N*K entries)."""
        w = self._dev(w, torch.float32)
        if w.dim() != 2:
            raise ValueError("split_weight_rows: w [N,K]")
        out = torch.empty(w.numel() * 2 + SPLIT_TRAILER // 2, dtype=torch.int16, device=self.device)
        self._check(self.lib.avcer_split_weight_rows(self.ctx, _ptr(w), _ptr(out), int(w.shape[0]), int(w.shape[1]), self._stream()))
        return out

    def weight_frags(self, w):
        """f32 [N,K] weight matrix -> the fragment-order split layout of conv_gemm dtypes 7 / 8 (int16 tensor of 2*N*K entries)."""
        w = self._dev(w, torch.float32)
        rows = self.split_weight_rows(w)
        out = torch.empty_like(rows)
        self._check(self.lib.avcer_weight_frags(self.ctx, _ptr(rows), _ptr(out), int(w.shape[0]), int(w.shape[1]), self._stream()))
        return out

    def conv_gemm_dual(self, desc: ConvDesc, dtype: int, x, x2, w, scale, bias, residual, y):
        self._check(self.lib.avcer_conv_gemm_dual(self.ctx, C.byref(desc), dtype, _ptr(x), _ptr(x2), _ptr(w), _ptr(scale),
                                                  _ptr(bias), _ptr(residual), _ptr(y), self._stream()))

    def bneck_chain(self, planes: int, nb: int, h: int, w: int, t1, x, out, t1n, w2, b2, w3, b3, w1n=None, b1n=None, ds_cin: int = 0,
                    out_step: int = 1, w2_frags=None):
        """Kernel-level entry of the fused bottleneck chain (csrc/fused.hip); all tensors already on the device.
        out_step = 2: the last block of a stage, evaluated at the even positions only (out is the compact grid).
        w2_frags: `weight_frags` of the conv2 matrix: selects the spatial-tile form where it applies (planes 64, 55 x 55)."""
        self._check(self.lib.avcer_bneck_chain(self.ctx, planes, nb, h, w, _ptr(t1), _ptr(x), int(ds_cin), int(out_step), _ptr(out),
                                               _ptr(t1n), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(w1n), _ptr(b1n),
                                               _ptr(w2_frags), self._stream()))

    def bneck_tail(self, planes: int, m: int, t2, x, out, t1n, w3, b3, w1n, b1n):
        """Kernel-level entry of the stage-3 tail (csrc/fused.hip bneck_tail2_kernel); all tensors already on the device: t2 sp32
        [m,256], x / out sp32 [m,1024], t1n sp32 [m,256]; w3 [1024,256] and w1n [256,1024] from `split_weight_rows`."""
        self._check(self.lib.avcer_bneck_tail(self.ctx, int(planes), int(m), _ptr(t2), _ptr(x), _ptr(out), _ptr(t1n), _ptr(w3),
                                              _ptr(b3), _ptr(w1n), _ptr(b1n), self._stream()))

    def bneck_chain_keep(self, planes: int, nb: int, h: int, w: int, t1, x, out, t1n, w2, b2, w3, b3, w1n, b1n, keep: int, w2_frags=None):
        """`bneck_chain` (no downsample, out_step 1, with a next conv1) with a row-keep step for `out`: keep = 2 stores only the rows
        at even (y, x) of every image and leaves the others as they are; keep = 1 is `bneck_chain`."""
        self._check(self.lib.avcer_bneck_chain_keep(self.ctx, planes, nb, h, w, _ptr(t1), _ptr(x), _ptr(out), _ptr(t1n), _ptr(w2), _ptr(b2),
                                                    _ptr(w3), _ptr(b3), _ptr(w1n), _ptr(b1n), _ptr(w2_frags), int(keep), self._stream()))

    def bneck_tail_keep(self, planes: int, nb: int, h: int, w: int, t2, x, out, t1n, w3, b3, w1n, b1n, keep: int):
        """`bneck_tail` on nb images of h x w positions (m = nb * h * w) with the same row-keep step for `out`."""
        self._check(self.lib.avcer_bneck_tail_keep(self.ctx, int(planes), nb, h, w, _ptr(t2), _ptr(x), _ptr(out), _ptr(t1n), _ptr(w3),
                                                   _ptr(b3), _ptr(w1n), _ptr(b1n), int(keep), self._stream()))

    def dwsep(self, x, dw_w, dw_s, dw_b, pw_w, pw_s, pw_b, stride: int, mode: int = MODE_FP32):
        """Kernel-level entry of one conv_dw block of MobileNet-0.25 (csrc/mnet.hip): x f32 NHWC [nb,h,w,cin], dw_w [9,cin],
        pw_w f32 [cout,cin] (padded and, in MODE_F16X3, split here) -> y f32 NHWC [nb,ceil(h/stride),ceil(w/stride),cout]."""
        x = self._dev(x, torch.float32)
        nb, h, w, cin = (int(v) for v in x.shape)
        pw = self._dev(pw_w, torch.float32)
        cout = int(pw.shape[0])
        pad = torch.zeros((cout + 63) // 64 * 64, (cin + 31) // 32 * 32, dtype=torch.float32, device=self.device)
        pad[:cout, :cin] = pw
        wdev = self.split_weight_rows(pad) if mode == MODE_F16X3 else pad
        args = [self._dev(t, torch.float32) for t in (dw_w, dw_s, dw_b, pw_s, pw_b)]
        y = self._new(nb, (h - 1) // stride + 1, (w - 1) // stride + 1, cout)
        self._check(self.lib.avcer_dwsep(self.ctx, cin, cout, int(stride), int(mode), nb, h, w, _ptr(x), _ptr(args[0]), _ptr(args[1]),
                                         _ptr(args[2]), _ptr(wdev), _ptr(args[3]), _ptr(args[4]), _ptr(y), self._stream()))
        return y

    # kernel-level entries of csrc/s3fd.hip.  `sp32` = the activations are sp32 storage (int16 tensors of twice the channels,
    # avcer_amd/sp32.py) instead of f32
    def s3fd_stem(self, frames_u8, wt, bias, rgb: bool = False, sp32: bool = False):
        """u8 frames [n,h,w,3] -> ReLU(conv1_1 of RGB pixel - (123, 117, 104)) as NHWC [n,h,w,64]; wt f32 [27,64], bias [64]."""
        x = self._dev(frames_u8, torch.uint8)
        n, h, w = (int(v) for v in x.shape[:3])
        wt, bias = self._dev(wt, torch.float32), self._dev(bias, torch.float32)
        y = self._new(n, h, w, 128, dtype=torch.int16) if sp32 else self._new(n, h, w, 64)
        self._check(self.lib.avcer_s3fd_stem(self.ctx, _ptr(x), n, h, w, 1 if rgb else 0, _ptr(wt), _ptr(bias), _ptr(y), 2 if sp32 else 0,
                                             self._stream()))
        return y

    def maxpool2(self, x, ceil_mode: bool = False, sp32: bool = False):
        """nn.MaxPool2d(2, 2, ceil_mode=ceil_mode) on NHWC x [n,h,w,c] (f32, or int16 [n,h,w,2c] sp32)."""
        x = self._dev(x, torch.int16 if sp32 else torch.float32)
        n, h, w = (int(v) for v in x.shape[:3])
        c = int(x.shape[3]) // (2 if sp32 else 1)
        oh, ow = ((h + 1) // 2, (w + 1) // 2) if ceil_mode else (h // 2, w // 2)
        if oh < 1 or ow < 1:
            raise ValueError(f"maxpool2: a {h} x {w} map has no 2 x 2 window")
        y = torch.empty(n, oh, ow, int(x.shape[3]), dtype=x.dtype, device=self.device)
        self._check(self.lib.avcer_maxpool2(self.ctx, _ptr(x), _ptr(y), n, h, w, c, int(ceil_mode), 2 if sp32 else 0, self._stream()))
        return y

    def s3fd_head(self, x, wt, bias, l2norm: bool, sp32: bool = False):
        """One S3FD level's heads: NHWC x [nb,h,w,c] (f32, or int16 [nb,h,w,2c] sp32), wt f32 [9,c,8 or 6], bias -> (loc [nb,h*w,4],
        conf [nb,h*w,2] softmaxed); `l2norm`: every tap is divided by its position's L2 norm + 1e-10."""
        x = self._dev(x, torch.int16 if sp32 else torch.float32)
        nb, h, w = (int(v) for v in x.shape[:3])
        c = int(x.shape[3]) // (2 if sp32 else 1)
        wt, bias = self._dev(wt, torch.float32), self._dev(bias, torch.float32)
        loc, conf = self._new(nb, h * w, 4), self._new(nb, h * w, 2)
        inv = self._new(nb * h * w) if l2norm else None
        self._check(self.lib.avcer_s3fd_head(self.ctx, _ptr(x), 2 if sp32 else 0, _ptr(inv), _ptr(wt), _ptr(bias), nb, h, w, c,
                                             int(wt.shape[2]), 0, h * w, _ptr(loc), _ptr(conf), self._stream()))
        return loc, conf

    def attention(self, qkv, out, n: int, s: int, heads: int, head_dim: int, scale: float, in_kind: int, out_kind: int):
        """Kernel-level entry of the attention kernel: qkv [n, s, 3 * heads * head_dim] -> out [n, s, heads * head_dim];
        storage kinds 0 = f32, 1 = bf16, 2 = sp32 (int16 tensor of twice the elements)."""
        self._check(self.lib.avcer_attention(self.ctx, _ptr(qkv), _ptr(out), n, s, heads, head_dim, float(scale), in_kind,
                                             out_kind, self._stream()))

    def attention_long(self, qkv, out, n: int, s: int, heads: int, head_dim: int, scale: float, in_kind: int, out_kind: int):
        """The same for 1 <= s <= 5000 (avcer_attention_long): the kernels that stream key tiles through LDS, at any s."""
        self._check(self.lib.avcer_attention_long(self.ctx, _ptr(qkv), _ptr(out), n, s, heads, head_dim, float(scale), in_kind,
                                                  out_kind, self._stream()))

    def measure_ceilings(self):
        """(f16 MFMA TFLOP/s of a register-only v_mfma_f32_16x16x32_f16 loop, TB/s of a 1 GiB streaming copy) measured on this GPU."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.avcer_measure_ceilings(self.ctx, C.byref(a), C.byref(b), self._stream()))
        return a.value, b.value

    def stem_pool(self, planes_hi_lo, w_split, scale, bias, n: int):
        """Kernel-level entry of the fused stem (csrc/fused.hip): planes int16 [2, n, 230, 230, 4] (fp16 hi plane, lo plane)
        -> sp32 [n, 55, 55, 64] as int16 [n, 55, 55, 128]."""
        planes = self._dev(planes_hi_lo, torch.int16)
        if tuple(planes.shape) != (2, n, 230, 230, 4):
            raise ValueError("stem_pool: planes [2, n, 230, 230, 4] int16 (fp16 bits)")
        y = torch.empty(n, 55, 55, 128, dtype=torch.int16, device=self.device)
        self._check(self.lib.avcer_stem_pool(self.ctx, _ptr(planes), n * 230 * 230 * 4 * 2, _ptr(w_split), _ptr(scale), _ptr(bias),
                                             _ptr(y), n, self._stream()))
        return y

    def stem_pool_u8(self, frames_u8, w_split, scale, shifts9):
        """The fused stem fed with u8 frames [n, h, w, 3] RGB (preprocessing inside, raw pixels as exact fp16 operands);
        shifts9 f32 [9, 64] from packing.stem_border_shifts.  -> sp32 [n, 55, 55, 64] as int16 [n, 55, 55, 128]."""
        fr = self._dev(frames_u8, torch.uint8)
        n, h, w = int(fr.shape[0]), int(fr.shape[1]), int(fr.shape[2])
        y = torch.empty(n, 55, 55, 128, dtype=torch.int16, device=self.device)
        self._check(self.lib.avcer_stem_pool_u8(self.ctx, _ptr(fr), n, h, w, _ptr(w_split), _ptr(scale), _ptr(shifts9), _ptr(y),
                                                self._stream()))
        return y

    def gemm_stats(self, reset: bool = True):
        n, f = C.c_int64(0), C.c_double(0.0)
        self._check(self.lib.avcer_gemm_stats(self.ctx, C.byref(n), C.byref(f), int(reset)))
        return n.value, f.value
