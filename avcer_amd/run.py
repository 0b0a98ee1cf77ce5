"""`run.run_inference` (src/run.py:190-303) on in-memory inputs: face detection and tracking, visual models on the
first track, audio model over sliding windows, compound-expression fusion.

What the reference does through files -- cv2.VideoCapture frames, JPEG crops under `<save>/<video>/00/`, an ffmpeg
wav at 16 kHz, CSV tables when `flag_save_prob` -- is replaced by arrays: decoded BGR frames `[T,H,W,3]` u8 and a mono
waveform at 16 kHz -- or the source audio as it lies in the WAV file, with its rate (`wav_sr`) -- go in; per-frame predictions
come out.  Grad-CAM heat maps (`flag_heatmaps`) come back as arrays and are written as JPEG files when a results path is given.
The result video (`path_save_video`) is drawn on the device and written as a Motion-JPEG AVI file (avcer_amd/annotate.py); the
prediction timeline chart (`flag_save_plot_pred`) is drawn there too and written as a JPEG file (avcer_amd/chart.py), PIL's
pixels, not matplotlib's.
"""
from __future__ import annotations

import os
import time
from typing import Optional, Sequence

import numpy as np
import torch

from . import io_formats
from .audio_pipeline import audio_forward, check_window, replicate_per_frame, resample_plan
from .engine import MODE_DEFAULT
from .face_tiles import (VideoTiler, check_detect_size, check_tracks, check_via_jpeg, face_crop_paths, pass_rects, roundtrip_face_tiles,
                         scaled_detector, select_tracks, track_clip, write_face_crops)
from .fusion import MODEL_ORDER, fuse, fuse_tracks
from .video_pipeline import tracks_plan, visual_forward, visual_from_static, visual_from_static_tracks


def run_inference_file(engine, path, detector=None, detections: Optional[Sequence[np.ndarray]] = None, fps: Optional[float] = None,
                       frames_per_pass: int = 64, stream_frames: Optional[int] = None, audio_windows_per_pass: int = 128, **kw):
    """`run_inference` on a recording: the reference's first line, `VideoPredictor.process` opening a video file
    (data/get_face_images.py:19-24, 44-47), for the one container this project reads without a decoder library -- the Motion-JPEG /
    PCM AVI file that `ffmpeg -i clip.mp4 -c:v mjpeg -q:v 2 -c:a pcm_s16le -ar 44100 -ac 2 clip.avi` writes (avcer_amd/avi.py).
    open_avi -> jpeg.decode_frames (the frames are decoded on the device and never exist on the host) ->
    run_inference(engine, frames, avi.pcm, fps, wav_sr=avi.audio_rate, name_video=<stem of path>, **kw).
    `fps` defaults to int(rate / scale), what int(cv2.CAP_PROP_FPS) gives the reference (get_face_images.py:23).
    A file without an audio stream raises ValueError unless `wav=` (with `wav_sr=`, or mono at `sr`) is passed; a rate pair the
    resampler does not cover raises before any decode, as in run_inference; what the container refuses: avi.open_avi.
    Each frame is PIL's decode of it (libjpeg-turbo), bit for bit; cv2 reads Motion-JPEG through ffmpeg's own decoder and colour
    conversion, which is not among this project's dependencies and is not claimed.
    `path_save_video=`: the result video (run_inference) with the source's own rate / scale pair and its PCM: the output has the
    source's timing and sound, sample for sample.
    `stream_frames`: None (the default) decodes the whole file onto the device and calls run_inference, so memory grows with the
    recording (6.2 MB per 1920 x 1080 frame, and the detector's outputs as much again).  An integer N >= 1 runs the file through the
    same pipeline in passes of N frames instead (_run_streamed): at most N decoded frames -- one pass buffer, decode and compute are
    not overlapped -- are alive on the device, whatever the length, and the dict, the CSV files, the face folders, the heat maps and
    the result video are the in-memory call's, bit for bit.  Only the PCM of the whole file stays on the device (30 minutes of
    44.1 kHz stereo: 318 MB), and the audio windows go through the model `audio_windows_per_pass` at a time (streamed calls only).
    With `path_save_video` the file is decoded a second time behind the fusion, which the labels need.  "No face track 00" is
    known at the end of the sweep and raises the same FileNotFoundError there.  Anything but None or an int >= 1 (0, a negative, a
    bool, a float) raises ValueError naming stream_frames before the file is opened.  run_dataset / video_job_from_avi stay
    in-memory.
    `tracks=` (run_inference) is refused, where it is refused, before the file is opened, and holds for both paths: streamed, a
    named track that never appeared raises its FileNotFoundError at the end of the sweep, as "no face track 00" does.
    `detect_size=` / `detect_filter=` (run_inference) hold for both paths too: a bad value is refused before the file is opened, an
    upscale once the container has named the frame size, before any decode; streamed, every pass is resized on its own (there is no
    state across frames), so the results are the in-memory call's.
    `flag_save_plot_pred=` (run_inference) holds for both paths: what it refuses is refused before the file is opened; streamed, the
    chart is made behind the last pass from the class tables the call keeps anyway, and the file is the in-memory call's.
    Returns run_inference's dict; `real_time_factor` includes demux and decode."""
    from . import jpeg
    from .avi import open_avi

    if stream_frames is not None and (isinstance(stream_frames, (bool, np.bool_)) or not isinstance(stream_frames, (int, np.integer))
                                      or stream_frames < 1):
        raise ValueError(f"stream_frames must be None or an integer >= 1, not {stream_frames!r}")
    if isinstance(audio_windows_per_pass, (bool, np.bool_)) or not isinstance(audio_windows_per_pass, (int, np.integer)) or audio_windows_per_pass < 1:
        raise ValueError(f"audio_windows_per_pass must be an integer >= 1, not {audio_windows_per_pass!r}")
    check_tracks(kw.get("tracks"), kw.get("flag_heatmaps", False))
    check_detect_size(kw.get("detect_size"), kw.get("detect_filter", "bilinear"), detector, detections)
    _check_plot(kw.get("flag_save_plot_pred", False), kw.get("path_save_results", ""), kw.get("ce_weights_type", True), kw.get("ce_mask", False),
                kw.get("plot_size", (200, 1200)))
    start_time = time.time()
    with open_avi(path) as avi:
        check_detect_size(kw.get("detect_size"), kw.get("detect_filter", "bilinear"), detector, detections, (avi.height, avi.width))
        if "wav" in kw:
            wav, wav_sr = kw.pop("wav"), kw.pop("wav_sr", None)
        elif avi.pcm is None:
            raise ValueError(f"{avi.path}: no audio stream (pass wav= and wav_sr= to give the audio some other way)")
        else:
            wav, wav_sr = avi.pcm, kw.pop("wav_sr", avi.audio_rate)
        if wav_sr is not None:
            resample_plan(wav_sr, kw.get("sr", 16000))
        check_window(engine, kw.get("window", 4), kw.get("sr", 16000))
        if detections is None and detector is None:
            raise ValueError("give a detector or the per-frame detections")
        fps = int(avi.rate / avi.scale) if fps is None else fps
        if stream_frames is not None:
            kw.setdefault("name_video", os.path.splitext(os.path.basename(os.fspath(path)))[0])
            if kw.get("path_save_video"):
                kw.setdefault("video_timing", (avi.rate, avi.scale))
            return _run_streamed(engine, avi, wav, wav_sr, fps, detector, detections, int(stream_frames), int(audio_windows_per_pass),
                                 frames_per_pass, start_time, **kw)
        frames, _ = jpeg.decode_frames(engine, avi.frames, avi.height, avi.width, bgr=True, frames_per_pass=frames_per_pass)
        n_frames = avi.n_frames
        timing = (avi.rate, avi.scale)
    kw.setdefault("name_video", os.path.splitext(os.path.basename(os.fspath(path)))[0])
    if kw.get("path_save_video"):
        kw.setdefault("video_timing", timing)  # the source's own rate / scale pair, not the rounded fps
    out = run_inference(engine, frames, wav, fps, detector=detector, detections=detections, wav_sr=wav_sr, **kw)
    duration = n_frames / fps if (fps and fps > 0 and n_frames > 0) else None
    out["real_time_factor"] = (time.time() - start_time) / duration if duration else None
    return out


def run_inference(engine, frames_bgr, wav, fps: float, detector=None, detections: Optional[Sequence[np.ndarray]] = None,
                  path_save_results: str = "", name_video: str = "video", flag_save_prob: bool = False,
                  weights_prob_model=None, weights_model=(1, 1, 1), ce_weights_type: bool = True, ce_mask: bool = False,
                  sr: int = 16000, window: float = 4, step: float = 0.5, padding: str = "mean", mode: int = MODE_DEFAULT,
                  flag_heatmaps: bool = False, model_heatmaps: str = "static", wav_sr: Optional[int] = None,
                  path_save_faces: Optional[str] = None, jpeg_entropy: str = "host", faces_via_jpeg: bool = False,
                  path_save_video: Optional[str] = None, video_model: str = "av", video_quality: int = 90, video_panel: bool = False,
                  video_timing: Optional[Sequence[int]] = None, tracks=None, detect_size=None, detect_filter: str = "bilinear",
                  flag_save_plot_pred: bool = False, plot_size: Sequence[int] = (200, 1200)):
    """engine: an `Engine` with the static, dynamic and audio weights loaded.  frames_bgr u8 [T,H,W,3] as cv2 decodes
    them; wav float32 [L] mono at `sr`; fps as `int(cv2.CAP_PROP_FPS)` gives it (get_face_images.py:23).
    `wav_sr`: `wav` is source audio at that rate instead -- int16 [L] / [L, C] as the frames lie in the WAV file ffmpeg writes
    (44.1 kHz stereo, data/utils.py:46) or float32 [L] / [C, L] -- and is converted, downmixed and resampled to `sr` on the device,
    on the audio stream in front of the chunker (data/utils.py:50-57, Engine.resample).  A rate pair the kernel does not cover
    raises ValueError before any work, and so does a `window` of more tokens than the loaded audio model accepts
    (Engine.load_audio(sd, max_tokens=...); the message names max_tokens).
    `detector`: a `face_tiles.RetinaFacePredictor` or `face_tiles.S3FDPredictor` (threshold 0.8 in the reference); or pass per-frame `detections`.
    Defaults follow `run_inference`'s signature (Rule 2 weights on, Rule 1 mask off; `run.py --help` flips them).
    Returns a dict: av / vs / vd / a predictions (int32 [T], compound class per frame), `compound_prob` f64 [4,T,7],
    `static_probs`, `dynamic_logits` [T,7], `audio_rows` / `audio_frames` (the audio table), `records` (face files),
    `real_time_factor` (elapsed / video duration, the figure run.py:307 prints).
    `flag_heatmaps` (run.py:231-239, get_prob_video.py:135-155): `out["heatmaps"]` = (frame_idx int32 [m], overlays u8
    [m,224,224,3] BGR), one Grad-CAM overlay per frame of track 00 that starts an LSTM evaluation, of the static softmax of the
    class the static or the dynamic model (`model_heatmaps`) chose; the base image is the crop cut from the frames on the device
    and resized with cv2's INTER_LINEAR.  Written as `<path_save_results>/<name_video>/heatmaps_<model>/NNNNNN.jpg` when
    `path_save_results` is given.  A `model_heatmaps` other than "static" / "dynamic" raises ValueError before any work (the
    reference dies with UnboundLocalError at its first heat-map frame).
    `path_save_faces`: stage 0's output on disk as well (get_face_images.py:52-63): every detection's crop as
    `<path_save_faces>/<name_video>/<track:02d>/<frame:06d>.jpg`, encoded from the frames on the device
    (face_tiles.write_face_crops); `out["face_files"]` lists the paths in record order.  Off by default.
    `jpeg_entropy`: where those files are Huffman-coded, "host" (the default) or "device" (jpeg.encode_images); the files are the
    same.  Any other value raises ValueError before any work.
    `faces_via_jpeg`: the visual models see every face crop as the reference's stage 1 does -- read back from the JPEG file stage 0
    writes of it (quality 95, 4:2:0; get_face_images.py:52-63, get_prob_video.py:93-109) -- instead of the raw crop: the results
    are then, bit for bit in the same arithmetic mode, those of `preprocess_video_and_predict` on the folder `path_save_faces`
    writes.  Computed on the device without the files (jpeg.roundtrip_tiles); with `path_save_faces` the files are packed from the
    same pass's coefficients, with `flag_heatmaps` the base image is the linear resize of the round-tripped crop
    (data/utils.py:105).  Off by default: nothing changes then.  Anything but a bool raises ValueError before any work.
    `path_save_video`: the result video (video/visualization.py, get_visualization.py:40-118) as a Motion-JPEG AVI file at that
    path, written behind the fusion from what is already on the device (annotate.write_result_video: every record's box, the label
    "<class>: <p>%" of `video_model`'s prediction on track 00, with `video_panel` a bar per class in the top left corner; JPEG
    quality `video_quality`); `out["result_video"]` is the path.  The frame rate is `fps` (or `video_timing` = the container's exact
    (rate, scale) pair); the sound is `wav` when it was given as int16 source audio with `wav_sr`, else there is none.  The
    drawing is PIL's ImageDraw, bit for bit, not cv2's.  `video_model`: "av", "vs", "vd" or "a"; anything else raises ValueError
    before any work.  Off by default: nothing changes then.
    `tracks`: which face tracks the visual models and the fusion run on.  None (the default): track directory 00 alone, as the
    reference (get_prob_video.py:79-94 walks `<faces>/00/`; get_face_images.py:73-76 leaves choosing a "target face" among the
    folders to the user) -- today's call, unchanged.  "all": every track directory stage 0 writes, ascending.  A list of distinct
    ints >= 0: those directories (tid - 1, the folder numbers), in that order.  Every selected track is treated as the reference
    would treat it were its folder named `00` -- its own present mask, hold / zero / reset rule and LSTM windows
    (video_pipeline.tracks_plan); the audio table is the video's -- and its tables are, bit for bit, what
    `visual_forward(engine, *track_clip(records, tiles, k, T), fps, mode)` and `fusion.fuse` on them give.  Detector, tracker,
    crops and the audio branch run once; ONE static CNN call takes the selected tracks' tiles, ONE LSTM call all their windows, ONE
    fusion launch a segment per track (fusion.fuse_tracks); the range contract is read once for all of it.
    `out["tracks"]` = {track: dict of av / vs / vd / a / compound_prob / static_probs / dynamic_logits / present (bool [T])} in the
    order selected; the top-level keys are the FIRST selected track's (`audio_rows`, `audio_frames`, `records`, `face_files` are the
    video's, as ever).  `flag_save_prob` writes the first track under today's names and every other track k through the same
    writers as the video `<name_video>__t<kk>`; the result video labels every selected track from its own prediction, the panel
    shows the first.  A named track without a record raises FileNotFoundError naming it before the visual models run, "all" without
    any record the same; anything that is not None, "all" or such a list, and `flag_heatmaps` together with `tracks` (heat maps
    stay with track 00), raises ValueError before any work.
    `detect_size`: the detector runs on a smaller copy of the frames -- (height, width), or an int = the longest side -- resized on
    the device with `detect_filter` ("box", "bilinear", "bicubic" or "lanczos": PIL's Image.resize, bit for bit; resize.py), and
    its rows are mapped back to source pixels (face_tiles.ScaledDetector wraps `detector`); tracker, rectangles and crops stay at
    full resolution.  The reference detects on whole frames (get_face_images.py:50): this departs from it on purpose, for HD
    material, where the detector's cost grows with the pixel count.  None (the default): no wrapper is constructed and nothing
    changes.  A size that shrinks neither side passes the frames straight through.  A value that is neither, an unknown filter, a
    target larger than the frames, and `detect_size` beside `detections=` without a detector raise ValueError before any work.
    `flag_save_plot_pred` (run.py:272-296, visualize.py:175-215): the prediction timeline chart, the compound class of AV, VS, VD
    and A against the frame number, written as `<path_save_results>/pedicted_CEs_Rule N.jpg` (the reference's spelling; N = 2 with
    `ce_weights_type`, else 1 with `ce_mask`, as run.py:281-284 picks it); `out["plot_pred"]` is the path.  `plot_size` = (height,
    width) of the picture.  Drawn on the device from the class tables where the fusion left them (chart.write_charts: one
    avcer_chart_series call, one annotate call, the JPEG encoder) -- the tables are not copied to the host for it.  With `tracks`
    one chart per selected track in that one call: the first under the name above, every other track k as
    `pedicted_CEs_Rule N__t<kk>.jpg`, and `out["tracks"][k]["plot_pred"]` holds its path.  The pixels are PIL's (ImageDraw.line,
    ImageDraw.bitmap, Image.save), bit for bit; matplotlib's are not claimed.  The reference switches this on by default; here it
    is off unless asked for, like every option, and nothing changes then.  Without `path_save_results`, with neither `ce_mask` nor
    `ce_weights_type` (the reference dies on an unbound `rule`), and with a `plot_size` that leaves no plot rectangle, ValueError
    before any work."""
    tracks = check_tracks(tracks, flag_heatmaps)
    plot = _check_plot(flag_save_plot_pred, path_save_results, ce_weights_type, ce_mask, plot_size)
    hm = _check_options(engine, video_model, jpeg_entropy, faces_via_jpeg, flag_heatmaps, model_heatmaps, window, sr)
    check_detect_size(detect_size, detect_filter, detector, detections, None if np.ndim(frames_bgr) != 4 else tuple(frames_bgr.shape[1:3]))
    detector = scaled_detector(detector, detect_size, detect_filter)
    start_time = time.time()                                                # run.py:200
    frames = frames_bgr if torch.is_tensor(frames_bgr) else torch.from_numpy(np.ascontiguousarray(frames_bgr))
    total_frames = int(frames.shape[0])
    # the duration the real-time factor divides by, settled before any work is queued: `int(cv2.CAP_PROP_FPS)` is 0 on a
    # broken container, and a finished prediction must not be lost to a ZeroDivisionError in the last statement
    duration = total_frames / fps if (fps and fps > 0 and total_frames > 0) else None
    if detections is None and detector is None:
        raise ValueError("give a detector or the per-frame detections")
    if wav_sr is None:
        wav_t = wav if torch.is_tensor(wav) else torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    else:
        resample_plan(wav_sr, sr)
        wav_t = wav if torch.is_tensor(wav) else torch.from_numpy(np.ascontiguousarray(wav))
    dev = engine.device
    wav_t = wav_t.to(dev)
    main, side = torch.cuda.current_stream(dev), _side_stream(engine)
    host = {}  # detector / tracker / crop results: independent of the arithmetic mode, computed once

    def gpu_work(m):
        # (1) the audio branch depends on nothing of the visual one: it is queued FIRST, on its own stream, and runs while
        #     the host walks the tracker loop below (750 numpy + linear_sum_assignment iterations for a 30 s video)
        side.wait_stream(main)
        wav_t.record_stream(side)  # allocated on `main`: the allocator must not hand it out while `side` still reads it
        joined = False
        try:
            with torch.cuda.stream(side):
                win_logits, lo, hi = audio_forward(engine, wav_t, sr, fps, window, step, padding, m, wav_sr=wav_sr)  # get_prob_audio_8_cl.py:68-138
            # (2) faces -> tracks -> tiles (get_face_images.py:38-63), then the visual models on track 00
            if "clip" not in host:
                dets = detections if detections is not None else detector.batch(frames, rgb=False)  # get_face_images.py:49
                if faces_via_jpeg:
                    records, tiles = VideoTiler(engine).process(frames, dets, path_save_faces or None, name_video if path_save_faces else None,
                                                                entropy=jpeg_entropy, via_jpeg=True)
                    if path_save_faces:
                        host["face_files"] = face_crop_paths(records, path_save_faces, name_video)
                else:
                    records, tiles = VideoTiler(engine).process(frames, dets)
                if path_save_faces and not faces_via_jpeg:
                    host["face_files"] = write_face_crops(engine, frames, records, path_save_faces, name_video, entropy=jpeg_entropy)
                if tracks is not None:
                    # the selected tracks as one ragged set of clips: their tiles alone, track after track (no dense clip per track)
                    tp = tracks_plan(records, select_tracks(records, tracks), total_frames, fps)
                    host["records"], host["tracks_plan"] = records, tp
                    host["clip"] = (tiles if len(tp.rows) == len(tiles) and (np.diff(tp.rows) == 1).all() else
                                    tiles.index_select(0, torch.from_numpy(tp.rows).to(dev)), tp)
                else:
                    if not (len(records) and (records[:, 1] == 0).any()):
                        raise FileNotFoundError("no face track 00 (os.listdir(<faces>/00) fails in the reference, get_prob_video.py:79)")
                    host["records"] = records
                    host["clip"] = track_clip(records, tiles, 0, total_frames)
            clip, present = host["clip"]
            maps = None
            if tracks is not None:
                # ONE static CNN sweep over all tracks' tiles, ONE LSTM call over all tracks' windows (video_pipeline.tracks_plan)
                _, probs, feats = engine.static_forward(clip, m)
                static_probs, dynamic_logits = visual_from_static_tracks(engine, probs, feats, present, fps, m)
            elif flag_heatmaps:
                static_probs, dynamic_logits, cam, fidx, rows, cls = hm.visual_forward_cam(engine, clip, present, fps, m, model_heatmaps)
                if len(rows):
                    recs = host["records"]
                    r00 = recs[recs[:, 1] == 0]
                    at = {int(f): k for k, f in enumerate(r00[:, 0])}
                    pick = r00[[at[int(f)] for f in fidx]]
                    rects = torch.from_numpy(pick[:, [0, 2, 3, 4, 5]].astype(np.int32))
                    if faces_via_jpeg:  # cv2.resize of the read-back crop (get_prob_video.py:99-100, data/utils.py:105)
                        from . import jpeg

                        base = engine.crop_resize_linear(*jpeg.roundtrip_canvas(engine, frames, rects, bgr=True), swap_rb=False)
                    else:
                        base = engine.crop_resize_linear(frames, rects, swap_rb=True)
                    maps = (fidx, engine.cam_render(cam, rows, cls, base, hm.JET_BGR, hm.IMAGE_WEIGHT))
                else:
                    maps = (fidx, torch.zeros((0, 224, 224, 3), dtype=torch.uint8, device=dev))
            else:
                static_probs, dynamic_logits = visual_forward(engine, clip, present, fps, m)         # get_prob_video.py:67-204
            # (3) fusion last, behind both branches; nothing has been copied to the host yet
            main.wait_stream(side)
            joined = True
            win_logits.record_stream(main)
            prob, am = (fuse if tracks is None else fuse_tracks)(engine, static_probs, dynamic_logits, win_logits, lo, hi, weights_prob_model,
                                                                 weights_model, ce_weights_type, ce_mask)  # run.py:25-189
            return static_probs, dynamic_logits, win_logits, lo, hi, prob, am, maps
        finally:
            # the reference's failure paths (no face track, a detector error) unwind from here: the audio branch already queued
            # on `side` is joined all the same, so that no launch of this video outlives the call (its workspace and the
            # range-contract counter belong to the next one)
            if not joined:
                main.wait_stream(side)

    # MODE_F16X3: one read of the range-contract counter behind the last launch; a video during which an activation left fp16's
    # range is run again in MODE_FP32 (engine.guarded)
    out = _results(engine, engine.guarded(mode, gpu_work), host, frames, wav, wav_sr, fps, path_save_results, name_video, flag_save_prob, model_heatmaps, path_save_video, video_model, video_quality,
                   video_panel, video_timing, plot)
    # "Real-time factor for compound expression prediction" as run.py:304-307 prints it: elapsed / video duration (the
    # device -> host copies above have synchronised the stream, so the clock covers all the work); None where the
    # container reported no frame rate
    out["real_time_factor"] = (time.time() - start_time) / duration if duration else None
    return out


def _check_options(engine, video_model, jpeg_entropy, faces_via_jpeg, flag_heatmaps, model_heatmaps, window, sr):
    """What run_inference refuses before any work, in its order; returns the heat-map module when `flag_heatmaps`, else None."""
    video_models = [m.lower() for m in MODEL_ORDER]
    if video_model not in video_models:
        raise ValueError(f"video_model must be one of {' / '.join(video_models)}, not {video_model!r}")
    if jpeg_entropy not in ("host", "device"):
        raise ValueError(f'jpeg_entropy must be "host" or "device", not {jpeg_entropy!r}')
    check_via_jpeg(faces_via_jpeg)
    hm = None
    if flag_heatmaps:
        from . import heatmaps as hm

        hm.check_model(model_heatmaps)
    check_window(engine, window, sr)
    return hm


def _check_plot(flag_save_plot_pred, path_save_results, ce_weights_type, ce_mask, plot_size):
    """`flag_save_plot_pred` off (the default): None, and the chart module is not even imported.  On: what chart.check_plot_pred
    refuses is refused here, before any work; returns (rule, (height, width))."""
    if flag_save_plot_pred is False:
        return None
    from .chart import check_plot_pred

    return check_plot_pred(flag_save_plot_pred, path_save_results, ce_weights_type, ce_mask, plot_size)


def _side_stream(engine):
    """The engine's second stream: the audio branch runs on it beside the visual one."""
    side = engine.__dict__.get("_side_stream")
    if side is None:
        side = engine.__dict__["_side_stream"] = torch.cuda.Stream(engine.device)
    return side


def _results(engine, res, host, frames, wav, wav_sr, fps, path_save_results, name_video, flag_save_prob, model_heatmaps, path_save_video,
             video_model, video_quality, video_panel, video_timing, plot=None):
    """Everything behind the guarded device work, for the in-memory and the streamed call alike: the tables to the host, the CSV
    files, the heat-map files, the result video, the prediction chart (`plot`: _check_plot's pair).  `res` is gpu_work's tuple; `frames`: the decoded frames, or -- streamed -- a
    callable that yields them once more in passes (annotate.write_result_video)."""
    static_probs, dynamic_logits, win_logits, lo, hi, prob, am, maps = res
    records = host["records"]
    rows, aud_frames = replicate_per_frame(win_logits.cpu().numpy(), lo, hi)
    tp = host.get("tracks_plan")
    plot_files = None
    if plot is not None:
        # am int32 [4, T], or [4, K, T] with tracks: K charts back to back in ONE call, read where the fusion left them
        from . import chart

        n_frames = int(am.shape[-1])
        plot_files = chart.plot_paths(path_save_results, plot[0], None if tp is None else tp.tracks)
        chart.write_charts(engine, am.reshape(am.shape[0], -1), plot_files, T=[n_frames] * len(plot_files),
                           plan=chart.chart_plan(n_frames, width=plot[1][1], height=plot[1][0]))
    am, prob, static_probs, dynamic_logits = am.cpu().numpy(), prob.cpu().numpy(), static_probs.cpu().numpy(), dynamic_logits.cpu().numpy()
    per_track = None
    if tp is not None:
        # [.., K, T, ..] tables of the selected tracks: a dict per track; the first one is the call's top level, under today's names
        per_track = {}
        for i, k in enumerate(tp.tracks):
            one = {name.lower(): am[j, i].copy() for j, name in enumerate(MODEL_ORDER)}
            one.update(compound_prob=prob[:, i].copy(), static_probs=static_probs[i].copy(),
                       dynamic_logits=dynamic_logits[i].copy(), present=tp.present[i].copy())
            per_track[k] = one
        # the top level holds arrays of its own, as with tracks=None: editing one in place leaves out["tracks"] alone
        first = per_track[tp.tracks[0]]
        am, prob = np.stack([first[name.lower()] for name in MODEL_ORDER]), first["compound_prob"].copy()
        static_probs, dynamic_logits = first["static_probs"].copy(), first["dynamic_logits"].copy()
    if flag_save_prob:
        io_formats.write_visual_csvs(static_probs, dynamic_logits, path_save_results, name_video)
        io_formats.write_audio_csv(rows, aud_frames, path_save_results, "audio", name_video)
        for k in (tp.tracks[1:] if tp is not None else ()):  # the other tracks: the same files, as the video `<name_video>__t<kk>`
            io_formats.write_visual_csvs(per_track[k]["static_probs"], per_track[k]["dynamic_logits"], path_save_results, f"{name_video}__t{k:02d}")
            io_formats.write_audio_csv(rows, aud_frames, path_save_results, "audio", f"{name_video}__t{k:02d}")
    out = {name.lower(): am[i] for i, name in enumerate(MODEL_ORDER)}
    out.update(compound_prob=prob, static_probs=static_probs, dynamic_logits=dynamic_logits, audio_rows=rows, audio_frames=aud_frames,
               records=records)
    if per_track is not None:
        out["tracks"] = per_track
    if plot_files is not None:
        out["plot_pred"] = plot_files[0]
        for k, path in zip(tp.tracks if tp is not None else (), plot_files):
            per_track[k]["plot_pred"] = path
    if "face_files" in host:
        out["face_files"] = host["face_files"]
    if maps is not None:
        from . import heatmaps as hm

        out["heatmaps"] = (maps[0].astype(np.int32), maps[1].cpu().numpy())
        if path_save_results:
            hm.write_heatmaps(hm.heatmap_dir(path_save_results, name_video, model_heatmaps), maps[0], maps[1], engine=engine)
    if path_save_video:
        from fractions import Fraction

        from .annotate import write_result_video

        if video_timing is None:
            fr = Fraction(fps).limit_denominator(100000)
            video_timing = (fr.numerator, fr.denominator)
        pcm = None
        if wav_sr is not None:  # source audio as it lay in the file: muxed sample for sample
            src_wav = wav.cpu().numpy() if torch.is_tensor(wav) else np.asarray(wav)
            pcm = src_wav if src_wav.dtype == np.int16 else None
        video_models = [m.lower() for m in MODEL_ORDER]
        j = video_models.index(video_model)
        if per_track is None:
            pred, prob_model, labelled = out[video_model], out["compound_prob"][j], None
        else:  # a label per selected track, from its own prediction
            pred = {k: one[video_model] for k, one in per_track.items()}
            prob_model = {k: one["compound_prob"][j] for k, one in per_track.items()}
            labelled = tp.tracks
        out["result_video"] = write_result_video(engine, frames, records, pred, prob_model, path_save_video, int(video_timing[0]),
                                                 int(video_timing[1]), pcm=pcm, audio_rate=int(wav_sr) if pcm is not None else 44100,
                                                 quality=video_quality, entropy="device", panel=video_panel, tracks=labelled)
    return out


def _options(**kw):
    """run_inference's keyword options with its own defaults (one statement of them), `kw` laid over; an unknown name is the
    TypeError the call itself would raise."""
    import inspect
    from types import SimpleNamespace

    opts = {k: p.default for k, p in inspect.signature(run_inference).parameters.items() if p.default is not inspect.Parameter.empty}
    unknown = sorted(set(kw) - set(opts))
    if unknown:
        raise TypeError(f"run_inference() got an unexpected keyword argument {unknown[0]!r}")
    opts.update(kw)
    return SimpleNamespace(**opts)


def _run_streamed(engine, avi, wav, wav_sr, fps, detector, detections, stream_frames: int, audio_windows_per_pass: int, frames_per_pass: int,
                  start_time: float, **kw):
    """`run_inference` on the open recording `avi` in passes of `stream_frames` frames (run_inference_file's `stream_frames`): the
    same results, bit for bit, with one pass of decoded frames on the device at a time.

    Per pass: jpeg.decode_frames -> detector (or the pass's slice of `detections`) -> the resumable tracker (Engine.tracker) -> the
    crop rectangles, their frame index rebased to the pass -> crop_tiles / roundtrip_face_tiles / write_face_crops -> the static CNN
    on the pass's tiles of track 00.  Kept between passes: the detections and records (host), and per frame of track 00 the static
    CNN's 7 probabilities and 512 features (2076 bytes); with `flag_heatmaps`, per heat-map frame (one in lstm_step(fps)) its 7
    raw maps [7,7,7] and its base image [224,224,3] -- as large as the overlays that are returned.  Which class a map shows may
    depend on the LSTM ("dynamic"), which runs behind the sweep, so the overlays of both `model_heatmaps` are rendered there, from
    what was kept.  With `tracks` the static CNN takes the pass's tiles of the SELECTED tracks and those 2076 bytes are kept per
    record of a selected track -- with "all" per record, since which tracks there are is known at the end only --, in record
    order; behind the sweep they are gathered track after track as video_pipeline.tracks_plan lays them out.  Behind the last
    pass: video_pipeline.visual_from_static / visual_from_static_tracks (plan_clip's windows over all features, one LSTM call), the
    audio branch joined, fuse (fuse_tracks).  With `path_save_video` the file is decoded a SECOND time, pass by pass, for
    annotate.write_result_video: the labels need the fused predictions.  Decode and compute are not overlapped: one pass buffer is
    alive at a time."""
    from . import jpeg
    from .video_pipeline import lstm_step

    o = _options(**kw)
    tracks = check_tracks(o.tracks, o.flag_heatmaps)
    hm = _check_options(engine, o.video_model, o.jpeg_entropy, o.faces_via_jpeg, o.flag_heatmaps, o.model_heatmaps, o.window, o.sr)
    check_detect_size(o.detect_size, o.detect_filter, detector, detections, (avi.height, avi.width))
    plot = _check_plot(o.flag_save_plot_pred, o.path_save_results, o.ce_weights_type, o.ce_mask, o.plot_size)
    detector = scaled_detector(detector, o.detect_size, o.detect_filter)
    total, height, width, per = avi.n_frames, avi.height, avi.width, int(stream_frames)
    duration = total / fps if (fps and fps > 0 and total > 0) else None
    if detections is not None and len(detections) != total:
        raise ValueError("one detection array per frame")
    dev = engine.device
    wav_t = (wav if torch.is_tensor(wav) else torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32 if wav_sr is None else None))).to(dev)
    main, side = torch.cuda.current_stream(dev), _side_stream(engine)
    save = (o.path_save_faces, o.name_video) if o.path_save_faces else (None, None)
    host = {}  # detections, records and face files of every pass: independent of the arithmetic mode, computed once

    def decode(a):
        return jpeg.decode_frames(engine, avi.frames[a:a + per], height, width, bgr=True, frames_per_pass=frames_per_pass)[0]

    def gpu_work(m):
        side.wait_stream(main)
        wav_t.record_stream(side)
        joined = False
        try:
            with torch.cuda.stream(side):
                win_logits, lo, hi = audio_forward(engine, wav_t, o.sr, fps, o.window, o.step, o.padding, m, wav_sr=wav_sr,
                                                   windows_per_pass=audio_windows_per_pass)
            first = "records" not in host
            if first:
                tracker, passes, files = engine.tracker(0.4, 0.0), [], []  # VideoTiler's tracker
            present = np.zeros(total, dtype=bool)
            every = lstm_step(fps)
            if every <= 0:
                raise ZeroDivisionError("integer division or modulo by zero")  # as plan_clip: `curr_idx_frame % step`
            probs, feats, cams, bases = [], [], [], []
            kept, n_rec = [], 0  # `tracks`: the records (numbered through the video) whose static outputs are kept
            for k, a in enumerate(range(0, total, per)):
                frames = decode(a)
                if first:
                    dets = detections[a:a + per] if detections is not None else detector.batch(frames, rgb=False)
                    records = tracker.push(dets, width, height)
                    passes.append(records)
                else:
                    records = host["passes"][k]
                if len(records):
                    if o.faces_via_jpeg:
                        tiles, paths = roundtrip_face_tiles(engine, frames, records, *(save if first else (None, None)), entropy=o.jpeg_entropy,
                                                            frame_base=a)
                    else:
                        tiles = engine.crop_tiles(frames, torch.from_numpy(pass_rects(records, a).astype(np.int32)), bgr=True)
                        paths = write_face_crops(engine, frames, records, *save, entropy=o.jpeg_entropy, frame_base=a) if first and save[0] else None
                    if first and save[0]:
                        files.extend(paths)
                    if tracks is None:
                        sel = np.flatnonzero(records[:, 1] == 0)
                    else:  # "all": which tracks there are is known at the end only, so every record is kept
                        sel = np.arange(len(records)) if tracks == "all" else np.flatnonzero(np.isin(records[:, 1], tracks))
                    if len(sel):
                        r00 = records[sel]
                        if tracks is None:
                            present[r00[:, 0]] = True
                        else:
                            kept.append(sel + n_rec)
                        tiles00 = tiles if len(sel) == len(records) else tiles.index_select(0, torch.from_numpy(sel).to(dev))
                        if o.flag_heatmaps:
                            _, p, f, cam = engine.static_forward_cam(tiles00, m)
                            pick = np.flatnonzero(r00[:, 0] % every == 0)
                            if len(pick):
                                cams.append(cam.index_select(0, torch.from_numpy(pick).to(dev)))
                                rects = torch.from_numpy(pass_rects(r00[pick], a).astype(np.int32))
                                if o.faces_via_jpeg:  # cv2.resize of the read-back crop, as in run_inference
                                    bases.append(engine.crop_resize_linear(*jpeg.roundtrip_canvas(engine, frames, rects, bgr=True), swap_rb=False))
                                else:
                                    bases.append(engine.crop_resize_linear(frames, rects, swap_rb=True))
                        else:
                            _, p, f = engine.static_forward(tiles00, m)
                        probs.append(p)
                        feats.append(f)
                    del tiles
                    n_rec += len(records)
                del frames
            if first:
                tracker.close()
                records = np.concatenate(passes) if passes else np.zeros((0, 6), dtype=np.int64)
                if save[0]:
                    host["face_files"] = files
                if tracks is not None:
                    host["tracks_plan"] = tracks_plan(records, select_tracks(records, tracks), total, fps)
                elif not present.any():
                    raise FileNotFoundError("no face track 00 (os.listdir(<faces>/00) fails in the reference, get_prob_video.py:79)")
                host["passes"], host["records"] = passes, records
            probs, feats = torch.cat(probs), torch.cat(feats)
            if tracks is not None:
                # what was kept lies in record order; the plan wants it track after track
                tp = host["tracks_plan"]
                pos = np.searchsorted(np.concatenate(kept), tp.rows)
                if len(pos) != len(probs) or (np.diff(pos) != 1).any():
                    pos = torch.from_numpy(pos).to(dev)
                    probs, feats = probs.index_select(0, pos), feats.index_select(0, pos)
                static_probs, dynamic_logits = visual_from_static_tracks(engine, probs, feats, tp, fps, m)
            else:
                static_probs, dynamic_logits, dl = visual_from_static(engine, probs, feats, present, fps, m, with_windows=True)
            maps = None
            if o.flag_heatmaps:
                fidx, rows, win = hm.heatmap_plan(present, fps)
                if len(rows):
                    cls = hm.heatmap_classes(engine, o.model_heatmaps, probs, dl, rows, win)
                    maps = (fidx, engine.cam_render(torch.cat(cams), np.arange(len(rows)), cls, torch.cat(bases), hm.JET_BGR, hm.IMAGE_WEIGHT))
                else:
                    maps = (fidx, torch.zeros((0, 224, 224, 3), dtype=torch.uint8, device=dev))
            main.wait_stream(side)
            joined = True
            win_logits.record_stream(main)
            prob, am = (fuse if tracks is None else fuse_tracks)(engine, static_probs, dynamic_logits, win_logits, lo, hi, o.weights_prob_model,
                                                                 o.weights_model, o.ce_weights_type, o.ce_mask)
            return static_probs, dynamic_logits, win_logits, lo, hi, prob, am, maps
        finally:
            if not joined:  # as in run_inference: no launch of this video outlives the call
                main.wait_stream(side)

    res = engine.guarded(o.mode, gpu_work)
    out = _results(engine, res, host, lambda: (decode(a) for a in range(0, total, per)), wav, wav_sr, fps, o.path_save_results, o.name_video,
                   o.flag_save_prob, o.model_heatmaps, o.path_save_video, o.video_model, o.video_quality, o.video_panel, o.video_timing, plot)
    out["real_time_factor"] = (time.time() - start_time) / duration if duration else None
    return out
