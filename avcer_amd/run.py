"""`run.run_inference` (src/run.py:190-303) on in-memory inputs: face detection and tracking, visual models on the
first track, audio model over sliding windows, compound-expression fusion.

What the reference does through files -- cv2.VideoCapture frames, JPEG crops under `<save>/<video>/00/`, an ffmpeg
wav at 16 kHz, CSV tables when `flag_save_prob` -- is replaced by arrays: decoded BGR frames `[T,H,W,3]` u8 and a mono
waveform at 16 kHz -- or the source audio as it lies in the WAV file, with its rate (`wav_sr`) -- go in; per-frame predictions
come out.  Grad-CAM heat maps (`flag_heatmaps`) come back as arrays and are written as JPEG files when a results path is given.
The result video (`path_save_video`) is drawn on the device and written as a Motion-JPEG AVI file (avcer_amd/annotate.py); the
prediction timeline chart (`flag_save_plot_pred`) is drawn there too and written as a JPEG file (avcer_amd/chart.py), PIL's
pixels, not matplotlib's.

The pipeline is stated once, as a loop over the passes of a frame source (_run): run_inference gives it the frames as one pass,
run_inference_file(stream_frames=N) the open recording in passes of N frames.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import io_formats, jpeg
from .audio_pipeline import audio_forward, check_window, replicate_per_frame, resample_plan
from .engine import MODE_DEFAULT
from .face_tiles import (check_detect_size, check_tracks, check_via_jpeg, pass_rects, pass_tiles, roundtrip_face_tiles, scaled_detector,
                         select_tracks, track_pass, write_face_crops)
from .fusion import MODEL_ORDER, fuse, fuse_tracks
from .video_pipeline import lstm_step, tracks_plan, visual_from_static, visual_from_static_tracks


@dataclass
class _Options:
    """run_inference's keyword options and their defaults, stated once (what each means: run_inference's docstring).  Both calls bind
    their keyword arguments to it, so an unknown name is Python's own TypeError naming it, and the pass loop reads one object."""
    path_save_results: str = ""
    name_video: str = "video"
    flag_save_prob: bool = False
    weights_prob_model: object = None
    weights_model: Sequence = (1, 1, 1)
    ce_weights_type: bool = True
    ce_mask: bool = False
    sr: int = 16000
    window: float = 4
    step: float = 0.5
    padding: str = "mean"
    mode: int = MODE_DEFAULT
    flag_heatmaps: bool = False
    model_heatmaps: str = "static"
    wav_sr: Optional[int] = None
    path_save_faces: Optional[str] = None
    jpeg_entropy: str = "host"
    faces_via_jpeg: bool = False
    path_save_video: Optional[str] = None
    video_model: str = "av"
    video_quality: int = 90
    video_panel: bool = False
    video_timing: Optional[Sequence[int]] = None
    video_opendml: bool = False
    video_segment_bytes: int = 1 << 30
    tracks: object = None
    detect_size: object = None
    detect_filter: str = "bilinear"
    flag_save_plot_pred: bool = False
    plot_size: Sequence[int] = (200, 1200)


class _Source:
    """A video as the pass loop reads it: `total` frames of `height` x `width` in passes of `per` frames; `decode(a)` returns the pass
    that starts at frame a, uint8 [<= per, height, width, 3] BGR on the device."""

    def __init__(self, total: int, height: int, width: int, per: int, decode):
        self.total, self.height, self.width, self.per, self.decode = int(total), int(height), int(width), int(per), decode

    def passes(self):
        return (self.decode(a) for a in range(0, self.total, self.per))


def run_inference_file(engine, path, detector=None, detections: Optional[Sequence[np.ndarray]] = None, fps: Optional[float] = None,
                       frames_per_pass: int = 64, stream_frames: Optional[int] = None, audio_windows_per_pass: int = 128, opendml: bool = True,
                       **kw):
    """`run_inference` on a recording: the reference's first line, `VideoPredictor.process` opening a video file
    (data/get_face_images.py:19-24, 44-47), for the one container this project reads without a decoder library -- the Motion-JPEG /
    PCM AVI file that `ffmpeg -i clip.mp4 -c:v mjpeg -q:v 2 -c:a pcm_s16le -ar 44100 -ac 2 clip.avi` writes (avcer_amd/avi.py).
    The same container with uncompressed BGR video (`-c:v rawvideo -pix_fmt bgr24`: the decoder's own frames, no lossy transcode; the
    device unpacks them, dib.unpack_frames) is read as well, and `opendml=True` (the default here; no test pins the refusal through
    this entry point) reads the OpenDML layout ffmpeg changes to past 1 GiB, so a long file simply runs; opendml=False refuses it as
    avi.open_avi does by default.
    open_avi -> AviFile.decode_frames (jpeg.decode_frames or dib.unpack_frames by the file's codec: the frames are decoded on the
    device and never exist on the host) ->
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
    same pass loop (_run) in passes of N frames instead of one pass holding all: at most N decoded frames -- one pass buffer, decode
    and compute are not overlapped -- are alive on the device, whatever the length, and the dict, the CSV files, the face folders, the
    heat maps and the result video are the in-memory call's, bit for bit (the loop's results do not depend on its pass size).  Only the PCM of the whole file stays on the device (30 minutes of
    44.1 kHz stereo: 318 MB), and the audio windows go through the model `audio_windows_per_pass` at a time (streamed calls only).
    With `path_save_video` the file is decoded a second time behind the fusion, which the labels need.  "No face track 00" is
    known at the end of the sweep and raises the same FileNotFoundError there.  Anything but None or an int >= 1 (0, a negative, a
    bool, a float) raises ValueError naming stream_frames before the file is opened.  A set of recordings: run_dataset(stream_frames=N)
    with video_job_from_avi jobs, the same passes with the videos sharing the GPU passes behind them.
    `tracks=` (run_inference) is refused, where it is refused, before the file is opened, and holds for both paths: streamed, a
    named track that never appeared raises its FileNotFoundError at the end of the sweep, as "no face track 00" does.
    `detect_size=` / `detect_filter=` (run_inference) hold for both paths too: a bad value is refused before the file is opened, an
    upscale once the container has named the frame size, before any decode; streamed, every pass is resized on its own (there is no
    state across frames), so the results are the in-memory call's.
    `flag_save_plot_pred=` (run_inference) holds for both paths: what it refuses is refused before the file is opened; streamed, the
    chart is made behind the last pass from the class tables the call keeps anyway, and the file is the in-memory call's.
    Returns run_inference's dict; `real_time_factor` includes demux and decode."""
    from .avi import open_avi

    if stream_frames is not None and (isinstance(stream_frames, (bool, np.bool_)) or not isinstance(stream_frames, (int, np.integer))
                                      or stream_frames < 1):
        raise ValueError(f"stream_frames must be None or an integer >= 1, not {stream_frames!r}")
    if isinstance(audio_windows_per_pass, (bool, np.bool_)) or not isinstance(audio_windows_per_pass, (int, np.integer)) or audio_windows_per_pass < 1:
        raise ValueError(f"audio_windows_per_pass must be an integer >= 1, not {audio_windows_per_pass!r}")
    given_wav = "wav" in kw
    wav = kw.pop("wav", None)
    kw.setdefault("name_video", os.path.splitext(os.path.basename(os.fspath(path)))[0])
    o = _Options(**kw)
    check_tracks(o.tracks, o.flag_heatmaps)
    check_detect_size(o.detect_size, o.detect_filter, detector, detections)
    _check_plot(o)
    start_time = time.time()
    with open_avi(path, opendml=opendml) as avi:
        check_detect_size(o.detect_size, o.detect_filter, detector, detections, (avi.height, avi.width))
        if not given_wav:
            if avi.pcm is None:
                raise ValueError(f"{avi.path}: no audio stream (pass wav= and wav_sr= to give the audio some other way)")
            wav = avi.pcm
            if "wav_sr" not in kw:
                o.wav_sr = avi.audio_rate
        if o.wav_sr is not None:
            resample_plan(o.wav_sr, o.sr)
        check_window(engine, o.window, o.sr)
        if detections is None and detector is None:
            raise ValueError("give a detector or the per-frame detections")
        fps = int(avi.rate / avi.scale) if fps is None else fps
        if o.path_save_video and "video_timing" not in kw:
            o.video_timing = (avi.rate, avi.scale)  # the source's own rate / scale pair, not the rounded fps
        if stream_frames is not None:
            per = int(stream_frames)
            src = _Source(avi.n_frames, avi.height, avi.width, per,
                          lambda a: avi.decode_frames(engine, a, a + per, bgr=True, frames_per_pass=frames_per_pass))
            return _run(engine, src, wav, fps, detector, detections, o, _check(engine, o, detector, detections, (avi.height, avi.width)),
                        start_time, int(audio_windows_per_pass))
        frames = avi.decode_frames(engine, bgr=True, frames_per_pass=frames_per_pass)
        n_frames = avi.n_frames
    out = run_inference(engine, frames, wav, fps, detector=detector, detections=detections, **vars(o))
    duration = n_frames / fps if (fps and fps > 0 and n_frames > 0) else None
    out["real_time_factor"] = (time.time() - start_time) / duration if duration else None
    return out


def run_inference(engine, frames_bgr, wav, fps: float, detector=None, detections: Optional[Sequence[np.ndarray]] = None, **options):
    """The frames as ONE pass of the pass loop (_run) that run_inference_file(stream_frames=N) runs in passes of N frames; frames given
    on the host or as numpy are copied to the device once.  `options`: the keyword options below (_Options states their defaults
    once); an unknown name raises TypeError.
    engine: an `Engine` with the static, dynamic and audio weights loaded.  frames_bgr u8 [T,H,W,3] as cv2 decodes
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
    before any work.  Off by default: nothing changes then.  `video_opendml=True` writes it in the OpenDML layout (avi.AviWriter:
    segments of `video_segment_bytes`, read back with open_avi(opendml=True)), which has no 4 GiB end: the result video of a long
    streamed recording; False (the default) changes nothing.
    `tracks`: which face tracks the visual models and the fusion run on.  None (the default): track directory 00 alone, as the
    reference (get_prob_video.py:79-94 walks `<faces>/00/`; get_face_images.py:73-76 leaves choosing a "target face" among the
    folders to the user) -- today's call, unchanged.  "all": every track directory stage 0 writes, ascending.  A list of distinct
    ints >= 0: those directories (tid - 1, the folder numbers), in that order.  Every selected track is treated as the reference
    would treat it were its folder named `00` -- its own present mask, hold / zero / reset rule and LSTM windows
    (video_pipeline.tracks_plan); the audio table is the video's -- and its tables are, bit for bit, what
    `visual_forward(engine, *track_clip(records, tiles, k, T), fps, mode)` on VideoTiler's tiles and `fusion.fuse` on them give.  Detector, tracker,
    crops and the audio branch run once; ONE static CNN call per pass takes the selected tracks' tiles, ONE LSTM call all their windows, ONE
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
    o = _Options(**options)
    frames = frames_bgr if torch.is_tensor(frames_bgr) else torch.from_numpy(np.ascontiguousarray(frames_bgr))
    checked = _check(engine, o, detector, detections, None if frames.dim() != 4 else tuple(frames.shape[1:3]))
    start_time = time.time()                                                # run.py:200
    if detections is None and detector is None:
        raise ValueError("give a detector or the per-frame detections")
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 [T,H,W,3] (BGR, as cv2 decodes them)")
    if o.wav_sr is not None:
        resample_plan(o.wav_sr, o.sr)
    frames = frames.to(engine.device)  # frames given on the host cross once, for the detector, the crops and the result video alike
    total = int(frames.shape[0])
    return _run(engine, _Source(total, frames.shape[1], frames.shape[2], max(total, 1), lambda a: frames), wav, fps, detector, detections, o,
                checked, start_time)


def _run(engine, src: _Source, wav, fps, detector, detections, o: _Options, checked, start_time: float, audio_windows_per_pass=None):
    """The per-video pipeline, once, for run_inference (ONE pass holding all frames) and run_inference_file(stream_frames=N) (passes of
    N frames, one pass of decoded frames on the device at a time): the results do not depend on the pass size, bit for bit.

    The audio branch is queued first, beside everything else (Engine.side_branch): it depends on nothing of the visual branch and
    runs while the host walks the tracker.  Per pass: src.decode -> detector (or the pass's slice of `detections`) -> the resumable
    tracker (Engine.tracker) -> the crop rectangles, their frame index rebased to the pass -> crop_tiles / roundtrip_face_tiles /
    write_face_crops -> the static CNN on the pass's tiles of track 00, in record order.  Kept between passes: the detections and
    records (host), and per frame of track 00 the static CNN's 7 probabilities and 512 features (2076 bytes); with `flag_heatmaps`,
    per heat-map frame (one in lstm_step(fps)) its 7 raw maps [7,7,7] and its base image [224,224,3] -- as large as the overlays
    that are returned.  Which class a map shows may depend on the LSTM ("dynamic"), which runs behind the sweep, so the overlays of
    both `model_heatmaps` are rendered there, from what was kept.  With `tracks` the static CNN takes the pass's tiles of the
    SELECTED tracks and those 2076 bytes are kept per record of a selected track -- with "all" per record, since which tracks there
    are is known at the end only --, in record order; behind the sweep they are gathered track after track as
    video_pipeline.tracks_plan lays them out.  "No face track" is known once the tracker has seen the last pass, and raises
    there, behind that pass's crops and face files and in front of its static CNN call.  Behind the last pass:
    video_pipeline.visual_from_static / visual_from_static_tracks (plan_clip's windows over all features, one LSTM call), the audio
    branch joined, fuse (fuse_tracks); nothing has been copied to the host yet.  With `path_save_video` the source is read a SECOND
    time, pass by pass, for annotate.write_result_video: the labels need the fused predictions.
    MODE_F16X3: one read of the range-contract counter behind the last launch; a video during which an activation left fp16's range
    is run again in MODE_FP32 (engine.guarded): records, detections and face files are those of the first sweep, the tiles are cut
    again.  `checked`: _check's triple."""
    tracks, plot, hm = checked
    detector = scaled_detector(detector, o.detect_size, o.detect_filter)
    total, per, height, width = src.total, src.per, src.height, src.width
    # the duration the real-time factor divides by, settled before any work is queued: `int(cv2.CAP_PROP_FPS)` is 0 on a
    # broken container, and a finished prediction must not be lost to a ZeroDivisionError in the last statement
    duration = total / fps if (fps and fps > 0 and total > 0) else None
    if detections is not None and len(detections) != total:
        raise ValueError("one detection array per frame")
    dev = engine.device
    wav_t = (wav if torch.is_tensor(wav) else torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32 if o.wav_sr is None else None))).to(dev)
    save = (o.path_save_faces, o.name_video) if o.path_save_faces else (None, None)
    host = {}  # detections, records and face files of every pass: independent of the arithmetic mode, computed once

    def gpu_work(m):
        # a failure on the way (no face track, a detector error) joins the audio branch all the same (Engine.side_branch)
        with engine.side_branch(wav_t) as side:
            with torch.cuda.stream(side.stream):
                win_logits, lo, hi = audio_forward(engine, wav_t, o.sr, fps, o.window, o.step, o.padding, m, wav_sr=o.wav_sr,
                                                   windows_per_pass=audio_windows_per_pass)  # get_prob_audio_8_cl.py:68-138
            side.results(win_logits)
            first = "records" not in host
            if first:
                tracker, passes, files = engine.tracker(0.4, 0.0), [], []  # VideoTiler's tracker settings

            def settle():
                # every frame has been tracked: which tracks there are is known, in front of the last pass's visual models
                tracker.close()
                records = np.concatenate(passes) if passes else np.zeros((0, 6), dtype=np.int64)
                if save[0]:
                    host["face_files"] = files
                if tracks is not None:
                    host["tracks_plan"] = tracks_plan(records, select_tracks(records, tracks), total, fps)
                elif not (records[:, 1] == 0).any():
                    raise FileNotFoundError("no face track 00 (os.listdir(<faces>/00) fails in the reference, get_prob_video.py:79)")
                host["passes"], host["records"] = passes, records

            present = np.zeros(total, dtype=bool)
            every = lstm_step(fps)
            if every <= 0:
                raise ZeroDivisionError("integer division or modulo by zero")  # as plan_clip: `curr_idx_frame % step`
            probs, feats, cams, bases = [], [], [], []
            kept, n_rec = [], 0  # `tracks`: the records (numbered through the video) whose static outputs are kept
            for k, a in enumerate(range(0, total, per)):
                frames = src.decode(a)
                if first:
                    records = track_pass(tracker, frames, a, width, height, detector, detections)  # get_face_images.py:49
                    passes.append(records)
                else:
                    records = host["passes"][k]
                tiles = None
                if len(records):
                    if o.faces_via_jpeg:
                        tiles, paths = roundtrip_face_tiles(engine, frames, records, *(save if first else (None, None)), entropy=o.jpeg_entropy,
                                                            frame_base=a)
                    else:
                        tiles = pass_tiles(engine, frames, records, a)
                        paths = write_face_crops(engine, frames, records, *save, entropy=o.jpeg_entropy, frame_base=a) if first and save[0] else None
                    if first and save[0]:
                        files.extend(paths)
                if first and a + per >= total:
                    settle()
                if len(records):
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
                        if hm is not None:
                            _, p, f, cam = engine.static_forward_cam(tiles00, m)
                            pick = np.flatnonzero(r00[:, 0] % every == 0)
                            if len(pick):
                                cams.append(cam.index_select(0, torch.from_numpy(pick).to(dev)))
                                rects = torch.from_numpy(pass_rects(r00[pick], a).astype(np.int32))
                                if o.faces_via_jpeg:  # cv2.resize of the read-back crop (get_prob_video.py:99-100, data/utils.py:105)
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
            if "records" not in host:  # a video without a frame
                settle()
            probs, feats = (t[0] if len(t) == 1 else torch.cat(t) for t in (probs, feats))
            maps = None
            if tracks is not None:
                # what was kept lies in record order; the plan wants it track after track
                tp = host["tracks_plan"]
                pos = np.searchsorted(np.concatenate(kept), tp.rows)
                if len(pos) != len(probs) or (np.diff(pos) != 1).any():
                    pos = torch.from_numpy(pos).to(dev)
                    probs, feats = probs.index_select(0, pos), feats.index_select(0, pos)
                static_probs, dynamic_logits = visual_from_static_tracks(engine, probs, feats, tp, fps, m)
            else:
                static_probs, dynamic_logits, dl = visual_from_static(engine, probs, feats, present, fps, m, with_windows=True)  # get_prob_video.py:67-204
                if hm is not None:
                    fidx, rows, win = hm.heatmap_plan(present, fps)
                    if len(rows):
                        cls = hm.heatmap_classes(engine, o.model_heatmaps, probs, dl, rows, win)
                        maps = (fidx, engine.cam_render(torch.cat(cams), np.arange(len(rows)), cls, torch.cat(bases), hm.JET_BGR, hm.IMAGE_WEIGHT))
                    else:
                        maps = (fidx, torch.zeros((0, 224, 224, 3), dtype=torch.uint8, device=dev))
        # fusion last, behind both branches
        prob, am = (fuse if tracks is None else fuse_tracks)(engine, static_probs, dynamic_logits, win_logits, lo, hi, o.weights_prob_model,
                                                             o.weights_model, o.ce_weights_type, o.ce_mask)  # run.py:25-189
        return static_probs, dynamic_logits, win_logits, lo, hi, prob, am, maps

    out = _results(engine, engine.guarded(o.mode, gpu_work), host, src.passes, wav, fps, o, plot)
    # "Real-time factor for compound expression prediction" as run.py:304-307 prints it: elapsed / video duration (the
    # device -> host copies above have synchronised the stream, so the clock covers all the work); None where the
    # container reported no frame rate
    out["real_time_factor"] = (time.time() - start_time) / duration if duration else None
    return out


def _check(engine, o: _Options, detector, detections, frame_size=None):
    """What both calls refuse before any work, in this order -> (tracks as check_tracks returns them, _check_plot's pair or None,
    the heat-map module when `flag_heatmaps`, else None)."""
    tracks = check_tracks(o.tracks, o.flag_heatmaps)
    plot = _check_plot(o)
    video_models = [m.lower() for m in MODEL_ORDER]
    if o.video_model not in video_models:
        raise ValueError(f"video_model must be one of {' / '.join(video_models)}, not {o.video_model!r}")
    if o.jpeg_entropy not in ("host", "device"):
        raise ValueError(f'jpeg_entropy must be "host" or "device", not {o.jpeg_entropy!r}')
    check_via_jpeg(o.faces_via_jpeg)
    hm = None
    if o.flag_heatmaps:
        from . import heatmaps as hm

        hm.check_model(o.model_heatmaps)
    check_window(engine, o.window, o.sr)
    check_detect_size(o.detect_size, o.detect_filter, detector, detections, frame_size)
    return tracks, plot, hm


def _check_plot(o: _Options):
    """`flag_save_plot_pred` off (the default): None, and the chart module is not even imported.  On: what chart.check_plot_pred
    refuses is refused here, before any work; returns (rule, (height, width))."""
    if o.flag_save_plot_pred is False:
        return None
    from .chart import check_plot_pred

    return check_plot_pred(o.flag_save_plot_pred, o.path_save_results, o.ce_weights_type, o.ce_mask, o.plot_size)


def _results(engine, res, host, frames, wav, fps, o: _Options, plot=None):
    """Everything behind the guarded device work: the tables to the host, the CSV files, the heat-map files, the result video, the
    prediction chart (`plot`: _check_plot's pair).  `res` is gpu_work's tuple; `frames`: a callable that yields the decoded frames
    once more in passes (annotate.write_result_video)."""
    path_save_results, name_video, wav_sr, video_model, video_timing = o.path_save_results, o.name_video, o.wav_sr, o.video_model, o.video_timing
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
    if o.flag_save_prob:
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
            hm.write_heatmaps(hm.heatmap_dir(path_save_results, name_video, o.model_heatmaps), maps[0], maps[1], engine=engine)
    if o.path_save_video:
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
        out["result_video"] = write_result_video(engine, frames, records, pred, prob_model, o.path_save_video, int(video_timing[0]),
                                                 int(video_timing[1]), pcm=pcm, audio_rate=int(wav_sr) if pcm is not None else 44100,
                                                 quality=o.video_quality, entropy="device", panel=o.video_panel, tracks=labelled,
                                                 **(dict(opendml=True, segment_bytes=o.video_segment_bytes) if o.video_opendml else {}))
    return out
