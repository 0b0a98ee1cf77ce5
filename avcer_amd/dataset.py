"""A set of videos of unequal length and frame rate, run as packed passes: the batch drivers of the reference
(get_prob_video.py:207-361, get_prob_audio_8_cl.py `__main__`, run.py:192-268 in a folder loop) without one chain of launches per video.

`run.run_inference` pays, per video, its own launches, host-to-device copies and range-contract read, and a 3 s video fills none
of them.  The kernels do not depend on what surrounds a frame or a window in its batch (tests/test_gpu_visual.py, tests/test_gpu_audio.py: one frame / window against its row in a batch),
so frames and windows of different videos share passes here and every video still gets the bits `run_inference` gives it:

  stage 0, per video   detector (or given detections) -> tracker -> the tiles of track 00       (resolutions differ)
  visual, packed       present tiles of consecutive videos -> static CNN in passes of <= max_frames_per_pass frames; a pass may
                       end inside a video.  Tiles are dropped behind their pass; the feature and probability tables stay.
  LSTM, ragged         `plan_clip` per video with its own fps, one index table for the set, gather + LSTM in passes
  audio, side stream   every waveform (resampled per video where `wav_sr` is set) into ONE device buffer, `chunk_spans` per
                       video shifted by the video's base, chunker + model in passes of <= max_windows_per_pass windows
  fusion               ONE `Engine.fuse_videos` launch for the set

`run_dataset(stream_frames=N)` changes the shape of stage 0 alone: a video's frames arrive in passes of at most N (VideoJob.open), each
pass goes through the detector, the resumable tracker and the tile cut (face_tiles.track_pass / pass_tiles, the step run._run takes per
pass of one file) and is dropped before the next one is fetched; its tiles of track 00 join the same static passes, cut at the same
places.  Device memory for frames is then one frame pass, whatever the length of the recording.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import dist as adist
from . import io_formats
from .audio_pipeline import check_window, chunk_spans, replicate_per_frame, resample_out_len, resample_plan
from .engine import MODE_DEFAULT, MODE_F16X3, MODE_FP32
from .face_tiles import check_detect_size, check_via_jpeg, pass_tiles, scaled_detector, track_pass
from .fusion import MODEL_ORDER, covered_frames
from .video_pipeline import _DevicePlan, _tables, clips_plan


@dataclass
class VideoJob:
    """One video of a set.  The metadata (what a container's header gives) is all that planning and sharding read; `load()` is
    called once, when the video's turn comes, and returns (frames_bgr u8 [n_frames, height, width, 3], wav) as `run_inference`
    takes them: wav float32 [n_samples] mono at the call's `sr`, or, with `wav_sr`, the source audio at that rate with
    n_samples frames per channel.  `detections`: per-frame detection arrays instead of the call's detector.
    `open(frames_per_pass)`: what `run_dataset(stream_frames=N)` calls instead of `load`, once, when the video's turn comes ->
    (passes, wav): `passes` an iterable of u8 [k, height, width, 3] BGR batches in frame order (device tensors or host arrays, as
    `load` may return either), every k <= frames_per_pass, the k's summing to n_frames; `wav` as `load` returns it.  The driver drops
    a batch before it asks for the next one and calls `passes.close()`, where there is one, on every exit path."""
    name: str
    n_frames: int
    height: int
    width: int
    fps: float
    n_samples: int
    wav_sr: Optional[int] = None
    load: Optional[Callable] = None
    detections: Optional[Sequence[np.ndarray]] = None
    open: Optional[Callable] = None


class _AviPasses:
    """The frames of an open AviFile in passes of `per`, decoded on the device as they are asked for (video_job_from_avi's `open`).  The
    file is closed behind the last pass, by `close()`, when a decode raises, and when the iterator is dropped."""

    def __init__(self, avi, engine, per: int, frames_per_pass: int):
        self.avi, self.engine, self.per, self.frames_per_pass, self.at = avi, engine, int(per), frames_per_pass, 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.avi is None or self.at >= self.avi.n_frames:
            self.close()
            raise StopIteration
        lo, hi = self.at, min(self.at + self.per, self.avi.n_frames)
        try:
            frames = self.avi.decode_frames(self.engine, lo, hi, bgr=True, frames_per_pass=self.frames_per_pass)
        except BaseException:
            self.close()
            raise
        self.at = hi
        if hi >= self.avi.n_frames:
            self.close()
        return frames

    def close(self):
        avi, self.avi = getattr(self, "avi", None), None
        if avi is not None:
            avi.close()

    def __del__(self):
        self.close()


def video_job_from_avi(path, detections: Optional[Sequence[np.ndarray]] = None, engine=None, frames_per_pass: int = 64,
                       opendml: bool = True) -> VideoJob:
    """The job of one Motion-JPEG or uncompressed-BGR / PCM AVI file (avcer_amd/avi.py: what is read, what is refused; `opendml`:
    open_avi's flag, True by default here -- no test pins the refusal through this entry point -- so a file past 1 GiB simply runs).  The metadata comes from the
    container's headers and its chunk walk alone -- no frame is decoded; fps is int(rate / scale), as run.run_inference_file
    takes it.  `load` opens the file again when the video's turn comes, decodes the frames on the device (AviFile.decode_frames; on
    `engine`, default: the engine alive for the current device, which is the one run_dataset was given) and returns them with the
    source audio, int16 [L, C] at the file's rate.  A file without an audio stream raises ValueError here.
    `open(n)` (run_dataset(stream_frames=n)) opens the file again as well and hands out AviFile.decode_frames(engine, lo, lo + n) pass
    after pass (_AviPasses) with the same audio: no more than n decoded frames of the file are alive, whatever its length and codec."""
    import os

    from .avi import open_avi

    path = os.fspath(path)
    with open_avi(path, opendml=opendml) as avi:
        if avi.pcm is None:
            raise ValueError(f"{path}: no audio stream")
        meta = (avi.n_frames, avi.height, avi.width, int(avi.rate / avi.scale), len(avi.pcm), avi.audio_rate)

    def load():
        from .engine import Engine

        with open_avi(path, opendml=opendml) as avi:
            eng = engine if engine is not None else Engine.live()
            return avi.decode_frames(eng, bgr=True, frames_per_pass=frames_per_pass), avi.pcm

    def open(per):
        from .engine import Engine

        avi = open_avi(path, opendml=opendml)
        try:
            return _AviPasses(avi, engine if engine is not None else Engine.live(), per, frames_per_pass), avi.pcm
        except BaseException:
            avi.close()
            raise

    name = os.path.splitext(os.path.basename(path))[0]
    return VideoJob(name, meta[0], meta[1], meta[2], meta[3], meta[4], wav_sr=meta[5], load=load, detections=detections, open=open)


class DatasetResults(list):
    """The per-video dicts in job order; `real_time_factor` = elapsed time of the call / summed duration of the videos that
    ran (None where no video reported a frame rate), `passes` = the sizes of the packed passes of the last attempt."""
    real_time_factor = None
    passes = None


def ragged_plan(presents, fpss):
    """`plan_clip` over a set of videos with their own frame rates -- video_pipeline.clips_plan with a mask and a frame rate per
    video: (static_src [N], dyn_src [N], windows [n_win,10], n_feat), row numbers counted through the set; -1 = the zero row."""
    s_src, d_src, win, f_off, _ = clips_plan(presents, fpss)
    return s_src, d_src, win, int(f_off[-1])


def _cat(parts):
    """The passes' outputs as one tensor (None when there was no pass); a single pass is not copied."""
    return None if not parts else parts[0] if len(parts) == 1 else torch.cat(parts)


def _n_audio(job: VideoJob, sr: int) -> int:
    if job.wav_sr is None:
        return int(job.n_samples)
    plan = resample_plan(job.wav_sr, sr)
    return resample_out_len(int(job.n_samples), plan.o, plan.n)


NO_TRACK_00 = "no face track 00 (os.listdir(<faces>/00) fails in the reference, get_prob_video.py:79)"


def _track00(engine, job: VideoJob, dets):
    """Tracker + crop rectangles of one video (host code): the records and the rows of track 00 in frame order."""
    if len(dets) != job.n_frames:
        raise ValueError("one detection array per frame")
    records = engine.track_faces(dets, job.width, job.height, 0.4, 0.0)  # VideoTiler's tracker settings
    if not (len(records) and (records[:, 1] == 0).any()):
        raise FileNotFoundError(NO_TRACK_00)
    rows = np.where(records[:, 1] == 0)[0]
    return records, rows[np.argsort(records[rows, 0], kind="stable")]


def check_stream_frames(value):
    """run_dataset's `stream_frames`: None or an int >= 1 (a bool is refused, as run.run_inference_file refuses it), else ValueError."""
    if value is not None and (isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 1):
        raise ValueError(f"stream_frames must be None or an integer >= 1, not {value!r}")
    return None if value is None else int(value)


def checked_passes(job: VideoJob, batches, per: int):
    """The batches `job.open(per)` hands out as (first frame, frames as a tensor) pairs, each held to what the job's metadata says:
    [k, height, width, 3] with k <= per, and n_frames in all -- the ValueError of the shape check on load() otherwise.  An empty
    batch is passed over.  No batch is referenced here once the consumer asks for the next one."""
    at, want = 0, (int(job.n_frames), int(job.height), int(job.width), 3)
    for batch in batches:
        frames = batch if torch.is_tensor(batch) else torch.from_numpy(np.ascontiguousarray(batch))
        del batch
        shape = tuple(frames.shape)
        if len(shape) != 4 or shape[1:] != want[1:] or shape[0] > per or at + shape[0] > want[0]:
            raise ValueError(f"video {job.name}: open({per}) gave frames {shape} at frame {at}, the job says passes of at most {per} "
                             f"frames and {want} in all")
        if shape[0]:
            yield at, frames
            at += shape[0]
        del frames
    if at != want[0]:
        raise ValueError(f"video {job.name}: open({per}) gave {at} frames, the job says {want}")


def pass_rows(frame_of_row: np.ndarray, a: int, b: int):
    """Rows lo..hi-1 of a table whose frame column `frame_of_row` ascends are those of the frame pass [a, b): how known records (given
    detections, or the first sweep's when the set is repeated in fp32) are dealt out to the passes."""
    lo, hi = np.searchsorted(frame_of_row, (a, b), side="left")
    return int(lo), int(hi)


def _local_tables(engine, jobs, idx, plans, detector, m, sr, window, padding, max_frames, max_windows, passes, via_jpeg=False, stream=None):
    """Stages 0 to audio for the videos `idx` (ascending): (stat|dyn rows [sum frames, 14], window logits [sum windows, c]).
    `stream`: run_dataset's stream_frames."""
    dev = engine.device
    win_a = int(window * sr)
    w_off = np.concatenate([[0], np.cumsum([len(plans[i]["starts"]) for i in idx])]).astype(np.int64)
    s_off = np.concatenate([[0], np.cumsum([plans[i]["n_audio"] for i in idx])]).astype(np.int64)
    if s_off[-1] > 2 ** 31 - 1:
        raise ValueError(f"run_dataset: {int(s_off[-1])} audio samples in one set (the chunker takes 2^31 - 1): split the set")
    starts = np.concatenate([plans[i]["starts"] + s_off[k] for k, i in enumerate(idx)] or [np.zeros(0, np.int64)])
    ends = np.concatenate([plans[i]["ends"] + s_off[k] for k, i in enumerate(idx)] or [np.zeros(0, np.int64)])
    # a failure in stage 0 or in load() unwinds through the join: no launch of this call outlives it (Engine.side_branch)
    with engine.side_branch() as branch:
        side = branch.stream
        with torch.cuda.stream(side):
            wav_all = torch.empty(int(s_off[-1]), dtype=torch.float32, device=dev)
        a_done, a_out = 0, []
        pend, n_pend, feats, probs, presents = [], 0, [], [], []

        def audio_passes(ready, flush):
            nonlocal a_done
            with torch.cuda.stream(side):
                while ready - a_done >= (1 if flush else max_windows):
                    b = min(a_done + max_windows, ready)
                    chunks = engine.audio_chunks(wav_all, starts[a_done:b], ends[a_done:b], win_a, padding)
                    a_out.append(engine.audio_forward(chunks, normalize=True, mode=m))
                    passes["audio"].append(b - a_done)
                    a_done = b

        def queue_audio(k, i, job, wav):
            # audio first, on its own stream: it depends on nothing of the visual branch
            wav_t = wav if torch.is_tensor(wav) else torch.from_numpy(
                np.ascontiguousarray(wav, dtype=np.float32) if job.wav_sr is None else np.ascontiguousarray(wav))
            with torch.cuda.stream(side):
                wav_d = wav_t.to(dev)
                wav_d = wav_d.reshape(-1) if job.wav_sr is None else engine.resample(wav_d, job.wav_sr, sr)
                if int(wav_d.numel()) != plans[i]["n_audio"]:
                    raise ValueError(f"video {job.name}: load() gave {int(wav_d.numel())} samples at {sr} Hz, the job's "
                                     f"n_samples / wav_sr give {plans[i]['n_audio']}")
                wav_all[int(s_off[k]):int(s_off[k + 1])] = wav_d
            audio_passes(int(w_off[k + 1]), False)

        def static_pass(tiles):
            _, p, f = engine.static_forward(tiles, m)
            probs.append(p)
            feats.append(f)
            passes["static"].append(int(p.shape[0]))

        def static_passes(flush):
            nonlocal pend, n_pend
            while n_pend >= (1 if flush else max_frames):
                tiles = pend[0] if len(pend) == 1 else torch.cat(pend)
                static_pass(tiles[:max_frames])
                pend = [tiles[max_frames:]] if tiles.shape[0] > max_frames else []
                n_pend = int(pend[0].shape[0]) if pend else 0

        # streamed, the pending tiles lie in ONE buffer of a static pass (or of every tile the videos can give, where that is less)
        # instead of a list of per-video tensors: a video arrives as many small passes, and joining them as the list is joined would
        # hold its tiles twice.  The passes are cut at the same places: behind every max_frames tiles of the set, and at its end.
        if stream is not None:
            room = sum(len(plans[i]["rows00"]) if "rows00" in plans[i] else int(jobs[i].n_frames) for i in idx)
            queue = torch.empty((min(max_frames, room), 224, 224, 3), dtype=torch.uint8, device=dev)

        def queue_tiles(tiles):
            nonlocal n_pend
            at, n = 0, int(tiles.shape[0])
            while at < n:
                take = min(n - at, max_frames - n_pend)
                queue[n_pend:n_pend + take] = tiles[at:at + take]
                n_pend, at = n_pend + take, at + take
                if n_pend == max_frames:
                    static_pass(queue)
                    n_pend = 0

        def stream_video(job, plan, batches):
            """Stage 0 of one video in frame passes -> its present mask; the records are the plan's, or are gathered here."""
            known = "records" in plan
            if known:
                records, rows = plan["records"], plan["rows00"]
                frame00 = records[rows, 0]
            else:
                tracker, parts = engine.tracker(0.4, 0.0), []  # VideoTiler's tracker settings
            present = np.zeros(job.n_frames, dtype=bool)
            try:
                for a, frames in checked_passes(job, batches, stream):
                    if known:
                        lo, hi = pass_rows(frame00, a, a + int(frames.shape[0]))
                        r00 = records[rows[lo:hi]]
                    else:
                        parts.append(track_pass(tracker, frames, a, job.width, job.height, detector))
                        r00 = parts[-1][parts[-1][:, 1] == 0]
                    if len(r00):
                        present[r00[:, 0]] = True
                        queue_tiles(pass_tiles(engine, frames, r00, a, via_jpeg))
                    del frames  # the pass is dropped before the next one is fetched
            finally:
                if not known:
                    tracker.close()
            if not known:  # every frame has been tracked: whether there is a track 00 is known now
                records = np.concatenate(parts) if parts else np.zeros((0, 6), dtype=np.int64)
                if not (records[:, 1] == 0).any():
                    raise FileNotFoundError(NO_TRACK_00)
                rows = np.where(records[:, 1] == 0)[0]
                plan["records"], plan["rows00"] = records, rows[np.argsort(records[rows, 0], kind="stable")]
            return present

        for k, i in enumerate(idx):
            job = jobs[i]
            passes["at"] = i  # the job a failure in this loop belongs to
            if stream is not None:
                batches, wav = job.open(stream)
                try:
                    queue_audio(k, i, job, wav)
                    presents.append(stream_video(job, plans[i], batches))
                finally:  # an open recording is closed on every path out of its video
                    getattr(batches, "close", lambda: None)()
                continue
            frames, wav = job.load()
            frames = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
            if tuple(frames.shape) != (job.n_frames, job.height, job.width, 3):
                raise ValueError(f"video {job.name}: load() gave frames {tuple(frames.shape)}, the job says "
                                 f"{(job.n_frames, job.height, job.width, 3)}")
            queue_audio(k, i, job, wav)
            # stage 0: the tiles of track 00, in frame order
            if "records" not in plans[i]:
                dets = job.detections if job.detections is not None else detector.batch(frames, rgb=False)
                plans[i]["records"], plans[i]["rows00"] = _track00(engine, job, dets)
            records, rows = plans[i]["records"], plans[i]["rows00"]
            present = np.zeros(job.n_frames, dtype=bool)
            present[records[rows, 0]] = True
            presents.append(present)
            rects = torch.from_numpy(records[rows][:, [0, 2, 3, 4, 5]].astype(np.int32))
            if via_jpeg:  # the tiles as stage 1 of the reference reads them back from stage 0's files (run_inference's faces_via_jpeg)
                from . import jpeg

                pend.append(jpeg.roundtrip_tiles(engine, frames, rects, bgr=True, quality=95, subsampling=2))
            else:
                pend.append(engine.crop_tiles(frames, rects, bgr=True))
            n_pend += len(rows)
            static_passes(False)
        passes["at"] = None
        if stream is None:
            static_passes(True)
        elif n_pend:
            static_pass(queue[:n_pend])
        audio_passes(int(w_off[-1]), True)
        # ragged LSTM plan over the whole set, then the per-frame tables by row gathers (video_pipeline._tables)
        plan = _DevicePlan(engine, None, None, clips_plan(presents, [jobs[i].fps for i in idx]))
        stat, dyn, _ = _tables(engine, plan, _cat(probs), _cat(feats), sum(len(p) for p in presents), m, max_frames, passes["lstm"])
        branch.results(*a_out)
    win_logits = _cat(a_out) if a_out else torch.zeros(0, engine.audio_classes, device=dev)
    return torch.cat([stat, dyn], dim=1), win_logits


def run_dataset(engine, jobs: Sequence[VideoJob], detector=None, *, mode: int = MODE_DEFAULT, sr: int = 16000, window: float = 4,
                step: float = 0.5, padding: str = "mean", weights_prob_model=None, weights_model=(1, 1, 1),
                ce_weights_type: bool = True, ce_mask: bool = False, max_frames_per_pass: int = 2048,
                max_windows_per_pass: int = 128, path_save_results: str = "", flag_save_prob: bool = False,
                skip_failed: bool = False, distributed: bool = False, faces_via_jpeg: bool = False, detect_size=None,
                detect_filter: str = "bilinear", flag_save_plot_pred: bool = False, plot_size: Sequence[int] = (200, 1200),
                stream_frames: Optional[int] = None) -> DatasetResults:
    """`run_inference` for every job of a set, with the videos sharing the GPU passes (module docstring).  Returns a
    `DatasetResults`: a list with one dict per job, in job order, holding `name` and the keys of `run_inference` -- av / vs / vd
    / a, compound_prob, static_probs, dynamic_logits, audio_rows, audio_frames, records -- with the bits `run_inference` gives for
    that video alone, in MODE_F16X3 and in MODE_FP32.  The real-time factor is one figure for the call, on the list's
    `real_time_factor` attribute: elapsed time over the summed duration of the videos that ran.  `flag_save_prob` writes each
    video's CSV files as `run_inference` does (io_formats).  Heat maps and `tracks=` are not part of this path, streamed or not.

    `stream_frames`: None (the default) is the call as it always was: `job.load()` hands over the whole clip, and device memory
    grows with the longest video.  An int N >= 1: every job's frames arrive through `job.open(N)` in passes of at most N frames;
    a pass goes through the detector (or takes its share of the job's `detections`), the resumable tracker and the tile cut, its
    tiles of track 00 join the pending tiles, and it is dropped before the next pass is fetched -- one frame pass of one video is
    on the device at a time, whatever the lengths.  The static passes are cut where the in-memory call cuts them (they may end
    inside a video, inside a frame pass, or span videos), so `passes` and every table are the in-memory call's, bit for bit, for
    every N; the pending tiles lie in one buffer of min(`max_frames_per_pass`, the tiles the set can give) tiles.  Audio, LSTM,
    fusion, files, `skip_failed`, the fp32 repeat (every job is opened a second time; the records are the first sweep's) and
    `distributed` are untouched.  With a detector "no face track 00" is known behind the video's last pass and raises the same
    FileNotFoundError there.  Anything but None or an int >= 1 (a bool, a float, a string), and a job without `open`, raise
    ValueError before any work; a batch of the wrong shape or size, and a total other than `n_frames`, raise the ValueError of
    load()'s shape check when they are met.

    `faces_via_jpeg` (for the call, as the other options): `run_inference`'s option of that name for every job -- the tiles of track
    00 are what reading stage 0's JPEG files back gives; the results are those of `run_inference(..., faces_via_jpeg=True)` for each
    video alone.  Off by default; anything but a bool raises ValueError before any work.

    `detect_size` / `detect_filter` (for the call): `run_inference`'s options of those names -- `detector` runs on a smaller copy of
    every job's frames (face_tiles.ScaledDetector) and is priced at its network's work on that copy.  None (the default): nothing
    changes.  A bad value, and a target larger than some job's frames, raise ValueError before any work.

    `flag_save_plot_pred` / `plot_size` (for the call): `run_inference`'s option -- the prediction timeline chart of every video that
    ran, as `<path_save_results>/<name>/pedicted_CEs_Rule N.jpg`, each file byte for byte that of the video's own `run_inference`
    call (which writes it to its own `path_save_results`); the dict's `plot_pred` is the path.  ONE chart.write_charts call draws
    the whole set from the fused class table where it lies on the device.  Off by default: nothing changes then.  What
    run_inference refuses (no `path_save_results`, neither rule, an empty plot rectangle) raises ValueError before any work.

    Passes: at most `max_frames_per_pass` tiles per static-CNN call (and LSTM windows per LSTM call), at most
    `max_windows_per_pass` audio windows per audio call; device memory for tiles is one pass plus one video, beside that video's
    decoded frames -- with `stream_frames` one pass plus one frame pass's tiles, beside that frame pass.

    Range contract: the packed computation sits inside ONE `engine.guarded(mode, ...)`.  One counter cannot say which video
    overflowed, so a set in which any activation leaves fp16's range is repeated in MODE_FP32 AS A WHOLE (every job is loaded
    a second time); that is the price of one counter read per set instead of one per video.

    Failures: whatever the metadata and given `detections` decide is decided before anything is launched -- a rate pair the
    resampler does not cover (ValueError), no face track 00 (FileNotFoundError), a tracker error (ValueError naming the frame),
    audio windows that cover no frame (IndexError); the message names the video.  With a `detector` the track is only known once
    the video has been decoded, so such a job fails when its turn comes (the side stream is joined on every exit path).
    `skip_failed`: a failed job's dict is {"name", "error": the exception} and the others proceed; failures found up front cost
    nothing, one found mid-way repeats the call without that job.

    `distributed` (torch.distributed initialised): rank r runs stages 0 to audio for the videos `dist.shard_videos` gives it
    (balanced by `dist.video_cost`); an int32 status per video, the stat|dyn rows and the window logits are exchanged with
    `dist.all_gather_ragged`; fusion runs replicated over the whole set in job order, and every rank returns every video."""
    start_time = time.time()
    jobs = list(jobs)
    stream_frames = check_stream_frames(stream_frames)
    for job in jobs if stream_frames is not None else ():
        if getattr(job, "open", None) is None:
            raise ValueError(f"video {job.name}: stream_frames={stream_frames} needs a job with `open` (VideoJob.open, video_job_from_avi)")
    if padding not in ("mean", "constant", "repeat"):
        raise ValueError(f"padding={padding!r}")
    if max_frames_per_pass < 1 or max_windows_per_pass < 1:
        raise ValueError("run_dataset: pass sizes >= 1")
    check_via_jpeg(faces_via_jpeg)
    plot = None
    if flag_save_plot_pred is not False:
        from . import chart

        plot = chart.check_plot_pred(flag_save_plot_pred, path_save_results, ce_weights_type, ce_mask, plot_size)
    check_window(engine, window, sr)
    check_detect_size(detect_size, detect_filter, detector, [] if detector is None else None)
    for job in jobs if detect_size is not None else ():
        if job.detections is None:
            check_detect_size(detect_size, detect_filter, detector, None, (job.height, job.width))
    detector = scaled_detector(detector, detect_size, detect_filter)
    errors = {}

    def fail(i, e):
        if not skip_failed:
            raise type(e)(f"video {jobs[i].name}: {e}") from e
        errors[i] = e

    # ---- planning: metadata and given detections only; nothing is launched
    plans = []
    for i, job in enumerate(jobs):
        plan = {}
        plans.append(plan)
        try:
            if job.detections is None and detector is None:
                raise ValueError("give a detector or the per-frame detections")
            plan["n_audio"] = _n_audio(job, sr)
            starts, ends, lo, hi = chunk_spans(plan["n_audio"], sr, job.fps, window, step)
            plan.update(starts=starts, ends=ends, lo=lo, hi=hi)
            covered_frames(lo, hi, int(job.n_frames))
            if job.detections is not None:
                plan["records"], plan["rows00"] = _track00(engine, job, job.detections)
        except (ValueError, FileNotFoundError, IndexError) as e:
            fail(i, e)

    world = torch.distributed.get_world_size() if distributed and torch.distributed.is_initialized() else 1
    rank = torch.distributed.get_rank() if world > 1 else 0
    # a detector is priced at its own network's work (R50 50.7 GFLOP per 640 x 360 frame, MobileNet-0.25 1.116, S3FD 144.27); one without the
    # attribute counts as R50, as before; a face_tiles.ScaledDetector at its inner network's work on the smaller copy of that job's frames
    def det_cost(j):
        if detector is None or j.detections is not None:
            return False
        if hasattr(detector, "gflop_at"):
            return float(detector.gflop_at(j.height, j.width))
        return True if getattr(detector, "kind", 1) == 1 else float(detector.gflop_per_frame)
    shards = adist.shard_videos([adist.video_cost(j, window, det_cost(j), sr, step) for j in jobs], world)
    passes = {}

    def local(m):
        """This rank's tables; a job that fails on the way is dropped (skip_failed) and the rest starts over."""
        while True:
            mine = [i for i in shards[rank] if i not in errors]
            passes.update(static=[], lstm=[], audio=[], at=None)
            if not mine:
                return (torch.zeros(0, 14, device=engine.device), torch.zeros(0, max(engine.audio_classes, 1), device=engine.device))
            try:
                return _local_tables(engine, jobs, mine, plans, detector, m, sr, window, padding, int(max_frames_per_pass),
                                     int(max_windows_per_pass), passes, bool(faces_via_jpeg), stream_frames)
            except (ValueError, FileNotFoundError) as e:
                bad = passes["at"]
                if bad is None:
                    raise
                if world > 1:
                    errors[bad] = e  # every rank learns of it from the status exchange and raises (or skips) there
                else:
                    fail(bad, e)

    def fuse_all(rows, win_logits, ok):
        n_f = [int(jobs[i].n_frames) for i in ok]
        n_w = [len(plans[i]["lo"]) for i in ok]
        prob, am, _, _ = engine.fuse_videos(rows[:, :7], rows[:, 7:], win_logits, np.concatenate([plans[i]["lo"] for i in ok]),
                                            np.concatenate([plans[i]["hi"] for i in ok]), n_f, n_w, weights_prob_model,
                                            weights_model, ce_weights_type, ce_mask, names=[jobs[i].name for i in ok], with_mean=False)
        return rows, win_logits, prob, am

    if world == 1:
        def call(m):
            rows, win_logits = local(m)
            ok = [i for i in range(len(jobs)) if i not in errors]
            return (fuse_all(rows, win_logits, ok) if ok else None), ok
        # MODE_F16X3: one read of the range-contract counter for the whole set (engine.guarded)
        tables, ok = engine.guarded(mode, call)
    else:
        tables, ok = _distributed(engine, jobs, plans, shards, rank, mode, local, fuse_all, errors, skip_failed)

    out = DatasetResults({"name": j.name} for j in jobs)
    for i, e in errors.items():
        out[i]["error"] = e
    if tables is not None:
        if plot is not None:  # one batched call for the whole set, from the class table [4, sum T] on the device
            plot_files = [chart.plot_paths(os.path.join(path_save_results, jobs[i].name), plot[0])[0] for i in ok]
            base = chart.chart_plan(int(jobs[ok[0]].n_frames), width=plot[1][1], height=plot[1][0])
            chart.write_charts(engine, tables[3], plot_files, T=[int(jobs[i].n_frames) for i in ok], plan=base)
            for i, path in zip(ok, plot_files):
                out[i]["plot_pred"] = path
        rows, win_logits, prob, am = (t.cpu().numpy() for t in tables)
        f_at = w_at = 0
        for i in ok:
            job, plan = jobs[i], plans[i]
            f_to, w_to = f_at + int(job.n_frames), w_at + len(plan["lo"])
            a_rows, a_frames = replicate_per_frame(win_logits[w_at:w_to], plan["lo"], plan["hi"])
            stat = np.ascontiguousarray(rows[f_at:f_to, :7])
            dyn = np.ascontiguousarray(rows[f_at:f_to, 7:])
            if flag_save_prob:
                io_formats.write_visual_csvs(stat, dyn, path_save_results, job.name)
                io_formats.write_audio_csv(a_rows, a_frames, path_save_results, "audio", job.name)
            out[i].update({name.lower(): np.ascontiguousarray(am[k, f_at:f_to]) for k, name in enumerate(MODEL_ORDER)})
            out[i].update(compound_prob=np.ascontiguousarray(prob[:, f_at:f_to]), static_probs=stat, dynamic_logits=dyn,
                          audio_rows=a_rows, audio_frames=a_frames, records=plan.get("records"))
            f_at, w_at = f_to, w_to
    duration = sum(jobs[i].n_frames / jobs[i].fps for i in ok if jobs[i].fps and jobs[i].fps > 0)
    out.real_time_factor = (time.time() - start_time) / duration if duration else None
    passes.pop("at", None)
    out.passes = passes
    return out


def exchange_tables(rows, win_logits, shards, n_frames, n_windows, force: bool = False):
    """The two payload collectives of the distributed path: this rank's stat|dyn rows [k,14] and window logits [w,c] (its videos
    in ascending order) -> the whole set's tables in job order.  n_frames / n_windows: rows per video, 0 for a video that
    contributes none (a failed one)."""
    return (adist.merge_shards(adist.all_gather_ragged(rows, force), shards, n_frames),
            adist.merge_shards(adist.all_gather_ragged(win_logits, force), shards, n_windows))


def _distributed(engine, jobs, plans, shards, rank, mode, local, fuse_all, errors, skip_failed):
    """Per-rank stages, one status exchange, two payload exchanges, replicated fusion.  The status word of a video: bit 0 = the
    video failed on its rank, bit 1 = its rank saw the range contract broken.  Every rank takes the same decisions from the
    gathered words: a set with a failure raises everywhere (unless skip_failed), a set with an overflow is repeated in
    MODE_FP32 on every rank, so the collectives stay matched."""
    if mode == MODE_F16X3:
        engine.x3_overflow_clear()
    rows, win_logits = local(mode)
    over = mode == MODE_F16X3 and engine.x3_overflow_count(reset=True) > 0
    mine = shards[rank]
    word = torch.tensor([[(1 if i in errors else 0) | (2 if over else 0)] for i in mine], dtype=torch.int32,
                        device=engine.device).reshape(len(mine), 1)
    status = adist.merge_shards(adist.all_gather_ragged(word), shards, [1] * len(jobs)).reshape(-1).cpu().numpy()
    for i in np.nonzero(status & 1)[0]:
        if not skip_failed:
            raise errors.get(int(i), RuntimeError(f"video {jobs[int(i)].name} failed on another rank"))
        errors.setdefault(int(i), RuntimeError(f"video {jobs[int(i)].name} failed on another rank"))
    if (status & 2).any():
        engine.x3_fallbacks += 1
        rows, win_logits = local(MODE_FP32)
    ok = [i for i in range(len(jobs)) if i not in errors]
    if not ok:
        return None, ok
    n_f = [int(j.n_frames) if i not in errors else 0 for i, j in enumerate(jobs)]
    n_w = [len(plans[i]["lo"]) if i not in errors else 0 for i in range(len(jobs))]
    rows, win_logits = exchange_tables(rows, win_logits, shards, n_f, n_w)
    return fuse_all(rows, win_logits, ok), ok
