"""The visual models over a corpus of face folders, in packed passes: the `__main__` of get_prob_video.py (:207-361, its loops over
AFEW, ABAW and C-EXPR-DB) without one chain of launches per folder -- the visual twin of audio_corpus.run_corpus.

    FaceFolder / list_corpus     one folder `<root>/<video>/<track>/NNNNNN.jpg` of stage 0 and what the reference's `df_fps` table says
                                 of it: frame rate and frame count
    corpus_plan                  everything decided before the device is touched: the present mask of every folder (read_face_dir's
                                 rule), `plan_clip` of every folder with its own frame rate, laid out through the set
                                 (video_pipeline.clips_plan), and the static passes the present tiles of consecutive folders are cut into
    run_video_corpus             per pass: the files' bytes (a reader thread, one pass ahead), jpeg.decode_tiles into the ONE pending tile buffer, the
                                 static CNN; then ONE ragged LSTM plan for the set and the per-frame tables by row gathers
                                 (video_pipeline._tables) -- `static__<video>.csv` / `dynamic__<video>.csv` as the reference writes them

`video_pipeline.preprocess_video_and_predict` pays, per folder, its own decode call, static-CNN launches, LSTM call, range-contract
read and host round trips, and a folder of 1 to 5 s of crops fills none of them.  The kernels do not depend on what surrounds a tile
or a window in its batch (tests/test_gpu_visual.py), so tiles and windows of different folders share passes here and every folder
still gets the bits the per-folder call gives it (tests/test_gpu_video_corpus.py).  The passes are cut where dataset.run_dataset
cuts them: behind every `max_frames_per_pass` tiles of the set, and at its end; a pass may end inside a folder.

Heat maps and `tracks=` stay on the per-folder call, there is no `distributed=`, and the AFEW / ABAW label handling stays in
avcer_amd/evaluate.py, which reads the directory this module writes unchanged."""
from __future__ import annotations

import os
import re
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from .engine import MODE_DEFAULT
from .video_pipeline import ClipPlan, _DevicePlan, _read_blob, _tables, clips_plan, lstm_step

_FILE = re.compile(r"(\d{6,})\.jpg")


@dataclass
class FaceFolder:
    """One face folder of a corpus: the crops `<path>/<track>/NNNNNN.jpg` stage 0 wrote of one video (data/get_face_images.py), the
    video's frame rate and its frame count -- the arguments `path_video`, `fps` and `total_frames` of the reference's
    preprocess_video_and_predict.  `name` is the `<video>` of `static__<video>.csv`."""
    name: str
    path: str
    fps: float
    total_frames: int
    track: str = "00"


def frame_name(i: int) -> str:
    """get_prob_video.py:93: the file of frame i."""
    return str(int(i)).zfill(6) + ".jpg"


def _rows(table):
    """The rows of a `df_fps` table: a CSV file with the columns name_video, frame_rate and, where it has it, total_frame (or
    total_frames) -- or the rows themselves, (name_video, frame_rate[, total_frames]) each."""
    if not isinstance(table, (str, os.PathLike)):
        return [tuple(r) for r in table]
    import pandas as pd

    df = pd.read_csv(table)
    for col in ("name_video", "frame_rate"):
        if col not in df.columns:
            raise ValueError(f"{os.fspath(table)}: no column {col!r} (name_video, frame_rate[, total_frame])")
    frames = next((c for c in ("total_frame", "total_frames") if c in df.columns), None)
    if frames is None:
        return list(zip(df.name_video.tolist(), df.frame_rate.tolist()))
    return list(zip(df.name_video.tolist(), df.frame_rate.tolist(), df[frames].tolist()))


def list_corpus(root, table, track: str = "00") -> list:
    """The FaceFolders of a corpus: `root` holds one face folder per video, `table` is what get_prob_video.py's main reads as
    `df_fps` (:216-220, :301-306, :335-339) -- a CSV file with the columns name_video, frame_rate and total_frame, or the rows
    (name_video, frame_rate[, total_frames]) themselves.  `name_video` carries the video file's extension, which is cut off as there
    (`[:-4]`).  One FaceFolder per row, in the table's order; the folder is `<root>/<name>`, or, where that is no directory and
    exactly one `<root>/*/<name>` is (AFEW keeps its folders under one directory per emotion), that one.  A row whose folder does not
    exist is listed all the same: corpus_plan reports it by name.
    Where the table has no frame count, `total_frames` is the number of the folder's last file + 1.  THIS CHOICE IS OURS, NOT THE
    REFERENCE'S, which always has the count of the video file: the frames behind the last crop (each would repeat the last row of
    the tables) are not there then.  It needs the listing, so such a row's missing track directory, or one without a numbered
    file, raises FileNotFoundError here."""
    root = os.fspath(root)
    out = []
    for row in _rows(table):
        if len(row) not in (2, 3):
            raise ValueError(f"a row is (name_video, frame_rate[, total_frames]), got {row!r}")
        name = str(row[0])[:-4]
        path = os.path.join(root, name)
        if not os.path.isdir(path):
            deeper = [os.path.join(root, d, name) for d in sorted(os.listdir(root)) if os.path.isdir(os.path.join(root, d, name))]
            path = deeper[0] if len(deeper) == 1 else path
        if len(row) == 3 and row[2] is not None and not (isinstance(row[2], float) and np.isnan(row[2])):
            total = int(row[2])
        else:
            numbers = [int(m.group(1)) for m in map(_FILE.fullmatch, os.listdir(os.path.join(path, track))) if m and frame_name(m.group(1)) == m.group(0)]
            if not numbers:
                raise FileNotFoundError(f"folder {name}: no NNNNNN.jpg in {os.path.join(path, track)} to take the frame count from")
            total = max(numbers) + 1
        out.append(FaceFolder(name, path, float(row[1]), total, track))
    return out


@dataclass
class CorpusPlan:
    """What corpus_plan decides.  The folders that run are `ok` (indices into the list given, ascending); everything below is laid
    out over them, one behind the other."""
    ok: list                       # the folders that run
    errors: dict                   # folder index -> the exception that leaves it out (skip_failed)
    presents: list                 # per folder of `ok`: bool [total_frames], read_face_dir's mask
    files: list                    # per tile of the set, in (folder, frame) order: the file's path
    host: tuple                    # video_pipeline.clips_plan(presents, the folders' frame rates)
    frame_off: np.ndarray          # int64 [len(ok) + 1]: folder k owns the table rows frame_off[k] : frame_off[k + 1]
    passes: list = field(default_factory=list)  # tiles per static pass: the cuts of the concatenated tile list

    @property
    def n_tiles(self) -> int:
        return len(self.files)

    def clip(self, k: int) -> ClipPlan:
        """Folder ok[k]'s share of the set's plan: plan_clip(presents[k], fps, feat_off[k], win_off[k]), rows counted through the set."""
        s_src, d_src, win, _, w_off = self.host
        a, b = int(self.frame_off[k]), int(self.frame_off[k + 1])
        return ClipPlan(s_src[a:b].tolist(), d_src[a:b].tolist(), win[int(w_off[k]):int(w_off[k + 1])].tolist())


def _check_folder(f: FaceFolder):
    """The present mask of one folder by the rule of read_face_dir (get_prob_video.py:79, 93-94), or the exception that refuses it."""
    if not (isinstance(f.fps, (int, float, np.integer, np.floating)) and f.fps > 0):  # NaN fails the comparison
        raise ValueError(f"folder {f.name}: fps must be a positive number, got {f.fps!r}")
    if isinstance(f.total_frames, (bool, np.bool_)) or not isinstance(f.total_frames, (int, np.integer)) or f.total_frames < 1:
        raise ValueError(f"folder {f.name}: total_frames must be an integer >= 1, got {f.total_frames!r}")
    folder = os.path.join(f.path, f.track)
    try:
        names = set(os.listdir(folder))
    except (FileNotFoundError, NotADirectoryError) as e:
        raise FileNotFoundError(f"folder {f.name}: no track directory {folder}") from e
    present = np.fromiter((frame_name(i) in names for i in range(int(f.total_frames))), dtype=bool, count=int(f.total_frames))
    if not present.any():
        raise FileNotFoundError(f"folder {f.name}: no file below total_frames={int(f.total_frames)} in {folder}")
    return present


def check_pass_size(name: str, value, none_ok: bool = False):
    if none_ok and value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"{name} must be an integer >= 1, not {value!r}")
    return int(value)


def corpus_plan(folders: Sequence[FaceFolder], max_frames_per_pass: int = 2048, skip_failed: bool = False) -> CorpusPlan:
    """Host work only; every track directory is listed once.  Per folder the present mask by read_face_dir's rule and `plan_clip`
    with the folder's own frame rate (step = round(5 * fps / 25)), numbered through the set by video_pipeline.clips_plan; the present
    tiles of consecutive folders, in (folder, frame) order, are cut into static passes of at most `max_frames_per_pass` -- where
    dataset.run_dataset cuts: behind every max_frames_per_pass tiles and at the end, so a pass may end inside a folder.
    ValueError: `max_frames_per_pass` < 1, two folders of one name (both whatever `skip_failed` says), a folder's fps <= 0 or
    total_frames < 1.  FileNotFoundError, naming the folder: no track directory, no file below total_frames.  A frame rate below
    2.5 raises plan_clip's ZeroDivisionError as in the reference.  `skip_failed`: a folder's own failure goes to `errors` and the
    rest are planned as if it had not been given."""
    per = check_pass_size("max_frames_per_pass", max_frames_per_pass)
    folders = list(folders)
    seen = set()
    for f in folders:
        if f.name in seen:
            raise ValueError(f"folder names must be distinct: {f.name!r} is given twice")
        seen.add(f.name)
    ok, errors, presents, files = [], {}, [], []
    for i, f in enumerate(folders):
        try:
            present = _check_folder(f)
            if lstm_step(f.fps) <= 0:  # the folder's own failure; the set's plan below cannot fail then
                raise ZeroDivisionError(f"folder {f.name}: integer division or modulo by zero (fps {f.fps!r}: an LSTM step of 0 frames)")
        except (ValueError, FileNotFoundError, ZeroDivisionError) as e:
            if not skip_failed:
                raise
            errors[i] = e
            continue
        ok.append(i)
        presents.append(present)
        files += [os.path.join(f.path, f.track, frame_name(t)) for t in np.flatnonzero(present)]
    host = clips_plan(presents, [folders[i].fps for i in ok])
    frame_off = np.concatenate([[0], np.cumsum([len(p) for p in presents])]).astype(np.int64)
    n = len(files)
    return CorpusPlan(ok, errors, presents, files, host, frame_off, [min(per, n - a) for a in range(0, n, per)])


class CorpusResults(list):
    """One dict per folder, in the order given: {"name", "static_probs" f32 [total_frames, 7], "dynamic_logits" f32 [total_frames,
    7], "present" bool [total_frames]}, tensors on the device -- or {"name", "error": the exception} for a folder skip_failed left
    out.  `passes`: the sizes of the static and LSTM passes of the last attempt, as DatasetResults.passes."""
    passes = None


def read_files(paths) -> list:
    """The bytes of the files `paths`, in order.  One after the other: a face crop is a few KiB, and handing such reads out file by
    file to a pool of Python threads costs more than it saves (tools/video_corpus_bench.py: 10 600 cached files in 376 ms on 16 pool
    threads, a third of that in a plain loop).  run_video_corpus hides the loop instead: one reader thread fetches the next pass."""
    return [_read_blob(p) for p in paths]


def decode_pass(engine, blobs, out, decode: str = "device", entropy: str = "host", threads: int = 0):
    """The tiles of one pass's files into `out` (the head of the pending tile buffer): jpeg.decode_tiles, or PIL's lines of
    read_face_dir with decode="pil"."""
    import torch

    from . import jpeg

    if decode == "device":
        jpeg.decode_tiles(engine, blobs, threads, entropy=entropy, out=out)
    else:
        out.copy_(torch.from_numpy(np.stack([jpeg._pil_tile(b) for b in blobs])), non_blocking=False)
    return out


def run_video_corpus(engine, folders: Sequence[FaceFolder], mode: int = MODE_DEFAULT, max_frames_per_pass: int = 2048,
                     max_windows_per_pass: Optional[int] = None, decode: str = "device", entropy: str = "host", threads: int = 0,
                     save_path: Optional[str] = None, flag_save_prob: bool = False, skip_failed: bool = False,
                     plan: Optional[CorpusPlan] = None) -> CorpusResults:
    """`preprocess_video_and_predict` for every face folder of a corpus, the folders sharing the GPU passes (module docstring).
    Returns a CorpusResults: per folder `static_probs`, `dynamic_logits` and `present` on the device, with the bits
    preprocess_video_and_predict(decode="device") gives for that folder alone, in MODE_F16X3 and in MODE_FP32, for every pass
    size and both `entropy` modes.  `flag_save_prob` writes `static__<name>.csv` and `dynamic__<name>.csv` under `save_path`
    (io_formats.write_visual_csvs: the per-folder call's files, byte for byte), the directory evaluate.afew_tables / abaw_tables read.

    Passes: the files of a pass are read by one reader thread, a pass ahead of the device, and decoded by ONE jpeg.decode_tiles call
    (`entropy`: "host" or "device", `threads`: the host threads of its entropy pass, 0: jpeg.host_threads, 16 at most; a file the
    device path does not handle goes through PIL there, as always) straight into the pending tile buffer -- ONE buffer of min(max_frames_per_pass, the tiles of the corpus) tiles, the
    shape run_dataset(stream_frames=) keeps; no per-folder tensor is joined, a pass is on the device once.  The static CNN runs
    on the buffer's head, and its tiles are overwritten by the next pass (stream order).  The host reads pass p + 2 and
    entropy-decodes pass p + 1 while the device runs the CNN on pass p.  decode="pil": the tiles come from PIL on the host.
    ONE LSTM call takes the windows of all folders (`max_windows_per_pass`: None, or at most that many per call; the logits are the
    same), the hold / zero / reset rule is each folder's own (plan_clip, get_prob_video.py:157-178).

    Range contract: everything sits inside ONE engine.guarded(mode, ...).  One counter cannot say which folder overflowed, so a
    corpus in which any activation leaves fp16's range is repeated in MODE_FP32 AS A WHOLE (every file is read a second time):
    the price of one counter read per corpus, as in run_dataset and run_corpus.

    Errors: what corpus_plan refuses, a pass size below 1, a `decode` or `entropy` it does not know, and flag_save_prob without
    save_path raise before anything is launched.  `skip_failed`: a refused folder's dict is {"name", "error"}, the others run
    and give the bits they give without it.  A file neither the device path nor PIL can read raises PIL's error when its pass
    comes, as in the per-folder call.  `plan`: what corpus_plan returned for these very arguments."""
    import torch

    from . import io_formats, jpeg

    if decode not in ("device", "pil"):
        raise ValueError(f"decode must be 'device' or 'pil', got {decode!r}")
    jpeg._check_entropy(entropy)
    per_lstm = check_pass_size("max_windows_per_pass", max_windows_per_pass, none_ok=True)
    if flag_save_prob and not save_path:
        raise ValueError("flag_save_prob needs a save_path")
    folders = list(folders)
    plan = corpus_plan(folders, max_frames_per_pass, skip_failed) if plan is None else plan
    out = CorpusResults({"name": f.name} for f in folders)
    for i, e in plan.errors.items():
        out[i]["error"] = e
    passes = {"static": [], "lstm": []}
    out.passes = passes
    if not plan.ok:
        return out
    dev = engine.device
    n_frames = int(plan.frame_off[-1])

    def call(m):
        passes.update(static=[], lstm=[])
        queue = torch.empty((max(plan.passes), 224, 224, 3), dtype=torch.uint8, device=dev)
        probs, feats, at = [], [], 0
        with ThreadPoolExecutor(1) as reader:  # the next pass's files are read while this pass is decoded and queued
            ahead = reader.submit(read_files, plan.files[:plan.passes[0]])
            for k, n in enumerate(plan.passes):
                blobs = ahead.result()
                at += n
                if k + 1 < len(plan.passes):
                    ahead = reader.submit(read_files, plan.files[at:at + plan.passes[k + 1]])
                tiles = decode_pass(engine, blobs, queue[:n], decode, entropy, threads)
                _, p, f = engine.static_forward(tiles, m)
                probs.append(p)
                feats.append(f)
                passes["static"].append(n)
        cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts)
        # the ragged LSTM plan of the whole set, then the per-frame tables by row gathers (video_pipeline._tables)
        stat, dyn, _ = _tables(engine, _DevicePlan(engine, None, None, plan.host), cat(probs), cat(feats), n_frames, m, per_lstm,
                               passes["lstm"])
        return stat, dyn

    # MODE_F16X3: one read of the range-contract counter for the whole corpus (engine.guarded)
    stat, dyn = engine.guarded(mode, call)
    present = torch.from_numpy(np.concatenate(plan.presents)).to(dev)
    if flag_save_prob:
        rows = torch.cat([stat, dyn], dim=1).cpu().numpy()  # one copy back for all files
    for k, i in enumerate(plan.ok):
        a, b = int(plan.frame_off[k]), int(plan.frame_off[k + 1])
        out[i].update(static_probs=stat[a:b], dynamic_logits=dyn[a:b], present=present[a:b])
        if flag_save_prob:
            io_formats.write_visual_csvs(np.ascontiguousarray(rows[a:b, :7]), np.ascontiguousarray(rows[a:b, 7:]), save_path, folders[i].name)
    return out
