"""The audio model over a labelled corpus: windows, features, votes -- the inference half of the reference's src/audio/**.

    cexpr_windows / abaw_windows / afew_windows   `parse_features` / `prepare_data` of src/audio/data/c_expr_dataset.py:111-179,
                                                  abaw_fe_dataset.py:103-202 and afew_fe_dataset.py:113-156: label files, mouth-open
                                                  tables and durations become the window tables the datasets hold as `meta`
    meld_windows                                  `prepare_data` of meld_dataset.py:93-180, the second training corpus of
                                                  train_c_audio.py, on one utterance's VAD segments
    window_samples                               the cut of their `__getitem__` (c_expr_dataset.py:283-285, abaw_fe_dataset.py:312-318)
    run_corpus                                    test_c_audio.iterate_model / NetTrainer.extract_features (net_trainer.py:469-535):
                                                  the model over every window of every file
    majority_voting                               utils/common_utils.py:74-108: one prediction per file
    extract_features / write_pickle               run_extract_features.py:223-271: the per-file dict and its pickle

The window rules are host code (numpy and Python; pandas is not needed): they are a few integers per window.  Everything per sample
and per window runs in libavcer_hip.so: every waveform of the corpus lies in ONE device buffer (as dataset.run_dataset keeps them),
the windows of all files are cut, padded with zeros and normalised by Engine.audio_chunks and run by Engine.audio_forward in passes
of `windows_per_pass` -- a pass may end inside a file -- and ONE avcer_window_votes launch (csrc/votes.hip) turns the corpus's window
logits into probabilities, classes and per-file votes.  The kernels do not depend on what surrounds a window in its batch
(tests/test_gpu_audio.py), so every window's row holds the bits of a one-window Engine.audio_forward call.

Where the reference is odd, so is this:
  * the end of a window is the frame BEHIND its last label ("skip last frame") unless the sequence ends there;
  * a window shorter than `min_w_len` (C-EXPR) or than `max_w_len` (ABAW) is replaced by the last `max_w_len` seconds of its sequence,
    which is often a window that exists already: duplicates are dropped;
  * the window label is `max(set(w), key=w.count)`: the most frequent value, and among equally frequent ones the first in CPython's
    set order -- stated here with that very expression, so it is that order by construction;
  * the C-EXPR planner leaves the order of its duplicate-free set to the set; here the windows come sorted by (start_f, end_f);
  * a window may be cut past the end of its file (fps rounding); the slice ends with the file, and zeros follow.

`votes_numpy` states the vote kernel in plain numpy for the tests; it is a statement of the arithmetic, not a CPU path."""
from __future__ import annotations

import json
import math
import os
import pickle
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .audio_pipeline import check_window

AFEW_TO_ABAW = {"Neutral": 0, "Angry": 1, "Disgust": 2, "Fear": 3, "Happy": 4, "Sad": 5, "Surprise": 6}  # afew_fe_dataset.py:82-90
NEW_FPS = 5              # abaw_fe_dataset.py:75: mouth_open is reported at 5 values per second
VOTES_MAX_CLASSES = 8    # include/avcer_hip.h AVCER_VOTES_MAX_CLASSES
VOTES_TARGET_MIN = -2    # include/avcer_hip.h AVCER_VOTES_TARGET_MIN
MELD_TO_ABAW = {"neutral": 0, "anger": 1, "disgust": 2, "fear": 3, "joy": 4, "sadness": 5, "surprise": 6}   # meld_dataset.py:81-89
KINDS = ("cexpr", "abaw", "afew")
# the kinds of a Windows table and the window_samples rule each is cut by: MELD's __getitem__ (meld_dataset.py:202-204) cuts
# round(sr * start_t) : round(sr * end_t), which is the C-EXPR rule (c_expr_dataset.py:283-285)
TABLE_CUTS = {"cexpr": "cexpr", "abaw": "abaw", "afew": "afew", "meld": "cexpr"}


def round_math(val: float) -> int:
    """utils/common_utils.py:111-130: halves away from zero (Python's round sends them to the even neighbour)."""
    frac, whole = math.modf(val)
    if frac >= 0.5:
        return int(whole + 1)
    if frac <= -0.5:
        return int(whole - 1)
    return int(math.ceil(whole))


@dataclass
class Windows:
    """The window table of one file: what the reference's datasets keep per window in `meta`.  `start_f` / `end_f` are frame
    numbers (1-based `lab_id`) for C-EXPR and ABAW and sample numbers for AFEW.  `mouth_open` [n, groups] (ABAW): the majority
    of the mouth-open flag per group of 5 values at 5 per second; `fps` (ABAW): the video's frame rate as given; `vad_info` (AFEW):
    the file's entry of the VAD pickle."""
    kind: str
    start_t: np.ndarray   # float64 [n] seconds
    end_t: np.ndarray     # float64 [n]
    start_f: np.ndarray   # int64 [n]
    end_f: np.ndarray     # int64 [n]
    expr: np.ndarray      # int64 [n]
    fps: Optional[float] = None
    mouth_open: Optional[np.ndarray] = None
    vad_info: object = None

    def __len__(self) -> int:
        return int(self.start_f.shape[0])


def _table(kind, rows, **extra) -> Windows:
    """rows: (start_t, end_t, start_f, end_f, expr) tuples."""
    col = lambda j, dt: np.asarray([r[j] for r in rows], dtype=dt).reshape(-1)
    return Windows(kind, col(0, np.float64), col(1, np.float64), col(2, np.int64), col(3, np.int64), col(4, np.int64), **extra)


def _check_plan(fps, expr, mouth_open, shift, min_w_len, max_w_len):
    if not (isinstance(fps, (int, float, np.integer, np.floating)) and math.isfinite(fps) and fps > 0):
        raise ValueError(f"the frame rate must be a positive number, got {fps!r}")
    for name, v in (("shift", shift), ("min_w_len", min_w_len), ("max_w_len", max_w_len)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1 (seconds), got {v!r}")
    if round_math(fps) < 1:
        raise ValueError(f"the frame rate {fps!r} rounds to 0 frames per second")
    expr, mouth_open = np.asarray(expr), np.asarray(mouth_open)
    if expr.ndim != 1 or mouth_open.ndim != 1 or expr.shape[0] != mouth_open.shape[0]:
        raise ValueError(f"expr and mouth_open are one value per frame each, got {expr.shape} and {mouth_open.shape}")
    return expr, mouth_open


def _vote(window: list):
    """The window label of the reference, c_expr_dataset.py:159 / abaw_fe_dataset.py:172, as it is written there: ties go to the
    first value in CPython's set order."""
    return max(set(window), key=window.count)


def _seg_windows(frames, exprs, shift, short, max_w_len):
    """The `seg` loop both frame planners share (c_expr_dataset.py:140-157, abaw_fe_dataset.py:130-149): (start index, stop index,
    start frame, end frame) per window; a window shorter than `short` becomes the last `max_w_len` labels of the sequence."""
    n = len(frames)
    for seg in range(0, n, shift):
        stop = min(seg + max_w_len, n)
        lo, end = seg, frames[stop - 1] if stop > n - 1 else frames[stop]   # skip last frame
        if stop - seg < short:
            lo, stop, end = max(0, n - max_w_len), n, frames[-1]
        yield lo, stop, frames[lo], end


def cexpr_windows(expr, mouth_open, fps, shift: int = 2, min_w_len: int = 2, max_w_len: int = 4, threshold: float = 0.5,
                  lab_id=None) -> Windows:
    """CExprDataset.parse_features (c_expr_dataset.py:111-179).  expr, mouth_open: one value per frame (frame k is `lab_id` k + 1;
    `lab_id`: other ascending frame numbers); fps: the video's frame rate; shift, min_w_len, max_w_len: seconds; threshold: seconds
    of closed mouth from which a run of frames is dropped.  Kept: `round_math` on the frame rate; the run-length filter (a frame
    stays when its run of equal mouth values is shorter than threshold * round_math(fps) or its mouth is open), which counts runs
    BEFORE the rows with expr == -1 leave; the split where `lab_id` jumps by more than 1; the skip of sequences shorter than
    min_w_len; the "skip last frame" end; the short tail, against min_w_len; the window label; the removal of duplicates.
    The reference leaves the order of its duplicate-free set to the set: here the windows are SORTED by (start_f, end_f).
    ValueError: a frame rate that is not positive, expr and mouth_open of different lengths, shift / min_w_len / max_w_len < 1."""
    expr, mouth_open = _check_plan(fps, expr, mouth_open, shift, min_w_len, max_w_len)
    rm = round_math(fps)
    shift_f, max_f, min_f = shift * rm, max_w_len * rm, min_w_len * rm
    n = int(expr.shape[0])
    ids = np.arange(1, n + 1, dtype=np.int64) if lab_id is None else np.asarray(lab_id, dtype=np.int64).reshape(-1)
    if ids.shape[0] != n:
        raise ValueError(f"lab_id is one frame number per label, got {ids.shape[0]} for {n}")
    closed = 1 - mouth_open.astype(np.float64)
    # runs of equal values (`diff().ne(0).cumsum()`; NaN differs from everything, itself included) and their sizes
    new_run = np.ones(n, dtype=bool)
    new_run[1:] = ~(closed[1:] == closed[:-1])
    run = np.cumsum(new_run) - 1
    size = np.bincount(run, minlength=1)[run] if n else np.zeros(0, np.int64)
    keep = (expr != -1) & ((size < threshold * rm) | (mouth_open == 1))
    ids, labels = ids[keep], expr[keep]
    rows = set()
    bounds = np.flatnonzero(np.diff(ids) > 1) + 1 if ids.size else np.zeros(0, np.int64)
    for a, b in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [ids.size]])):
        frames, exprs = [int(v) for v in ids[a:b]], [v.item() for v in labels[a:b]]
        if len(frames) < min_f:
            continue
        for lo, stop, start, end in _seg_windows(frames, exprs, shift_f, min_f, max_f):
            rows.add((start / rm, end / rm, start, end, _vote(exprs[lo:stop])))
    return _table("cexpr", sorted(rows, key=lambda r: (r[2], r[3], r[4])))


def abaw_windows(expr, mouth_open, fps, shift: int = 2, min_w_len: int = 2, max_w_len: int = 4, num_classes: int = 8,
                 new_fps: int = NEW_FPS) -> Windows:
    """AbawFEDataset.parse_features (abaw_fe_dataset.py:103-202): every frame takes part (no mouth filter, no split), a window
    shorter than MAX_w_len becomes the last max_w_len seconds; `mouth_open` (as int) is edge-padded to round_math(fps) * max_w_len
    values, sampled at `downsampled_frames` and reduced per group of `new_fps` by majority; windows whose label is above
    num_classes - 1 are dropped; duplicates leave; the result is sorted by start_t (distinct windows start at distinct frames).
    ValueError as cexpr_windows."""
    expr, mouth_open = _check_plan(fps, expr, mouth_open, shift, min_w_len, max_w_len)
    if isinstance(new_fps, bool) or not isinstance(new_fps, (int, np.integer)) or new_fps < 1:
        raise ValueError(f"new_fps must be an integer >= 1, got {new_fps!r}")
    rm = round_math(fps)
    shift_f, max_f = shift * rm, max_w_len * rm
    n = int(expr.shape[0])
    frames = list(range(1, n + 1))
    mouth = mouth_open.astype(int)
    exprs = [v.item() for v in expr]
    down = [round_math(v) for v in np.arange(0, rm * max_w_len - 1, rm / new_fps, dtype=float)]
    rows = {}
    for lo, stop, start, end in _seg_windows(frames, exprs, shift_f, max_f, max_f):
        label = _vote(exprs[lo:stop])
        if label > num_classes - 1:
            continue
        m = np.pad(mouth[lo:stop], (0, max(0, max_f - (stop - lo))), "edge")[down]
        groups = np.split(m, np.arange(new_fps, len(m), new_fps))
        m = np.asarray([_vote([int(v) for v in g]) for g in groups], dtype=np.int64)
        rows[(start / rm, end / rm, start, end, label, m.tobytes())] = m
    keys = sorted(rows, key=lambda r: (r[0], r[3]))
    width = len(np.arange(new_fps, len(down), new_fps)) + 1
    mouth_rows = np.stack([rows[k] for k in keys]) if keys else np.zeros((0, width), np.int64)
    return _table("abaw", keys, fps=float(fps), mouth_open=mouth_rows)


def afew_label(label) -> int:
    """afew_fe_dataset.py:73-92: the AFEW folder name as the ABAW class number; an int passes through."""
    if isinstance(label, (int, np.integer)) and not isinstance(label, bool):
        return int(label)
    if label not in AFEW_TO_ABAW:
        raise ValueError(f"AFEW label {label!r}: one of {sorted(AFEW_TO_ABAW)}")
    return AFEW_TO_ABAW[label]


def afew_windows(duration: int, label, sr: int = 16000, shift: float = 2, min_w_len: float = 2, max_w_len: float = 4,
                 num_classes: int = 8, vad_info=None) -> Windows:
    """The window loop of AfewFEDataset.prepare_data (afew_fe_dataset.py:113-156) for one file of `duration` samples at `sr` in the
    folder `label`: windows in SAMPLES, every `shift` seconds, `max_w_len` seconds long and ending at the last sample at the latest;
    one shorter than min_w_len becomes the last max_w_len seconds; duplicates leave; sorted by start_t.  The label is the folder's
    ABAW class (afew_label); a file whose class is above num_classes - 1 has no windows.  `vad_info`: the file's entry of the VAD
    pickle, carried along.  ValueError: a negative duration, sr or shift that round to less than one sample."""
    if isinstance(duration, bool) or not isinstance(duration, (int, np.integer)) or duration < 0:
        raise ValueError(f"duration is a number of samples >= 0, got {duration!r}")
    shift_s, max_s, min_s = round(shift * sr), round(max_w_len * sr), round(min_w_len * sr)
    if sr <= 0 or shift_s < 1 or max_s < 1:
        raise ValueError(f"sr={sr!r}, shift={shift!r}, max_w_len={max_w_len!r}: the shift and the window must be at least one sample")
    expr = afew_label(label)
    rows = set()
    for seg in range(0, int(duration), shift_s) if expr <= num_classes - 1 else ():
        start, end = seg, min(duration - 1, seg + max_s)
        if end - start < min_s:
            start, end = max(0, duration - 1 - max_s), duration - 1
        rows.add((start / sr, end / sr, int(start), int(end), expr))
    return _table("afew", sorted(rows, key=lambda r: (r[0], r[3])), vad_info=vad_info)


def meld_label(label) -> int:
    """meld_dataset.py:72-91: the MELD emotion name as the ABAW class number; an int passes through."""
    if isinstance(label, (int, np.integer)) and not isinstance(label, bool):
        return int(label)
    if label not in MELD_TO_ABAW:
        raise ValueError(f"MELD label {label!r}: one of {sorted(MELD_TO_ABAW)}")
    return MELD_TO_ABAW[label]


def meld_windows(segments, emotion, sr: int = 16000, shift: float = 2, min_w_len: float = 2, max_w_len: float = 4,
                 num_classes: int = 8) -> Windows:
    """The window loop of MeldDataset.prepare_data (meld_dataset.py:115-170) for one utterance: `segments` are its entries of the
    VAD pickle, {"start": sample, "end": sample} each, `emotion` its label (meld_label).  Per segment of at least min_w_len
    seconds: windows in SAMPLES every `shift` seconds from the segment's start, max_w_len seconds long and ending with the segment
    at the latest; one shorter than min_w_len becomes the segment's last max_w_len seconds (from its start at the earliest), which
    is often a window that exists already: duplicates leave.  An utterance whose class is above num_classes - 1 has no windows.
    The reference de-duplicates through a set and leaves the order to it: here the windows are SORTED by (start_f, end_f).
    ValueError: an unknown emotion, sr, shift or a window length that round to less than one sample, a segment that is no pair of
    integers with start <= end."""
    shift_s, max_s, min_s = round(shift * sr), round(max_w_len * sr), round(min_w_len * sr)
    if sr <= 0 or shift_s < 1 or max_s < 1:
        raise ValueError(f"sr={sr!r}, shift={shift!r}, max_w_len={max_w_len!r}: the shift and the window must be at least one sample")
    expr = meld_label(emotion)
    rows = set()
    for s in segments:
        a, b = s["start"], s["end"]
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (a, b)) or a < 0 or b < a:
            raise ValueError(f"a VAD segment is {{'start': sample, 'end': sample}} with 0 <= start <= end, got {s!r}")
        a, b = int(a), int(b)
        if b - a < min_s or expr > num_classes - 1:
            continue
        for seg in range(0, b - a, shift_s):
            start, end = a + seg, min(b, a + seg + max_s)
            if end - start < min_s:
                start, end = max(a, b - max_s), b
            rows.add((start / sr, end / sr, start, end, expr))
    return _table("meld", sorted(rows, key=lambda r: (r[2], r[3])), vad_info=list(segments))


def window_samples(start_t: float, end_t: float, sr: int, max_w_len: int = 4, kind: str = "cexpr"):
    """The sample range `__getitem__` cuts: (round(sr * start_t), round(sr * end_t)) with Python's round (halves to even), and for
    the ABAW dataset min(round(sr * end_t), sr * (end_t + max_w_len)) as its end (abaw_fe_dataset.py:312-318).  The range is what
    the slice is asked for: it ends with the file where the file is shorter.  A MELD table is cut by the "cexpr" rule (TABLE_CUTS)."""
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r}: one of {KINDS}")
    a, b = round(sr * start_t), round(sr * end_t)
    if kind == "abaw":
        b = int(min(b, sr * (end_t + max_w_len)))
    return int(a), int(b)


# ------------------------------------------------------------------------------------------------ thin readers
def read_labels(path: str) -> np.ndarray:
    """An expression label file (one header line, then one class number per frame; `pd.read_csv(sep=".", header=0)` in
    c_expr_dataset.py:223) -> int64 [frames]."""
    with open(path) as f:
        lines = [ln.strip() for ln in f.read().splitlines()[1:]]
    return np.asarray([int(ln) for ln in lines if ln], dtype=np.int64)


def read_mouth_open(path: str, n_frames: int) -> np.ndarray:
    """A mouth-open CSV (header, then feat_id, frame, surface_area_mouth, mouth_open) joined to frames 1 .. n_frames as
    c_expr_dataset.py:231-243 joins it: float64 [n_frames], 0.0 for a frame the file does not list.  A frame listed twice raises
    ValueError (the reference's merge would double the label row)."""
    out = np.zeros(int(n_frames), dtype=np.float64)
    seen = set()
    with open(path) as f:
        for ln in f.read().splitlines()[1:]:
            if not ln.strip():
                continue
            cells = ln.split(",")
            frame = int(float(cells[1]))
            if frame in seen:
                raise ValueError(f"{path}: frame {frame} is listed twice")
            seen.add(frame)
            if 1 <= frame <= n_frames and cells[3].strip() != "":
                out[frame - 1] = float(cells[3])
    return out


def read_vad(path: str) -> dict:
    """The VAD pickle of afew_fe_dataset.py:117-119: {wav file name: speech timestamps}."""
    with open(path, "rb") as f:
        return pickle.load(f)


def read_meld_labels(path: str, vad: dict) -> list:
    """A MELD label file (`*_sent_emo.csv`: a header naming Dialogue_ID, Utterance_ID and Emotion among its columns) ->
    [(wav file name, emotion)] in the file's order, "dia{Dialogue_ID}_utt{Utterance_ID}.wav" as meld_dataset.py:128 names it, with
    the reference's two filters (:129-133): the broken dia125_utt3 and every name the VAD pickle `vad` (read_vad) does not list."""
    import csv

    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            fn = "dia{0}_utt{1}.wav".format(int(row["Dialogue_ID"]), int(row["Utterance_ID"]))
            if "dia125_utt3" in fn or fn not in vad:
                continue
            out.append((fn, row["Emotion"]))
    return out


def avi_fps_frames(path: str):
    """(frame rate, frame count) of an AVI file from its headers, what find_corresponding_video_info asks cv2 for."""
    from .avi import open_avi

    with open_avi(path) as avi:
        return avi.rate / avi.scale, int(avi.n_frames)


# ------------------------------------------------------------------------------------------------ the vote, stated in numpy
def votes_numpy(logits, targets, file_off):
    """What avcer_window_votes computes (include/avcer_hip.h), in numpy: (probs f32 [n, c], pred i32 [n], file_pred i32 [F],
    file_target i32 [F], file_onehot i32 [F, c]).  Float32 softmax in the kernel's order -- exp(x - max), the sum from class 0 up,
    the quotient; numpy's exp and the device's may differ in the last place --, the first maximum of the logits as the class, per
    file the most frequent class and target, the smallest among equals; -1 and a zero row for a file without windows."""
    x = np.asarray(logits, dtype=np.float32)
    t = np.asarray(targets, dtype=np.int64).reshape(-1)
    off = np.asarray(file_off, dtype=np.int64).reshape(-1)
    n, c = x.shape
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True), dtype=np.float32) if n else x.copy()
        den = e[:, 0].copy()
        for k in range(1, c):
            den = den + e[:, k]
        probs = (e / den[:, None]).astype(np.float32)
    pred = (np.argmax(x, axis=1) if n else np.zeros(0)).astype(np.int32)
    nf = off.shape[0] - 1
    file_pred, file_target = np.full(nf, -1, np.int32), np.full(nf, -1, np.int32)
    onehot = np.zeros((nf, c), np.int32)
    for f in range(nf):
        p, tt = pred[off[f]:off[f + 1]], t[off[f]:off[f + 1]]
        tt = tt[(tt >= VOTES_TARGET_MIN) & (tt < c)]
        if p.size:
            file_pred[f] = np.argmax(np.bincount(p, minlength=c))
            onehot[f, file_pred[f]] = 1
        if tt.size:
            file_target[f] = np.argmax(np.bincount(tt - VOTES_TARGET_MIN)) + VOTES_TARGET_MIN
    return probs, pred, file_pred, file_target, onehot


def _check_targets(targets, c: int) -> np.ndarray:
    t = np.asarray(targets).reshape(-1)
    if t.size and (not np.issubdtype(t.dtype, np.integer) or t.min() < VOTES_TARGET_MIN or t.max() >= c):
        raise ValueError(f"targets are integers in [{VOTES_TARGET_MIN}, {c}) (-2: no labels, -1: unlabelled), got "
                         f"{t.dtype} in [{t.min()}, {t.max()}]")
    return t.astype(np.int32)


def majority_voting(engine, logits, targets, file_off, names: Optional[Sequence[str]] = None):
    """common_utils.majority_voting (utils/common_utils.py:74-108) on the device: window logits [n, c] (a device tensor stays
    where it is), targets [n] (host integers in [-2, c)), file_off [F + 1] (host) -> (targets, preds, filenames) as the reference
    returns them: per file its most frequent target, the one-hot row (int64 [c]) of its most frequent window class, its name.
    The reference groups by file name and `groupby` sorts its keys: with `names` the files come back in SORTED-NAME order whatever
    order they were given in; without, in the order given and numbered.  A file without windows is in no group and is left out.
    One launch (Engine.window_votes) and one copy back."""
    off = np.asarray(file_off, dtype=np.int64).reshape(-1)
    if names is not None and len(names) != off.shape[0] - 1:
        raise ValueError(f"{len(names)} names for {off.shape[0] - 1} files")
    if names is not None and len(set(names)) != len(names):
        raise ValueError("file names must be distinct (the reference groups by them)")
    c = int(logits.shape[1])
    _, _, _, file_target, onehot = engine.window_votes(logits, _check_targets(targets, c), off)
    file_target, onehot = file_target.cpu().numpy(), onehot.cpu().numpy()
    order = [f for f in (range(len(off) - 1) if names is None else np.argsort(np.asarray(names, dtype=object), kind="stable"))
             if off[f + 1] > off[f]]
    return ([int(file_target[f]) for f in order], [onehot[f].astype(np.int64) for f in order],
            [f if names is None else names[f] for f in order])


# ------------------------------------------------------------------------------------------------ the corpus pass
@dataclass
class CorpusResult:
    """What run_corpus returns; tensors are on the device, one row per window, the files' windows one behind the other in the
    order the files were given (file f owns rows file_off[f] : file_off[f + 1])."""
    names: list
    file_off: np.ndarray          # int64 [F + 1]
    starts: np.ndarray            # int64 [n]: first sample of each window in its own file
    ends: np.ndarray              # int64 [n]: the sample behind its last one (clipped to the file)
    targets: np.ndarray           # int32 [n]: the windows' labels
    logits: object                # f32 [n, C]
    probs: object                 # f32 [n, C]: softmax
    pred: object                  # i32 [n]
    file_pred: object             # i32 [F]; -1: no windows
    file_target: object           # i32 [F]
    file_onehot: object           # i32 [F, C]
    features: object = None       # f32 [n, 1024 (ExprModelV2 / V3) or 256 (ExprModelV1)]
    passes: tuple = ()            # windows per pass of the last attempt


def _file_parts(entry):
    if len(entry) == 2:
        return entry[0], entry[1], None
    if len(entry) == 3:
        return entry
    raise ValueError("a file is (name, wav) or (name, wav, wav_sr)")


def plan_corpus(engine, files, windows, sr: int = 16000, max_w_len: int = 4, windows_per_pass: int = 128):
    """Everything run_corpus decides before it touches the device: (names, lengths at `sr`, file_off, starts, ends, targets); the
    window ranges are clipped to their files.  ValueError: a window of more tokens than the loaded model accepts
    (audio_pipeline.check_window), a pass size below 1, files and window tables that do not pair up, a window longer than
    max_w_len seconds, more than 2^31 - 1 samples in the corpus."""
    from .audio_pipeline import resample_out_len, resample_plan

    if isinstance(windows_per_pass, bool) or not isinstance(windows_per_pass, (int, np.integer)) or windows_per_pass < 1:
        raise ValueError(f"windows_per_pass must be an integer >= 1, not {windows_per_pass!r}")
    if isinstance(max_w_len, bool) or not isinstance(max_w_len, (int, np.integer)) or max_w_len < 1:
        raise ValueError(f"max_w_len must be an integer >= 1 (seconds), got {max_w_len!r}")
    check_window(engine, max_w_len, sr)
    files = [_file_parts(f) for f in files]
    if not files:
        raise ValueError("run_corpus: no files")
    if len(files) != len(windows):
        raise ValueError(f"{len(files)} files and {len(windows)} window tables")
    names = [f[0] for f in files]
    if len(set(names)) != len(names):
        raise ValueError("file names must be distinct")
    lengths = []
    for name, wav, wav_sr in files:
        if wav_sr is None:
            if getattr(wav, "ndim", 1) != 1:
                raise ValueError(f"file {name}: a mono waveform [L] at {sr} Hz, or give its rate as (name, wav, wav_sr)")
            lengths.append(int(len(wav)))
        else:
            plan = resample_plan(int(wav_sr), int(sr))
            shape = tuple(wav.shape)
            frames = shape[0] if len(shape) == 1 or str(wav.dtype).endswith("int16") else shape[1]
            lengths.append(resample_out_len(int(frames), plan.o, plan.n))
    s_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if s_off[-1] > 2 ** 31 - 1:
        raise ValueError(f"run_corpus: {int(s_off[-1])} audio samples in one call (the chunker takes 2^31 - 1): split the corpus")
    starts, ends, targets = [], [], []
    for (name, _, _), length, tab in zip(files, lengths, windows):
        if tab.kind not in TABLE_CUTS:
            raise ValueError(f"file {name}: window kind {tab.kind!r}")
        for i in range(len(tab)):
            a, b = window_samples(float(tab.start_t[i]), float(tab.end_t[i]), sr, max_w_len, TABLE_CUTS[tab.kind])
            a, b = min(max(a, 0), length), min(max(b, 0), length)   # a slice ends with the file
            b = max(a, b)
            if b - a > max_w_len * sr:
                raise ValueError(f"file {name}: window {i} ({tab.start_t[i]} s .. {tab.end_t[i]} s) is {b - a} samples, more than "
                                 f"max_w_len={max_w_len} s at {sr} Hz")
            starts.append(a)
            ends.append(b)
        targets.append(tab.expr)
    file_off = np.concatenate([[0], np.cumsum([len(t) for t in windows])]).astype(np.int64)
    tg = np.concatenate(targets).astype(np.int64) if targets else np.zeros(0, np.int64)
    classes = int(getattr(engine, "audio_classes", 0)) or VOTES_MAX_CLASSES
    return names, s_off, file_off, np.asarray(starts, np.int64), np.asarray(ends, np.int64), _check_targets(tg, classes)


def run_corpus(engine, files, windows, sr: int = 16000, max_w_len: int = 4, mode: Optional[int] = None, windows_per_pass: int = 128,
               features: bool = False, plan=None, transform=None) -> CorpusResult:
    """The audio model over every window of a corpus.  files: (name, wav) with wav mono float32 [L] at `sr`, or (name, wav,
    wav_sr) with the source audio at `wav_sr` as Engine.resample takes it (int16 [L] / [L, C] or float32 [L] / [C, L]), brought to
    mono at `sr` on the device; windows: one `Windows` table per file (cexpr_windows / abaw_windows / afew_windows).
    All waveforms go into ONE device buffer; the window ranges (window_samples, clipped to their file) are shifted by their file's
    base; Engine.audio_chunks(padding="constant") and Engine.audio_forward(normalize=True) run in passes of at most
    `windows_per_pass` windows -- a pass may end inside a file --; ONE avcer_window_votes launch makes the probabilities, classes and
    file votes.  Everything sits inside one `engine.guarded(mode, ...)`: a corpus in which any activation leaves fp16's range is
    repeated in MODE_FP32 as a whole.  `features`: also the pooled head activations per window.
    Every window's row holds the bits a one-window Engine.audio_forward call on that window gives (tests/test_gpu_audio_corpus.py).
    What plan_corpus refuses raises ValueError before anything is launched.  `plan`: what plan_corpus returned for these very
    arguments, for a caller that runs one corpus under several models (validate.validate_checkpoints) and plans it once.
    `transform`: an augment.AugmentSpec -- the training windows of train_c_audio.py:112-119 -- puts ONE Engine.wave_augment call
    between the chunker and the forward of every pass; the records of all windows are drawn once, in front of the first pass, from
    (the spec's seed, the window's row in the corpus), so a window's bits do not depend on `windows_per_pass`.  None: nothing of it
    is imported, constructed or launched."""
    import torch

    from .engine import MODE_DEFAULT

    if transform is not None:
        from . import augment

        if not isinstance(transform, augment.AugmentSpec):
            raise ValueError(f"run_corpus: transform is an augment.AugmentSpec or None, got {type(transform).__name__}")
    mode = MODE_DEFAULT if mode is None else mode
    names, s_off, file_off, starts, ends, targets = plan if plan is not None else plan_corpus(engine, files, windows, sr, max_w_len,
                                                                                                 windows_per_pass)
    aug_plan = None if transform is None else augment.draw_plan(transform, int(starts.shape[0]))
    files = [_file_parts(f) for f in files]
    win = int(max_w_len * sr)
    n = int(starts.shape[0])
    g_starts = starts + np.repeat(s_off[:-1], np.diff(file_off))
    g_ends = ends + np.repeat(s_off[:-1], np.diff(file_off))
    passes = []

    def call(m):
        passes.clear()
        dev = engine.device
        wav_all = torch.empty(int(s_off[-1]), dtype=torch.float32, device=dev)
        for k, (name, wav, wav_sr) in enumerate(files):
            t = wav if torch.is_tensor(wav) else torch.from_numpy(
                np.ascontiguousarray(wav, dtype=np.float32) if wav_sr is None else np.ascontiguousarray(wav))
            t = t.to(dev)
            t = t.reshape(-1).to(torch.float32) if wav_sr is None else engine.resample(t, int(wav_sr), int(sr))
            if int(t.numel()) != int(s_off[k + 1] - s_off[k]):
                raise ValueError(f"file {name}: {int(t.numel())} samples at {sr} Hz, planned for {int(s_off[k + 1] - s_off[k])}")
            wav_all[int(s_off[k]):int(s_off[k + 1])] = t
        lg, ft = [], []
        for a in range(0, n, int(windows_per_pass)):
            b = min(a + int(windows_per_pass), n)
            chunks = engine.audio_chunks(wav_all, g_starts[a:b], g_ends[a:b], win, "constant")
            if aug_plan is not None:
                augment.augment(engine, chunks, aug_plan.rows(a, b))
            out = engine.audio_forward(chunks, normalize=True, mode=m, return_features=features)
            lg.append(out[0] if features else out)
            if features:
                ft.append(out[1])
            passes.append(b - a)
        c = int(engine.audio_classes)
        logits = torch.cat(lg) if len(lg) > 1 else lg[0] if lg else torch.zeros(0, c, device=dev)
        feats = None
        if features:
            feats = torch.cat(ft) if len(ft) > 1 else ft[0] if ft else torch.zeros(0, 256 if engine.audio_head_kind == 1 else 1024,
                                                                                    device=dev)
        return logits, feats, engine.window_votes(logits, targets, file_off)

    logits, feats, (probs, pred, file_pred, file_target, onehot) = engine.guarded(mode, call)
    return CorpusResult(names, file_off, starts, ends, targets, logits, probs, pred, file_pred, file_target, onehot, feats, tuple(passes))


# ------------------------------------------------------------------------------------------------ per-file regrouping
def extract_features(engine, files, windows, sr: int = 16000, max_w_len: int = 4, mode: Optional[int] = None,
                     windows_per_pass: int = 128, transform=None) -> dict:
    """run_extract_features.py:223-260: run_corpus with features, regrouped per file.  {file name: {"targets": [np.int64],
    "predicts": [float32 [C] softmax rows], "features": [float32 [1024 or 256] rows], "frame_start" / "frame_end": [int],
    "timestep_start" / "timestep_end": [float]}}, one list entry per window in the table's order, and with them, as the
    datasets' sample_info has them: "fps": [float] and "mouth_open": [int64 [groups]] for ABAW tables, "vad_info": [str, the entry
    as JSON] for AFEW tables.  A file without windows never reaches the reference's loop: it has no entry.  `transform`: as
    run_corpus takes it."""
    res = run_corpus(engine, files, windows, sr, max_w_len, mode, windows_per_pass, features=True, transform=transform)
    probs, feats = res.probs.cpu().numpy(), res.features.cpu().numpy()
    out = {}
    for f, (name, tab) in enumerate(zip(res.names, windows)):
        a, b = int(res.file_off[f]), int(res.file_off[f + 1])
        if b == a:
            continue
        d = {"targets": [np.int64(v) for v in tab.expr], "predicts": [probs[i] for i in range(a, b)],
             "features": [feats[i] for i in range(a, b)]}
        if tab.kind == "abaw":
            d["fps"] = [float(tab.fps)] * (b - a)
        d["timestep_start"] = [float(v) for v in tab.start_t]
        d["timestep_end"] = [float(v) for v in tab.end_t]
        d["frame_start"] = [int(v) for v in tab.start_f]
        d["frame_end"] = [int(v) for v in tab.end_f]
        if tab.kind == "abaw":
            d["mouth_open"] = [np.asarray(r) for r in tab.mouth_open]
        if tab.kind == "afew":
            d["vad_info"] = [json.dumps(tab.vad_info)] * (b - a)
        out[name] = d
    return out


def write_pickle(path: str, d: dict) -> str:
    """run_extract_features.py:262-271: the dict as a pickle of the highest protocol."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(d, f, protocol=pickle.HIGHEST_PROTOCOL)
    return path
