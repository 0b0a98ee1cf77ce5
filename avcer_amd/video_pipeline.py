"""Batched counterpart of get_prob_video.preprocess_video_and_predict (get_prob_video.py:67-204).

The reference walks frames one by one; its rules only decide WHICH feature rows form each LSTM window and WHICH
result row each frame reports.  `plan_clip` restates those rules as index arithmetic on the host (no tensor data),
the GPU then runs the static CNN once over all present frames, gathers the windows, runs the LSTM once, and the
per-frame tables are assembled by row gathers.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np
import torch

from .engine import Engine, MODE_DEFAULT

DICT_EMO_VIDEO = ("Neutral", "Happiness", "Sadness", "Surprise", "Fear", "Disgust", "Anger")  # get_prob_video.py:56-64


def lstm_step(fps: float) -> int:
    """get_prob_video.py:77 (Python's round: banker's rounding)."""
    return round((5 * fps) / 25)


@dataclass
class ClipPlan:
    static_src: list = field(default_factory=list)  # per frame: row of the feature/prob table, -1 = zeros
    dyn_src: list = field(default_factory=list)     # per frame: row of the LSTM output table, -1 = zeros
    windows: list = field(default_factory=list)     # per LSTM evaluation: 10 feature-table rows


def plan_clip(present, fps: float, feat_base: int = 0, win_base: int = 0) -> ClipPlan:
    """Hold / zero / reset rules of get_prob_video.py:91-178 for one clip.  `present[i]` = a face crop exists."""
    step = lstm_step(fps)
    if step <= 0:
        raise ZeroDivisionError("integer division or modulo by zero")  # `curr_idx_frame % step`, get_prob_video.py:114
    plan = ClipPlan()
    window: list[int] = []
    last = None
    nfeat = 0
    for i, p in enumerate(present):
        if p:
            s = feat_base + nfeat
            nfeat += 1
            if i % step == 0:
                window = [s] * 10 if not window else window[1:] + [s]   # :117-120
                plan.windows.append(list(window))
                last = win_base + len(plan.windows) - 1
                d = last
            else:
                d = last if last is not None else -1                      # :157-162
            plan.static_src.append(s)
            plan.dyn_src.append(d)
        else:
            window = []                                                   # :169
            if last is not None:                                          # :170-173
                plan.static_src.append(plan.static_src[-1])
                plan.dyn_src.append(plan.dyn_src[-1])
            else:                                                         # :175-178
                plan.static_src.append(-1)
                plan.dyn_src.append(-1)
    return plan


def clips_plan(present, fps):
    """`plan_clip` over the rows of present bool [n,T] -- or over n masks of their own lengths, the videos of a set --, row numbers
    counted through the set: (static_src int64 [sum T], dyn_src int64 [sum T], windows int32 [n_win,10], feat_off int64 [n+1], win_off
    int64 [n+1]); -1 = the zero row, as in ClipPlan.  Clip c owns the feature rows feat_off[c]..feat_off[c+1] and the LSTM windows
    win_off[c]..win_off[c+1].  `fps`: one frame rate for all clips, or one per clip."""
    present = [np.asarray(row, dtype=bool).reshape(-1) for row in present]
    fpss = [fps] * len(present) if np.ndim(fps) == 0 else list(fps)
    if len(fpss) != len(present):
        raise ValueError(f"clips_plan: {len(fpss)} frame rates for {len(present)} clips")
    s_src, d_src, win, f_off, w_off = [], [], [], [0], [0]
    for row, one_fps in zip(present, fpss):
        p = plan_clip(row, one_fps, f_off[-1], w_off[-1])
        f_off.append(f_off[-1] + int(row.sum()))
        w_off.append(w_off[-1] + len(p.windows))
        s_src += p.static_src
        d_src += p.dyn_src
        win += p.windows
    return (np.asarray(s_src, dtype=np.int64), np.asarray(d_src, dtype=np.int64), np.asarray(win, dtype=np.int32).reshape(-1, 10),
            np.asarray(f_off, dtype=np.int64), np.asarray(w_off, dtype=np.int64))


@dataclass
class TracksPlan:
    """The face tracks `tracks` of one video as one ragged set of clips (tracks_plan)."""
    tracks: tuple            # the track directories, in the order asked for
    rows: np.ndarray         # int64 [n_feat]: the record (= tile) of every feature row, track after track, each in frame order
    present: np.ndarray      # bool [K,T]: present[i, t] = track tracks[i] has a crop of frame t
    static_src: np.ndarray   # clips_plan(present, fps)
    dyn_src: np.ndarray
    windows: np.ndarray
    feat_off: np.ndarray
    win_off: np.ndarray


def tracks_plan(records, tracks, total_frames: int, fps: float) -> TracksPlan:
    """Every track directory of `tracks` as the reference would walk it were it named `00` (get_prob_video.py:79-178): its own
    present mask over the video's `total_frames` frames and `plan_clip` of that mask, laid out one behind the other (clips_plan),
    so that ONE static CNN call over the tiles `rows`, ONE LSTM call over `windows` and two row gathers give all tracks' tables.
    records int64 [n,6] = frame, track directory, box (face_tiles.VideoTiler); host arithmetic only."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, 6)
    present = np.zeros((len(tracks), int(total_frames)), dtype=bool)
    rows = []
    for i, k in enumerate(tracks):
        r = np.flatnonzero(records[:, 1] == int(k))
        r = r[np.argsort(records[r, 0], kind="stable")]
        present[i, records[r, 0]] = True
        rows.append(r)
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return TracksPlan(tuple(int(k) for k in tracks), rows, present, *clips_plan(present, fps))


class _DevicePlan:
    """Index tensors of one (present mask, fps) combination, resident on the device.  Building them costs Python loops
    and host->device copies that serialise behind in-flight GPU work, so they are cached per mask.  `host`: clips_plan's tuple where
    the caller has it; `present` None beside it: a ragged set (run_dataset), whose tiles never lay in a dense clip to select from."""

    def __init__(self, engine: Engine, present, fps, host=None):
        s_src, d_src, win, f_off, w_off = clips_plan(present, fps) if host is None else host
        fb, wb = int(f_off[-1]), int(w_off[-1])
        dev = engine.device
        self.n_feat, self.n_win = fb, wb
        self.sel = None if present is None or fb == present.size else torch.from_numpy(np.nonzero(present.reshape(-1))[0]).to(dev)
        s_src = np.where(s_src >= 0, s_src, fb)
        d_src = np.where(d_src >= 0, d_src, wb)
        assert win.size == 0 or (win.min() >= 0 and win.max() < max(fb, 1))
        self.s_src = torch.from_numpy(s_src).to(dev)
        self.d_src = torch.from_numpy(d_src).to(dev)
        self.win = torch.from_numpy(win).to(dev)
        self.zero_row = torch.zeros(1, 7, device=dev)


def _device_plan(engine: Engine, present: np.ndarray, fps: float, host=None) -> _DevicePlan:
    """Index plans live ON the Engine object (they hold tensors of its device), so they die with it.  `host`: clips_plan(present,
    fps) where the caller has it already."""
    cache = engine.__dict__.setdefault("_plan_cache", {})
    key = (present.shape, present.tobytes(), float(fps))
    plan = cache.get(key)
    if plan is None:
        if len(cache) > 64:
            cache.clear()
        plan = cache[key] = _DevicePlan(engine, present, fps, host)
    return plan


def visual_forward(engine: Engine, frames_u8: torch.Tensor, present, fps: float, mode: int = MODE_DEFAULT):
    """frames_u8 [N,T,H,W,3] (or [T,H,W,3]) RGB tiles, present [N,T] bool.
    Returns (static_probs [N,T,7], dynamic_logits [N,T,7]) float32 in VIDEO column order (DICT_EMO_VIDEO).
    The reference's tables turn float64 when they contain a zero placeholder row; the values are the same."""
    single = frames_u8.dim() == 4
    if single:
        frames_u8 = frames_u8[None]
    present = np.ascontiguousarray(np.asarray(present, dtype=bool).reshape(frames_u8.shape[0], frames_u8.shape[1]))
    n, t = present.shape
    plan = _device_plan(engine, present, fps)
    dev = engine.device
    flat = frames_u8.reshape(n * t, *frames_u8.shape[2:])
    probs = feats = None
    if plan.n_feat:
        frames_sel = flat.to(dev) if plan.sel is None else flat.to(dev).index_select(0, plan.sel)
        _, probs, feats = engine.static_forward(frames_sel, mode)
    stat, dyn, _ = _tables(engine, plan, probs, feats, n * t, mode)
    stat, dyn = stat.view(n, t, 7), dyn.view(n, t, 7)
    return (stat[0], dyn[0]) if single else (stat, dyn)


def _tables(engine: Engine, plan: _DevicePlan, probs, feats, rows: int, mode: int, windows_per_pass=None, passes=None):
    """The window logic's one statement: the static CNN's outputs of the present frames (probs [n_feat,7], feats [n_feat,512], in
    frame order; None when there is none) -> (static table [rows,7], dynamic table [rows,7], the LSTM's logits per window or
    None): the LSTM over the plan's windows, hold-last / zeros rows gathered as the plan says (get_prob_video.py:157-178).
    `windows_per_pass`: the LSTM takes that many windows per call (None: all in one; the logits are the same); `passes`: a list
    that receives the size of every LSTM call."""
    dev = engine.device
    dl = None
    if plan.n_feat:
        stat = torch.cat([probs, plan.zero_row]).index_select(0, plan.s_src)
        if plan.n_win:
            per = plan.n_win if windows_per_pass is None else int(windows_per_pass)
            parts = [engine.dynamic_forward(engine.gather_windows(feats, plan.win[a:a + per], validated=True), mode)
                     for a in range(0, plan.n_win, per)]
            if passes is not None:
                passes.extend(int(p.shape[0]) for p in parts)
            dl = parts[0] if len(parts) == 1 else torch.cat(parts)
            dyn = torch.cat([dl, plan.zero_row]).index_select(0, plan.d_src)
        else:
            dyn = torch.zeros(rows, 7, device=dev)
    else:
        stat = torch.zeros(rows, 7, device=dev)
        dyn = torch.zeros(rows, 7, device=dev)
    return stat, dyn, dl


def visual_from_static(engine: Engine, probs, feats, present, fps: float, mode: int = MODE_DEFAULT, with_windows: bool = False):
    """`visual_forward` behind the static CNN, for a caller that ran it in passes and kept only its outputs: probs [n_feat,7] and
    feats [n_feat,512] (Engine.static_forward) of the PRESENT frames of one clip in frame order, present bool [T] -> (static_probs
    [T,7], dynamic_logits [T,7]), the tables visual_forward returns for that clip -- the same plan, the same LSTM call.
    `with_windows`: the LSTM's logits per window [n_win,7] (None when there is no window) as a third value."""
    present = np.ascontiguousarray(np.asarray(present, dtype=bool).reshape(1, -1))
    plan = _device_plan(engine, present, fps)
    n_rows = 0 if probs is None else int(probs.shape[0])
    if n_rows != plan.n_feat or (plan.n_feat and int(feats.shape[0]) != plan.n_feat):
        raise ValueError(f"visual_from_static: {n_rows} rows of static outputs for {plan.n_feat} present frames")
    stat, dyn, dl = _tables(engine, plan, probs, feats, present.shape[1], mode)
    return (stat, dyn, dl) if with_windows else (stat, dyn)


def visual_from_static_tracks(engine: Engine, probs, feats, tp: TracksPlan, fps: float, mode: int = MODE_DEFAULT):
    """`visual_from_static` for the face tracks of a `tracks_plan`: probs [n_feat,7] and feats [n_feat,512] are the static CNN's
    outputs of the plan's tiles `tp.rows`, in that order -> (static_probs [K,T,7], dynamic_logits [K,T,7]).  One LSTM call holds all
    tracks' windows; track i's tables are what visual_from_static gives for that track alone, bit for bit (the same `_tables`)."""
    present = np.ascontiguousarray(tp.present)
    plan = _device_plan(engine, present, fps, (tp.static_src, tp.dyn_src, tp.windows, tp.feat_off, tp.win_off))
    if int(probs.shape[0]) != plan.n_feat or int(feats.shape[0]) != plan.n_feat:
        raise ValueError(f"visual_from_static_tracks: {int(probs.shape[0])} rows of static outputs for {plan.n_feat} tiles of the plan")
    stat, dyn, _ = _tables(engine, plan, probs, feats, present.size, mode)
    return stat.view(*present.shape, 7), dyn.view(*present.shape, 7)


def read_face_dir(path_images: str, total_frames: int, track: str = "00"):
    """The file side of `preprocess_video_and_predict` (get_prob_video.py:79-100): the face crops stage 0 wrote as
    `<path_images>/<track>/NNNNNN.jpg`, one per frame in which the track was seen.  Returns (frames u8 [total_frames,224,224,3] RGB,
    present bool [total_frames]): frame i is the JPEG `%06d.jpg` decoded to RGB and resized to 224 x 224 with PIL's NEAREST filter --
    the very call `pth_processing` makes (data/utils.py:34) -- or zeros where the file does not exist.  PIL decodes here where the
    reference decodes with cv2.imread; both sit on libjpeg, a decoder difference of a grey level cannot be excluded.
    `os.listdir` of a missing track directory raises FileNotFoundError as in the reference."""
    from PIL import Image

    folder = os.path.join(path_images, track)
    names = set(os.listdir(folder))
    frames = np.zeros((total_frames, 224, 224, 3), dtype=np.uint8)
    present = np.zeros(total_frames, dtype=bool)
    for i in range(total_frames):
        name = str(i).zfill(6) + ".jpg"
        if name in names:
            with Image.open(os.path.join(folder, name)) as img:
                frames[i] = np.asarray(img.convert("RGB").resize((224, 224), Image.Resampling.NEAREST))
            present[i] = True
    return frames, present


def read_face_crops(path_images: str, frame_idx, track: str = "00"):
    """The original-size crops `<path_images>/<track>/NNNNNN.jpg` of the frames `frame_idx`, decoded to RGB (PIL), packed into
    one canvas u8 [m, max h, max w, 3] with rects i32 [m,5] = (i, 0, 0, w, h): the input of Engine.crop_resize_linear.  The
    heat-map base image is cv2.resize of this crop (get_prob_video.py:99-100, data/utils.py:105), not the NEAREST tile."""
    from PIL import Image

    crops = []
    for i in np.asarray(frame_idx).reshape(-1):
        with Image.open(os.path.join(path_images, track, str(int(i)).zfill(6) + ".jpg")) as img:
            crops.append(np.asarray(img.convert("RGB")))
    hmax = max([c.shape[0] for c in crops], default=1)
    wmax = max([c.shape[1] for c in crops], default=1)
    canvas = np.zeros((max(len(crops), 1), hmax, wmax, 3), dtype=np.uint8)
    rects = np.zeros((len(crops), 5), dtype=np.int32)
    for i, c in enumerate(crops):
        canvas[i, :c.shape[0], :c.shape[1]] = c
        rects[i] = (i, 0, 0, c.shape[1], c.shape[0])
    return canvas, rects


def _read_blob(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def read_face_dir_device(engine: Engine, path_images: str, total_frames: int, track: str = "00", threads: int = 0, entropy: str = "host"):
    """`read_face_dir` with the decode on the device (avcer_amd/jpeg.py): the same files, the same meaning, the same
    FileNotFoundError for a missing track directory -> (frames u8 [total_frames,224,224,3] RGB ON THE DEVICE, bit-identical to
    read_face_dir's, present bool [total_frames]).  A file the native parser does not handle is decoded by PIL as there.
    `threads`: host threads of the entropy pass, at most 16 (0: OMP_NUM_THREADS, or 16).  `entropy`: where the files are
    Huffman-decoded, "host" (the default) or "device" (jpeg.decode_tiles); the tiles are the same."""
    from . import jpeg

    folder = os.path.join(path_images, track)
    names = set(os.listdir(folder))
    idx = [i for i in range(total_frames) if str(i).zfill(6) + ".jpg" in names]
    present = np.zeros(total_frames, dtype=bool)
    present[idx] = True
    tiles, _ = jpeg.decode_tiles(engine, [_read_blob(os.path.join(folder, str(i).zfill(6) + ".jpg")) for i in idx], threads, entropy=entropy)
    if len(idx) == total_frames:
        return tiles, present
    frames = torch.zeros(total_frames, 224, 224, 3, dtype=torch.uint8, device=engine.device)
    if idx:
        frames[torch.as_tensor(idx, device=engine.device)] = tiles
    return frames, present


def read_face_crops_device(engine: Engine, path_images: str, frame_idx, track: str = "00", entropy: str = "host"):
    """`read_face_crops` with the decode on the device: (canvas u8 [max(m,1), max h, max w, 3] on the device, rects i32 [m,5])."""
    from . import jpeg

    blobs = [_read_blob(os.path.join(path_images, track, str(int(i)).zfill(6) + ".jpg")) for i in np.asarray(frame_idx).reshape(-1)]
    return jpeg.decode_canvas(engine, blobs, entropy=entropy)[0]


def preprocess_video_and_predict(engine: Engine, path_images: str = "", save_path: str = "", fps: float = 30, total_frames: int = 0,
                                 flag_save_prob: bool = False, mode: int = MODE_DEFAULT, flag_heatmaps: bool = False,
                                 model_heatmaps: str = "static", decode: str = "device", jpeg_entropy: str = "host"):
    """`get_prob_video.preprocess_video_and_predict` (get_prob_video.py:67-204) with the reference's argument meaning, on the HIP
    path: the face-crop directory of one video in, the two per-frame tables out -- (dynamic logits, static probabilities), float32
    [total_frames, 7] in DICT_EMO_VIDEO column order -- and `dynamic__<video>.csv` / `static__<video>.csv` under `save_path` when
    `flag_save_prob` (the reference's files, io_formats.write_visual_csvs).
    `flag_heatmaps`: one Grad-CAM overlay per frame that starts an LSTM evaluation, written as
    `<save_path>/<video>/heatmaps_<model_heatmaps>/NNNNNN.jpg` (avcer_amd/heatmaps.py); the tables are the same as without it.
    The visual call runs through `engine.guarded`, with or without maps.  `model_heatmaps` other than "static" / "dynamic" raises
    ValueError before any work (the reference dies with UnboundLocalError at its first heat-map frame).
    `decode`: "device" reads the crops through read_face_dir_device / read_face_crops_device (host entropy pass, HIP pixel pass),
    "pil" through read_face_dir / read_face_crops; the tiles are bit-identical, so tables, CSV files and heat maps are the same.
    `jpeg_entropy` (with decode="device"): where the files are Huffman-decoded, "host" (the default) or "device"; the same tiles."""
    from . import io_formats

    if decode not in ("device", "pil"):
        raise ValueError(f"decode must be 'device' or 'pil', got {decode!r}")
    if jpeg_entropy not in ("host", "device"):
        raise ValueError(f'jpeg_entropy must be "host" or "device", not {jpeg_entropy!r}')
    if decode == "device":
        def read_dir(p, t):
            return read_face_dir_device(engine, p, t, entropy=jpeg_entropy)

        def read_crops(p, idx):
            return read_face_crops_device(engine, p, idx, entropy=jpeg_entropy)
    else:
        def read_dir(p, t):
            frames, present = read_face_dir(p, t)
            return torch.from_numpy(frames), present

        def read_crops(p, idx):
            canvas, rects = read_face_crops(p, idx)
            return torch.from_numpy(canvas), rects

    hm = None
    if flag_heatmaps:
        from . import heatmaps as hm

        hm.check_model(model_heatmaps)
    frames, present = read_dir(path_images, total_frames)
    if hm is not None:
        frame_idx = hm.heatmap_plan(present, fps)[0]
        canvas, rects = read_crops(path_images, frame_idx)

    def call(m):
        if hm is None:
            return (*visual_forward(engine, frames, present, fps, m), None)
        stat, dyn, cam, _, rows, cls = hm.visual_forward_cam(engine, frames, present, fps, m, model_heatmaps)
        imgs = None
        if len(rows):
            base = engine.crop_resize_linear(canvas, rects, swap_rb=False)
            imgs = engine.cam_render(cam, rows, cls, base, hm.JET_BGR, hm.IMAGE_WEIGHT)
        return stat, dyn, imgs

    # MODE_F16X3: a call during which an activation left fp16's range is repeated in MODE_FP32, maps included (engine.guarded)
    stat, dyn, imgs = engine.guarded(mode, call)
    if imgs is not None:
        hm.write_heatmaps(hm.heatmap_dir(save_path, os.path.basename(path_images), model_heatmaps), frame_idx, imgs, engine=engine)
    if flag_save_prob:
        io_formats.write_visual_csvs(stat, dyn, save_path, os.path.basename(path_images))
    return dyn.cpu().numpy(), stat.cpu().numpy()
