"""Grad-CAM heat maps of the static CNN: `flag_heatmaps` / `model_heatmaps` of get_prob_video.preprocess_video_and_predict
(get_prob_video.py:101-155) and run.run_inference (run.py:190-239).

For every frame that starts an LSTM evaluation (present and `i % step == 0`) the reference back-propagates the static softmax
p_k of one class k to layer 4's output, weights layer 4's channels by the spatial mean of that gradient (data/utils.py:92-112)
and blends the map onto the face crop (visualization/visualize.py:218-253).  Here the maps of all 7 classes come out of the
static forward (Engine.static_forward_cam), the class is chosen on the device and the overlays are rendered by
Engine.cam_render; this module holds the frame plan, the class choice, the colour table, the JPEG writer and the numpy statement
of the rendering that the HIP kernels restate bit for bit.
"""
from __future__ import annotations

import os

import numpy as np
import torch

MODELS = ("static", "dynamic")
IMAGE_WEIGHT = 0.8  # get_prob_video.py:145


def check_model(model_heatmaps) -> str:
    """`model_heatmaps` must be "static" or "dynamic".  The reference does not check it: any other value dies with
    UnboundLocalError (`max_idx`) at the first heat-map frame, after work has been done; here it is a ValueError before any."""
    if model_heatmaps not in MODELS:
        raise ValueError(f"model_heatmaps must be one of {MODELS}, got {model_heatmaps!r}")
    return model_heatmaps


def heatmap_plan(present, fps: float):
    """The frames that get a heat map (get_prob_video.py:114,135): present and `i % step == 0`.  Returns int64 arrays
    (frame index, row among the present frames = row of the static tables, LSTM window index = the window ending there)."""
    step = round((5 * fps) / 25)
    if step <= 0:
        raise ZeroDivisionError("integer division or modulo by zero")
    frame, row, win = [], [], []
    nfeat = 0
    for i, p in enumerate(np.asarray(present, dtype=bool).reshape(-1)):
        if p:
            if i % step == 0:
                frame.append(i)
                row.append(nfeat)
                win.append(len(win))
            nfeat += 1
    return np.array(frame, np.int64), np.array(row, np.int64), np.array(win, np.int64)


def choose_classes(model_heatmaps: str, probs_rows: torch.Tensor, dyn_logits_rows: torch.Tensor | None) -> torch.Tensor:
    """get_prob_video.py:136-140 on the device: argmax of the frame's static probabilities, or of the LSTM logits of the window
    ending at the frame; the first index on a tie, as np.argmax.  Either way the map is of the STATIC softmax of that class."""
    src = probs_rows if model_heatmaps == "static" else dyn_logits_rows
    return torch.argmax(src, dim=1).to(torch.int32)


# OpenCV's COLORMAP_JET (modules/imgproc/src/colormap.cpp, class Jet: the MATLAB jet ramps sampled over 256 levels), restated as
# its piecewise-linear closed form -- blue, green and red are clip(1.5 - |4 i/255 - c|, 0, 1) for c = 1, 2, 3 -- and rounded to
# u8.  BGR order, as cv2.applyColorMap returns it.  OpenCV is not available to pin it: a level of difference in some entries
# cannot be excluded.
def _jet_bgr() -> np.ndarray:
    x = np.arange(256, dtype=np.float64) * 4.0 / 255.0
    chans = [np.clip(1.5 - np.abs(x - c), 0.0, 1.0) for c in (1.0, 2.0, 3.0)]
    return np.round(np.stack(chans, axis=1) * 255.0).astype(np.uint8)


JET_BGR = _jet_bgr()


# ----------------------------------------------------------------------------------------------- numpy statement (tests)
def _lin_taps(dsize: int, ssize: int):
    """cv2's INTER_LINEAR table of one axis: source taps and the f32 weight of the second tap (clamped borders)."""
    scale = 1.0 / (dsize / ssize)
    fx = ((np.arange(dsize) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo = sx < 0
    sx[lo], fx[lo] = 0, 0
    hi = sx >= ssize - 1
    sx[hi], fx[hi] = ssize - 1, 0
    return sx, np.minimum(sx + 1, ssize - 1), fx


def resize_linear_u8(img: np.ndarray, out_h: int = 224, out_w: int = 224) -> np.ndarray:
    """cv2.resize(img, (out_w, out_h)) with INTER_LINEAR on u8 HWC (what avcer_crop_resize_linear computes)."""
    h, w = img.shape[:2]
    if (h, w) == (out_h, out_w):
        return img.copy()
    x0, x1, fx = _lin_taps(out_w, w)
    y0, y1, fy = _lin_taps(out_h, h)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    b0 = np.rint((np.float32(1) - fy) * np.float32(2048)).astype(np.int64)[:, None, None]
    b1 = np.rint(fy * np.float32(2048)).astype(np.int64)[:, None, None]
    im = img.astype(np.int64)
    rows = im[:, x0] * a0[None, :, None] + im[:, x1] * a1[None, :, None]
    s0, s1 = rows[y0], rows[y1]
    q = (((s0 >> 4) * b0) >> 16) + (((s1 >> 4) * b1) >> 16)
    return np.clip((q + 2) >> 2, 0, 255).astype(np.uint8)


def resize_linear_map(m: np.ndarray, size: int = 224) -> np.ndarray:
    """cv2.resize(map, (size, size)) with INTER_LINEAR on f32: horizontal pass then vertical, a * w0 + b * w1 each, one
    rounding per operation."""
    h, w = m.shape
    m = m.astype(np.float32)
    x0, x1, fx = _lin_taps(size, w)
    y0, y1, fy = _lin_taps(size, h)
    one = np.float32(1)
    rows = m[:, x0] * (one - fx)[None, :] + m[:, x1] * fx[None, :]
    return rows[y0] * (one - fy)[:, None] + rows[y1] * fy[:, None]


def normalise_map(raw: np.ndarray) -> np.ndarray:
    """data/utils.py:99-101: max(M, 0) / max (0 / 0 = NaN when no value is positive)."""
    m = np.maximum(raw.astype(np.float32), np.float32(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return m / m.max()


def u8_trunc(x: np.ndarray) -> np.ndarray:
    """np.uint8 of f32 values in [0, 255]: truncation; NaN gives 0 (numpy's cast on x86-64, recorded in the golden)."""
    x = np.where(np.isnan(x), np.float32(0), x)
    return x.astype(np.uint8)


def render_overlay(norm_map: np.ndarray, base_rgb: np.ndarray, lut_bgr: np.ndarray = JET_BGR,
                   image_weight: float = IMAGE_WEIGHT) -> np.ndarray:
    """show_cam_on_image(base / 255, resize(map), use_rgb=False, image_weight) (visualize.py:218-253) as numpy computes it:
    u8 BGR [224,224,3]."""
    mask = resize_linear_map(norm_map)
    heat = lut_bgr[u8_trunc(np.float32(255) * mask)]
    heat = heat.astype(np.float32) / np.float32(255)
    img = base_rgb.astype(np.float32) / np.float32(255)
    cam = np.float32(1 - image_weight) * heat + np.float32(image_weight) * img
    cam = cam / cam.max()
    return u8_trunc(np.float32(255) * cam)


# ----------------------------------------------------------------------------------------------- files
def heatmap_dir(save_path: str, video_name: str, model_heatmaps: str) -> str:
    """get_prob_video.py:149-153: <save_path>/<video>/heatmaps_<model>/"""
    return os.path.join(save_path, video_name, f"heatmaps_{model_heatmaps}")


def write_heatmaps(folder: str, frame_idx, images_bgr, engine=None, entropy: str = "host") -> list:
    """cv2.imwrite(<folder>/<NNNNNN>.jpg, overlay) for every heat-map frame (get_prob_video.py:154): JPEG quality 95 (cv2's
    default), the BGR array flipped to RGB first so that the file's colours are the reference's.  With an `engine` and overlays on
    the device the files come from jpeg.encode_images (forward pass on the device, Huffman coding on host threads); else from
    PIL, one file at a time.  `entropy` = "device" moves the Huffman coding to the device as well (jpeg.encode_images).  The bytes
    are the same either way."""
    os.makedirs(folder, exist_ok=True)
    idx = np.asarray(frame_idx).reshape(-1)
    paths = [os.path.join(folder, str(int(i)).zfill(6) + ".jpg") for i in idx]
    if engine is not None and torch.is_tensor(images_bgr) and images_bgr.is_cuda:
        from . import jpeg

        m, h, w = min(len(paths), int(images_bgr.shape[0])), int(images_bgr.shape[1]), int(images_bgr.shape[2])
        rects = np.array([(i, 0, 0, w, h) for i in range(m)], dtype=np.int32).reshape(m, 5)
        for p, blob in zip(paths, jpeg.encode_images(engine, images_bgr, rects, bgr=True, quality=95, subsampling=2, entropy=entropy)):
            with open(p, "wb") as f:
                f.write(blob)
        return paths[:m]
    from PIL import Image

    imgs = images_bgr.cpu().numpy() if torch.is_tensor(images_bgr) else np.asarray(images_bgr)
    paths = paths[:len(imgs)]
    for p, img in zip(paths, imgs):
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(p, quality=95)
    return paths


# ----------------------------------------------------------------------------------------------- device flow
def visual_forward_cam(engine, frames_u8: torch.Tensor, present, fps: float, mode: int, model_heatmaps: str):
    """`video_pipeline.visual_forward` of ONE clip with the maps: frames u8 [T,H,W,3] RGB tiles, present [T].  Returns
    (static_probs [T,7], dynamic_logits [T,7], cam f32 [n_present,7,7,7], frame_idx int64 [m], rows int64 [m], cls int32 [m] on
    the device).  The tables are the ones visual_forward computes (the same kernels), the maps come with them."""
    from .video_pipeline import _device_plan, _tables

    present = np.ascontiguousarray(np.asarray(present, dtype=bool).reshape(1, -1))
    t = present.shape[1]
    plan = _device_plan(engine, present, fps)
    frame_idx, rows, win = heatmap_plan(present[0], fps)
    dev = engine.device
    flat = frames_u8.reshape(t, *frames_u8.shape[-3:])
    cam = torch.zeros(0, 7, 7, 7, device=dev)
    probs = feats = None
    if plan.n_feat:
        frames_sel = flat.to(dev) if plan.sel is None else flat.to(dev).index_select(0, plan.sel)
        _, probs, feats, cam = engine.static_forward_cam(frames_sel, mode)
    stat, dyn, dl = _tables(engine, plan, probs, feats, t, mode)
    return stat, dyn, cam, frame_idx, rows, heatmap_classes(engine, model_heatmaps, probs, dl, rows, win)


def heatmap_classes(engine, model_heatmaps: str, probs, dl, rows, win) -> torch.Tensor:
    """The class of every heat-map frame, int32 [m] on the device: `choose_classes` on the rows `rows` of the static
    probabilities of the present frames and on the windows `win` of the LSTM's logits (both from heatmap_plan)."""
    if probs is None or not len(rows):
        return torch.zeros(0, dtype=torch.int32, device=engine.device)
    r = torch.from_numpy(np.asarray(rows)).to(engine.device)
    w = torch.from_numpy(np.asarray(win)).to(engine.device)
    return choose_classes(model_heatmaps, probs.index_select(0, r), None if dl is None else dl.index_select(0, w))
