#!/usr/bin/env python3
"""Generate tests/golden/gradcam.npz by running the REFERENCE's unmodified get_prob_video.preprocess_video_and_predict with
flag_heatmaps=True (model_heatmaps "static" and "dynamic") on the synthetic weights (seed 42), on CPU.

Run in the build container only (`python tests/golden/make_golden_gradcam.py`), like make_golden.py, whose stubs and in-memory
frame store it reuses (that file is unchanged).  The Grad-CAM maps are the reference's own autograd; what comes after them is
pinned only as far as the stubs go:
  * OpenCV is not installed.  cv2.resize is restated (avcer_amd/heatmaps.py: INTER_LINEAR on f32 for the 7 x 7 map, on u8 with
    11-bit fixed-point weights for the crop), cv2.applyColorMap by the restated COLORMAP_JET table, and cv2.imwrite captures the
    array and the file name.  These three are NOT pinned by this fixture; show_cam_on_image (visualization/visualize.py) and
    get_heatmaps (data/utils.py) run unmodified around them.
  * `data.utils` binds show_cam_on_image at import time: the reference's own function is loaded from its file and bound there.
Stored: file names, the chosen class per heat-map frame (argmax of the reference's own table rows), the normalised 7 x 7 map
that reached cv2.resize, strided samples and SHA-256 of every overlay, and one direct get_heatmaps call on an all-negative map
(the NaN rule: what np.uint8(255 * NaN) gives on this machine).
"""
from __future__ import annotations

import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository root and the reference on sys.path)

from avcer_amd import heatmaps as hm  # noqa: E402
from avcer_amd import synth  # noqa: E402

CASES = {  # two of make_golden's harness presence patterns, both with a gap
    "gap25": (25, [1] * 6 + [0] * 3 + [1] * 7),
    "gap30": (30, [1] * 4 + [0] * 2 + [1] * 10),
}
SIZES = ((224, 224), (150, 131), (97, 203), (224, 224))  # crop (h, w) by frame index % 4
STRIDE = 8


def crop_for(i: int, clip) -> np.ndarray:
    h, w = SIZES[i % 4]
    return clip[i] if (h, w) == (224, 224) else synth.u8(500 + i, "gradcam_crop", (h, w, 3))


def main():
    mg.install_stubs()
    cv2 = sys.modules["cv2"]
    cv2.COLORMAP_JET = 2
    cap = {"maps": [], "u8": [], "writes": []}

    def resize(img, size):
        assert tuple(size) == (224, 224)
        if img.dtype == np.float32:
            m = img.reshape(img.shape[0], img.shape[1])
            cap["maps"].append(m.copy())
            return hm.resize_linear_map(m)
        return hm.resize_linear_u8(img, size[1], size[0])

    def apply_color_map(u8, cmap):
        assert cmap == cv2.COLORMAP_JET
        cap["u8"].append(u8.copy())
        return hm.JET_BGR[u8]

    def imwrite(path, img):
        cap["writes"].append((path, img.copy()))
        return True

    cv2.resize, cv2.applyColorMap, cv2.imwrite = resize, apply_color_map, imwrite
    spec = importlib.util.spec_from_file_location("ref_visualize", os.path.join(mg.REF, "visualization", "visualize.py"))
    vis = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vis)
    import data.utils as du

    du.show_cam_on_image = vis.show_cam_on_image

    sd_s = synth.to_torch(synth.static_state_dict(42))
    sd_d = synth.to_torch(synth.dynamic_state_dict(42))
    real_load, real_listdir, real_makedirs = torch.load, os.listdir, os.makedirs
    torch.load = lambda p, *a, **k: sd_s if "static" in p else sd_d
    import get_prob_video as gpv

    torch.load = real_load
    clip = synth.face_frames(4321, 16)
    out = {}
    for name, (fps, present) in CASES.items():
        mg.FRAME_STORE.clear()
        names = []
        for i, p in enumerate(present):
            if p:
                mg.FRAME_STORE[f"{i:06d}.jpg"] = crop_for(i, clip)
                names.append(f"{i:06d}.jpg")
        out[f"{name}_present"] = np.array(present, dtype=np.bool_)
        out[f"{name}_fps"] = np.array(fps)
        out[f"{name}_crop_hw"] = np.array([crop_for(i, clip).shape[:2] for i in range(16)], dtype=np.int32)
        for model in ("static", "dynamic"):
            cap["maps"].clear(), cap["writes"].clear()
            os.listdir = lambda p, names=names: list(names)
            os.makedirs = lambda *a, **k: None
            try:
                df_d, df_s = gpv.preprocess_video_and_predict(path_images="/nonexistent/clip", save_path="/out", fps=fps,
                                                              total_frames=16, flag_heatmaps=True, model_heatmaps=model)
            finally:
                os.listdir, os.makedirs = real_listdir, real_makedirs
            files = [os.path.relpath(p, "/out") for p, _ in cap["writes"]]
            frames = np.array([int(os.path.basename(f)[:6]) for f in files], dtype=np.int32)
            table = df_s.values if model == "static" else df_d.values
            key = f"{name}_{model}"
            out[f"{key}_files"] = np.array(files)
            out[f"{key}_frames"] = frames
            out[f"{key}_cls"] = np.array([int(np.argmax(table[f])) for f in frames], dtype=np.int32)
            out[f"{key}_maps"] = np.stack(cap["maps"]).astype(np.float32)
            imgs = np.stack([img for _, img in cap["writes"]])
            out[f"{key}_img_samples"] = imgs[:, ::STRIDE, ::STRIDE].copy()
            out[f"{key}_img_sha256"] = np.array([hashlib.sha256(i.tobytes()).hexdigest() for i in imgs])
            out[f"{key}_static"] = df_s.values.astype(np.float64)
            out[f"{key}_dynamic"] = df_d.values.astype(np.float64)
            print(key, files, out[f"{key}_cls"])

    # the NaN rule: every channel weight positive, every activation negative -> max(M, 0) is all zero -> 0 / 0
    cap["maps"].clear(), cap["u8"].clear()
    grad = torch.full((1, 2048, 7, 7), 1e-3)
    act = -torch.rand(1, 2048, 7, 7, generator=torch.Generator().manual_seed(3))
    face = synth.u8(901, "gradcam_nan_face", (224, 224, 3))
    img = du.get_heatmaps({"layer4": (grad,)}, {"layer4": act}, "layer4", face, use_rgb=False, image_weight=0.8)
    assert np.isnan(cap["maps"][0]).all()
    out["nan_u8"] = np.array(np.unique(cap["u8"][0]), dtype=np.uint8)
    out["nan_face"] = face[::STRIDE, ::STRIDE].copy()
    out["nan_img_sha256"] = np.array(hashlib.sha256(img.tobytes()).hexdigest())
    out["nan_img_samples"] = img[::STRIDE, ::STRIDE].copy()
    out["stride"] = np.array(STRIDE)
    np.savez_compressed(os.path.join(HERE, "gradcam.npz"), **out)
    print("nan -> u8", out["nan_u8"], "size", os.path.getsize(os.path.join(HERE, "gradcam.npz")))


if __name__ == "__main__":
    main()
