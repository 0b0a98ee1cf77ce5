"""Cost of the Grad-CAM heat maps: the static forward against avcer_static_forward_cam at 256 frames, and the overlay
rendering (avcer_crop_resize_linear + avcer_cam_render) of 125 images, about the LSTM step frames of a 30 s clip at 25 fps.
Writes profiles/gradcam_bench.json.  `python tools/gradcam_bench.py [--frames 256] [--images 125] [--iters 20]`."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import heatmaps as hm  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine  # noqa: E402


def _time(fn, iters: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--images", type=int, default=125)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    eng = Engine(0)
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    frames = torch.from_numpy(synth.face_frames(3, a.frames)).cuda()
    res = {"frames": a.frames, "images": a.images, "iters": a.iters}
    for name, mode in (("x3", MODE_F16X3), ("fp32", MODE_FP32)):
        plain = _time(lambda: eng.static_forward(frames, mode), a.iters)
        cam = _time(lambda: eng.static_forward_cam(frames, mode), a.iters)
        res[name] = {"static_forward_ms": plain, "static_forward_cam_ms": cam, "cam_overhead_pct": 100.0 * (cam - plain) / plain}
    *_, maps = eng.static_forward_cam(frames[:a.images], MODE_F16X3)
    canvas = torch.from_numpy(synth.u8(5, "bench_canvas", (a.images, 180, 150, 3))).cuda()
    rects = torch.tensor([[i, 0, 0, 150, 180] for i in range(a.images)], dtype=torch.int32)
    rows = torch.arange(a.images, dtype=torch.int32)
    cls = (rows % 7).cuda()
    lut = torch.from_numpy(hm.JET_BGR).cuda()
    base = eng.crop_resize_linear(canvas, rects)
    res["crop_resize_ms"] = _time(lambda: eng.crop_resize_linear(canvas, rects), a.iters)
    res["cam_render_ms"] = _time(lambda: eng.cam_render(maps, rows, cls, base, lut, 0.8), a.iters)
    res["render_images_per_s"] = a.images / ((res["crop_resize_ms"] + res["cam_render_ms"]) / 1e3)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gradcam_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
