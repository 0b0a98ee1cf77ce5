"""Cost of the JPEG round trip of face crops (avcer_amd/jpeg.py roundtrip_tiles): the fused call (avcer_jpeg_roundtrip_tiles: forward
DCT, quantisation, dequantisation and inverse DCT in one kernel, then the pixel kernel) against the composition of the kernels that
were there before it (avcer_jpeg_forward into a coefficient buffer, then avcer_jpeg_tiles), on one machine, in one process, arms
alternating within every repeat, device events around 20 back-to-back calls per sample.  Input: --crops 200 x 200 rectangles (the size of
tools/jpeg_bench.py's crops) at scattered, mostly odd offsets of 64 synthetic 360 x 640 BGR frames, quality 95, 4:2:0, warmed.
Then what `faces_via_jpeg=True` adds to one run_inference call: the scripted two-track 96 x 128 clip of
tests/test_gpu_jpeg_roundtrip.py drawn out to --frames frames, option on against option off, alternating, host clock.
Writes profiles/jpeg_roundtrip_bench.json (or --out).  `python tools/jpeg_roundtrip_bench.py [--crops 2048] [--frames 750] [--repeats 7]`."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import jpeg, synth  # noqa: E402
from avcer_amd import run as arun  # noqa: E402
from avcer_amd.engine import MODE_F16X3, Engine  # noqa: E402


def frames_bgr(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """Smooth waves plus noise (what a photograph costs a quantiser), u8 [n,h,w,3]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for t in range(n):
        ph = rng.uniform(0, 6.28, 6)
        a = np.stack([np.sin(xx / (23.0 + 5 * c) + ph[c]) * 60 + np.cos(yy / (31.0 - 4 * c) + ph[3 + c]) * 50 + 128 for c in range(3)], axis=2)
        out[t] = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
    return out


def spread(xs) -> dict:
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


CALLS = 20  # back-to-back calls per sample: a window of some 40 ms and not of 2


def timed(fn) -> float:
    """Device time of one of CALLS back-to-back calls of `fn`, ms."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def kernel_bench(eng, crops: int, repeats: int) -> dict:
    n_src, h, w, side = 64, 360, 640, 200
    src = torch.from_numpy(frames_bgr(n_src, h, w, 7)).to(eng.device)
    rng = np.random.default_rng(11)
    x0, y0 = rng.integers(0, w - side + 1, crops), rng.integers(0, h - side + 1, crops)
    rects = np.stack([rng.integers(0, n_src, crops), x0, y0, x0 + side, y0 + side], axis=1).astype(np.int32)
    desc, blocks = jpeg.plan(eng.lib, [(side, side)] * crops, 95, 2)
    d_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(eng.device)
    r_dev = torch.from_numpy(rects).to(eng.device)
    coeffs = torch.empty(64 * blocks, dtype=torch.int16, device=eng.device)
    tiles = torch.empty(crops, 224, 224, 3, dtype=torch.uint8, device=eng.device)
    got = {}

    def fused():
        got["fused"] = eng.jpeg_roundtrip_tiles(src, r_dev, d_dev, crops, blocks, bgr=True)

    def fused_keep():
        got["fused_keep"] = eng.jpeg_roundtrip_tiles(src, r_dev, d_dev, crops, blocks, bgr=True, keep_coeffs=True)

    def composed():
        eng.jpeg_forward(src, r_dev, d_dev, crops, blocks, bgr=True, out=coeffs)
        got["composed"] = eng.jpeg_tiles(coeffs, d_dev, crops, blocks, out=tiles)

    arms = {"fused": fused, "fused_keep_coeffs": fused_keep, "composed": composed}
    for fn in arms.values():  # warm-up of every arm: workspace growth, code objects, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(got["fused"][0], got["composed"][0]) and torch.equal(got["fused_keep"][0], got["composed"][0]) and
                torch.equal(got["fused_keep"][2], coeffs))
    flags = int(got["fused"][1].sum().item() + got["composed"][1].sum().item())
    t = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    res = {"crops": crops, "size": "200x200 out of 64 BGR frames of 360x640, quality 95, 4:2:0", "blocks": blocks, "repeats": repeats,
           "tiles_and_coefficients_bit_identical": same, "flags_raised": flags,
           "calls_per_sample": CALLS, "samples_ms": t, "ms": {k: spread(v) for k, v in t.items()},
           "crops_per_s": {k: {"median": crops / (statistics.median(v) / 1e3), "min": crops / (max(v) / 1e3), "max": crops / (min(v) / 1e3)}
                           for k, v in t.items()}}
    res["composed_over_fused"] = statistics.median(t["composed"]) / statistics.median(t["fused"])
    res["composed_over_fused_keep_coeffs"] = statistics.median(t["composed"]) / statistics.median(t["fused_keep_coeffs"])
    # the verdict the fused kernel stands or falls by: faster than the composition by more than the spread of the two sample sets
    res["fused_faster_beyond_spread"] = bool(max(t["fused"]) < min(t["composed"]))
    res["coefficient_bytes_not_moved"] = 2 * 128 * blocks
    return res


def clip(frames: int):
    """tests/test_gpu_jpeg_roundtrip.py's clip drawn out: two faces that sway, the second from frame 2 on, the last frame without
    the first."""
    bgr = frames_bgr(min(frames, 50), 96, 128, 47)
    bgr = bgr[np.arange(frames) % len(bgr)]
    dets = []
    for t in range(frames):
        s = 10 * np.sin(t / 20.0)
        d = [[20.4 + s, 12.2 + s / 2, 61.7 + s, 64.3 + s / 2, 0.99]] if t < frames - 1 else []
        if t >= 2:
            d.append([75.0 + s / 2, 30.5, 116.0 + s / 2, 80.9, 0.95])
        dets.append(np.array(d, dtype=np.float32).reshape(-1, 5))
    return bgr, dets


def run_bench(eng, frames: int, repeats: int) -> dict:
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    bgr, dets = clip(frames)
    bgr_dev = torch.from_numpy(bgr).to(eng.device)
    wav = synth.waveforms(99, 1, int(frames / 25 * 16000))[0]

    def call(on):
        t0 = time.perf_counter()
        out = arun.run_inference(eng, bgr_dev, wav, 25, detections=dets, mode=MODE_F16X3, faces_via_jpeg=on)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for on in (False, True, False, True):
        _, out = call(on)
    t = {"off": [], "on": []}
    for _ in range(repeats):
        for name, on in (("off", False), ("on", True)):
            t[name].append(call(on)[0])
    return {"frames": frames, "frame_size": "96x128", "records": int(len(out["records"])), "fps": 25, "repeats": repeats,
            "run_inference_ms": {k: spread(v) for k, v in t.items()},
            "faces_via_jpeg_adds_ms": statistics.median(t["on"]) - statistics.median(t["off"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=750)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_roundtrip_bench.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("at least 5 samples per arm")
    eng = Engine(0)
    res = {"kernels": kernel_bench(eng, a.crops, a.repeats), "run_inference": run_bench(eng, a.frames, a.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
