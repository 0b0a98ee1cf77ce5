#!/usr/bin/env python3
"""Throughput of the face detector networks (row f4) on synthetic video frames, per arithmetic mode.

    face_bench.py [--model resnet50|mobilenet0.25|s3fd]   the table of one model (default: resnet50)
    face_bench.py --compare [--out FILE]                  the three models on 750 frames of 640 x 360 in ONE process: warmed,
                                                          alternating, five samples each -> profiles/s3fd_face_bench.json, with
                                                          S3FD against RetinaFace-R50 scaled by work and the time of S3FD's MFMA
                                                          families; fails unless the MobileNet-0.25 detector is the fastest."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avcer_amd import build, synth  # noqa: E402
from avcer_amd.engine import Engine, MODE_BF16, MODE_F16X3, MODE_FP32  # noqa: E402

STATE_DICTS = {"resnet50": synth.retina_state_dict, "mobilenet0.25": synth.retina_mnet_state_dict, "s3fd": synth.s3fd_state_dict}
S3FD_GFLOP, R50_GFLOP = 144.27, 50.7   # algorithmic GFLOP per 640 x 360 frame


def mnet_bytes_per_frame(h, w):
    """Compulsory HBM bytes of the MobileNet path per frame: every activation written once and read once by each consumer (f32 NHWC),
    the u8 frame; weights (1.7 MB in all) not counted."""
    c = lambda v: (v - 1) // 2 + 1
    h, w = c(h), c(w)
    total = (2 * h) * (2 * w) * 3 + h * w * 8 * 4
    blocks = [(8, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2)] + [(128, 128, 1)] * 5 + [(128, 256, 2), (256, 256, 1)]
    lv = []
    for i, (ci, co, s) in enumerate(blocks):
        oh, ow = (c(h), c(w)) if s == 2 else (h, w)
        total += 4 * (h * w * ci + oh * ow * co)
        h, w = oh, ow
        if i in (4, 10, 12):
            lv.append((h * w, co))
    for i, (m, cin) in enumerate(lv):
        total += 4 * m * (cin + 64)                     # lateral
        if i < 2:
            total += 4 * m * (3 * 64 + 2 * 64)          # upsample-add (read 2, write 1), merge (read, write)
        total += 4 * m * (64 + 32 + 64 + 16 + 16 + 16 + 16 + 16 + 16 + 16)  # SSH: c3, c51, c52, c72, c73
        total += 4 * m * (64 + 32 + 32 + 32)            # heads: merged 1x1, scatter
    return total


def table(model):
    eng = Engine(0)
    eng.load_face(synth.to_torch(STATE_DICTS[model](42)))
    modes = (("fp32", MODE_FP32), ("x3", MODE_F16X3)) + ((("bf16", MODE_BF16),) if model == "resnet50" else ())
    for h, w, n in ((360, 640, 32), (720, 1280, 8)):
        if model == "s3fd":
            eng.face_forward(torch.from_numpy(synth.video_frames(3, 2, h, w)).cuda(), MODE_FP32)  # lazy copies before the timing
        frames = torch.from_numpy(synth.video_frames(3, 2, h, w)).cuda().repeat(n // 2, 1, 1, 1)
        for name, mode in modes:
            for _ in range(2):
                eng.face_forward(frames, mode)
            torch.cuda.synchronize()
            eng.gemm_stats(reset=True)
            t0 = time.perf_counter()
            for _ in range(3):
                eng.face_forward(frames, mode)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 3
            launches, flops = eng.gemm_stats(reset=True)
            print(f"{h}x{w} batch {n:3d} {name:5s}: {dt * 1e3:8.2f} ms  {n / dt:8.1f} frames/s  "
                  f"{flops / 3 / dt / 1e12:6.1f} TFLOP/s algorithmic ({flops / 3 / n / 1e9:.1f} GFLOP/frame)")


def compare(out, n=750, h=360, w=640, samples=5, mode=MODE_F16X3):
    engines = {}
    for model, make in STATE_DICTS.items():
        engines[model] = Engine(0)
        engines[model].load_face(synth.to_torch(make(42)))
    frames = torch.from_numpy(synth.video_frames(3, 6, h, w)).cuda().repeat(n // 6, 1, 1, 1)
    _, copy_tbs = engines["resnet50"].measure_ceilings()
    launches, gflop = {}, {}
    for model, eng in engines.items():  # warm-up: lazy weight copies, workspaces, clocks
        for _ in range(2):
            eng.face_forward(frames, mode)
        torch.cuda.synchronize()
        eng.gemm_stats(reset=True)
        eng.face_forward(frames, mode)
        torch.cuda.synchronize()
        k, f = eng.gemm_stats(reset=True)
        launches[model], gflop[model] = int(k), f / n / 1e9
    ms = {m: [] for m in engines}
    for _ in range(samples):
        for model, eng in engines.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.face_forward(frames, mode)
            torch.cuda.synchronize()
            ms[model].append((time.perf_counter() - t0) * 1e3)
    res = {"frames": n, "height": h, "width": w, "mode": "x3", "samples": samples, "kernel_source_hash": build.source_hash(),
           "hbm_copy_ceiling_tbs": copy_tbs, "models": {}}
    for model in engines:
        v = ms[model]
        res["models"][model] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "ms_samples": v,
                                "launches_per_batch": launches[model], "gflop_per_frame": gflop[model]}
    b = mnet_bytes_per_frame(h, w)
    t = res["models"]["mobilenet0.25"]["ms_median"] * 1e-3
    res["models"]["mobilenet0.25"].update(bytes_per_frame=b, achieved_tbs=b * n / t / 1e12,
                                          fraction_of_copy_ceiling=b * n / t / 1e12 / copy_tbs if copy_tbs else None)
    print(json.dumps(res))
    # S3FD against the R50 detector of the same run, scaled by work, and where its time goes: one more pass under the event
    # profile (one lane, every MFMA launch timed), the rest being the stem, the pools and the heads
    r50, s3 = res["models"]["resnet50"]["ms_median"], res["models"]["s3fd"]["ms_median"]
    eng = engines["s3fd"]
    eng.profile_enable(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.face_forward(frames, mode)
    torch.cuda.synchronize()
    one_lane_ms = (time.perf_counter() - t0) * 1e3
    fams = eng.profile_read_families()
    eng.profile_enable(False)
    res["models"]["s3fd"].update(r50_scaled_by_work_ms=r50 * S3FD_GFLOP / R50_GFLOP, ratio_to_r50_scaled_by_work=s3 / (r50 * S3FD_GFLOP / R50_GFLOP),
                                 tflops_algorithmic=S3FD_GFLOP * n / s3 / 1e3, profiled_one_lane_ms=one_lane_ms, families=fams)
    print(json.dumps(res["models"]["s3fd"]))
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not res["models"]["mobilenet0.25"]["ms_median"] < min(r50, s3):
        raise SystemExit("the MobileNet-0.25 detector is not the fastest of the three: something is broken")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=sorted(STATE_DICTS), default="resnet50")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s3fd_face_bench.json"))
    a = ap.parse_args()
    compare(a.out) if a.compare else table(a.model)
