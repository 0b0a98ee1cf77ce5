"""run.run_inference_file in memory against stream_frames=N, in one run on one GPU -> profiles/stream_bench.json.

  throughput      640 x 360 x 750 frames and 1920 x 1080 x 256 frames (the clips of tools/avi_bench.py): the in-memory call -- the
                  parent's path, untouched -- against stream_frames in {64, 256}; `--reps` interleaved repetitions, frames/s as
                  median (min..max), torch.cuda.max_memory_allocated of every arm.  All arms get the same per-frame detections
                  (one synthetic face per frame: no detector weights are needed, and every arm does the same work behind them).
  length          one 1080p run of 2048 frames (the 256 blobs repeated), streamed only: its peak memory beside the 256-frame arm's.
  result video    stream_frames=256 with path_save_video against without: the second decode sweep, draw and encode, beside the
                  decode rate profiles/avi_decode_bench.json measured.
The models are the synthetic ones of the test suite (avcer_amd.synth); the arithmetic is the product's.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from avcer_amd import avi, synth  # noqa: E402
from avcer_amd import run as arun  # noqa: E402
from avcer_amd.engine import MODE_F16X3, Engine  # noqa: E402
from avi_bench import DISTINCT, SIZES, pictures  # noqa: E402

ARMS = (("in_memory", None), ("stream_64", 64), ("stream_256", 256))


def clip(path, w, h, n):
    import io

    from PIL import Image

    blobs = []
    for img in pictures(w, h, DISTINCT, seed=w):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    pcm = np.zeros((44100 * n // 25, 2), dtype=np.int16)
    avi.write_avi(path, [blobs[i % DISTINCT] for i in range(n)], 25, pcm=pcm)
    # one face per frame, drifting: track 00 lives through the clip
    return [np.array([[w // 4 + t % 7, h // 4, w // 4 + t % 7 + h // 2, h // 4 + h // 2, 0.99] + [0] * 10], dtype=np.float32) for t in range(n)]


def one(eng, path, dets, n_stream, **kw):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = arun.run_inference_file(eng, path, detections=dets, mode=MODE_F16X3, stream_frames=n_stream, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated(), out


def spread(frames, secs):
    r = [frames / s for s in secs]
    return {"median": round(statistics.median(r), 1), "min": round(min(r), 1), "max": round(max(r), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsals)")
    ap.add_argument("--long", type=int, default=2048, help="frames of the long 1080p run (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    args = ap.parse_args()
    eng = Engine(0)
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    res = {"what": "run_inference_file: frames/s, median of the interleaved repetitions (min, max); peak = torch.cuda.max_memory_allocated",
           "reps": args.reps, "detections": "one synthetic face per frame, the same arrays for every arm", "mode": "F16X3", "sizes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for w, h, n in SIZES:
            n = max(8, int(n * args.scale))
            path = os.path.join(tmp, f"{w}x{h}.avi")
            dets = clip(path, w, h, n)
            ref = one(eng, path, dets, None)[2]                                             # warm-up, and the reference
            secs = {name: [] for name, _ in ARMS}
            peak = {name: 0 for name, _ in ARMS}
            same = True
            for _ in range(args.reps):
                for name, ns in ARMS:
                    s, p, out = one(eng, path, dets, ns)
                    secs[name].append(s)
                    peak[name] = max(peak[name], p)
                    same = same and all(np.array_equal(out[k], ref[k], equal_nan=True) for k in ("av", "compound_prob", "static_probs", "dynamic_logits"))
            entry = {"frames": n, "arms_agree_bit_for_bit": bool(same),
                     "frames_per_s": {name: spread(n, secs[name]) for name, _ in ARMS},
                     "peak_bytes": peak, "passes": {name: (1 if ns is None else -(-n // ns)) for name, ns in ARMS}}
            mem, st = entry["frames_per_s"]["in_memory"], entry["frames_per_s"]["stream_256"]
            allowed = (mem["max"] - mem["min"]) / mem["median"] + 0.05
            entry["stream_256_slower_by"] = round(1.0 - st["median"] / mem["median"], 4)
            entry["allowed_by_spread_plus_5_percent"] = round(allowed, 4)
            entry["ms_per_pass_over_in_memory"] = {name: round(1e3 * (statistics.median(secs[name]) - statistics.median(secs["in_memory"])) /
                                                               entry["passes"][name], 3) for name, _ in ARMS[1:]}
            if (w, h) == (1920, 1080):
                s0 = statistics.median(one(eng, path, dets, 256)[0] for _ in range(3))
                s1 = statistics.median(one(eng, path, dets, 256, path_save_video=os.path.join(tmp, "out.avi"))[0] for _ in range(3))
                entry["result_video_stream_256"] = {"seconds_without": round(s0, 4), "seconds_with": round(s1, 4),
                                                    "extra_ms_per_frame": round(1e3 * (s1 - s0) / n, 3)}
                bench = os.path.join(ROOT, "profiles", "avi_decode_bench.json")
                if os.path.exists(bench):
                    with open(bench) as f:
                        rate = json.load(f)["sizes"]["1920x1080"]["frames_per_s"]["decode_frames_entropy_device"]["median"]
                    entry["result_video_stream_256"]["second_decode_ms_per_frame_at_avi_decode_bench_rate"] = round(1e3 / rate, 3)
                if args.long:
                    with avi.open_avi(path) as a:
                        blobs = [bytes(f) for f in a.frames]
                    m = int(args.long)
                    long_path = os.path.join(tmp, "long.avi")
                    avi.write_avi(long_path, [blobs[i % len(blobs)] for i in range(m)], 25, pcm=np.zeros((44100 * m // 25, 2), dtype=np.int16))
                    del blobs
                    s, p, _ = one(eng, long_path, [dets[i % n] for i in range(m)], 256)
                    entry["long_run_stream_256"] = {"frames": m, "frames_per_s": round(m / s, 1), "peak_bytes": p,
                                                    "peak_bytes_of_the_%d_frame_arm" % n: peak["stream_256"]}
            res["sizes"][f"{w}x{h}"] = entry
            print(json.dumps({f"{w}x{h}": entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
