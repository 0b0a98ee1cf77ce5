"""A folder of unequal videos: a loop of `run_inference` against one `run_dataset` call, on one GPU with synthetic weights.

    python tools/dataset_bench.py [--videos 24] [--reps 5] [--out profiles/dataset_bench.json]

24 videos of 1 to 12 s at 25 and 30 frames per second (synthetic frames, one scripted face per frame, 16 kHz mono audio of the
video's length).  Both paths get the same jobs and give the same bits (tests/test_gpu_dataset.py); what differs is how many
launches, copies and range-contract reads the set costs.  Both are warmed with the whole set first (every shape of the timed
window has run once), then timed alternately, `reps` times each, wall clock around a device synchronisation; the file holds
every sample, the medians, their ratio, the library's GEMM-family launch count per video and the pass sizes used.

    python tools/dataset_bench.py --stream [--reps 5] [--long 2048]      -> profiles/dataset_stream_bench.json

The same 24 videos written as AVI files (uncompressed BGR, so the frames are the set's own; 44.1 kHz stereo PCM of the video's
length): `run_dataset` in memory against stream_frames=64 and =256, and a loop of `run_inference_file(stream_frames=64)` over the
files.  Every arm is first held to the in-memory call's tables, bit for bit, then the arms are timed interleaved; median (min..max)
ms and torch.cuda.max_memory_allocated per arm, measured as tools/stream_bench.py measures it.  One long item beside them, streamed
only: the 2048-frame 1080p Motion-JPEG recording of tools/stream_bench.py as a set of one."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from avcer_amd import build, synth  # noqa: E402
from avcer_amd.dataset import VideoJob, run_dataset  # noqa: E402
from avcer_amd.engine import MODE_DEFAULT, Engine  # noqa: E402
from avcer_amd.run import run_inference  # noqa: E402

H, W, SR = 120, 160, 16000


def make_jobs(n_videos: int):
    seconds = [1 + (11 * k) // max(n_videos - 1, 1) for k in range(n_videos)]
    seconds = [seconds[(7 * k) % n_videos] for k in range(n_videos)]          # long and short videos interleaved
    pool = synth.video_frames(1, 12 * 30 + 8, H, W)
    jobs = []
    for k, s in enumerate(seconds):
        fps = 25 if k % 2 == 0 else 30
        t = s * fps
        frames = pool[k % 8:k % 8 + t]
        # one face per frame, drifting: x0, y0, x1, y1, score, 5 landmarks.  The drift wraps round, and the tracker starts a new
        # track at every jump: track 00 holds the first stretch of each video (an eighth of the set's frames reach the CNN), the
        # frames behind it repeat its last row, as for a recording in which the first face leaves
        dets = []
        for f in range(t):
            x0, y0 = 20 + (f + 3 * k) % 40, 10 + (2 * f + k) % 30
            dets.append(np.array([[x0, y0, x0 + 64, y0 + 72, 0.99] + [0.0] * 10], dtype=np.float32))
        wav = synth.waveforms(100 + k, 1, s * SR + (k % 3) * 1234)[0]
        jobs.append(VideoJob(f"video_{k:02d}", t, H, W, fps, len(wav), detections=dets, load=lambda fr=frames, wv=wav: (fr, wv)))
    return jobs


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


STREAM_ARMS = (("in_memory", None), ("stream_64", 64), ("stream_256", 256))
STREAM_KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")


def spread_ms(secs):
    return {"median": round(1e3 * statistics.median(secs), 2), "min": round(1e3 * min(secs), 2), "max": round(1e3 * max(secs), 2)}


def stream_main(args, engine):
    import tempfile

    from avcer_amd import avi
    from avcer_amd.dataset import video_job_from_avi
    from avcer_amd.run import run_inference_file

    def measured(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        secs, out = timed(fn)
        return secs, torch.cuda.max_memory_allocated(), out

    with tempfile.TemporaryDirectory() as tmp:
        jobs, rng = [], np.random.default_rng(7)
        for j in make_jobs(args.videos):
            frames, _ = j.load()
            pcm = rng.integers(-20000, 20000, (44100 * j.n_frames // int(j.fps), 2)).astype(np.int16)
            path = avi.write_avi_raw(os.path.join(tmp, j.name + ".avi"), frames, int(j.fps), 1, pcm)
            jobs.append(video_job_from_avi(path, detections=j.detections, engine=engine))
        paths = [os.path.join(tmp, j.name + ".avi") for j in jobs]
        kw = dict(mode=args.mode, max_frames_per_pass=args.max_frames_per_pass, max_windows_per_pass=args.max_windows_per_pass)
        arms = {name: (lambda n=n: run_dataset(engine, jobs, stream_frames=n, **kw)) for name, n in STREAM_ARMS}
        arms["run_inference_file_loop_stream_64"] = lambda: [run_inference_file(engine, p, detections=j.detections, mode=args.mode, stream_frames=64)
                                                             for p, j in zip(paths, jobs)]
        # warm-up, and the condition of every timing: the arm's tables are the in-memory call's, bit for bit (NaN equal to NaN)
        ref = arms["in_memory"]()
        for name, fn in arms.items():
            got = fn()
            assert all(np.array_equal(g[k], r[k], equal_nan=True) for g, r in zip(got, ref) for k in STREAM_KEYS), name
            assert isinstance(got, list) and (name.startswith("run_inference_file") or got.passes == ref.passes), name
        secs, peak = {name: [] for name in arms}, {name: 0 for name in arms}
        for _ in range(args.reps):
            for name, fn in arms.items():
                s, p, _ = measured(fn)
                secs[name].append(s)
                peak[name] = max(peak[name], p)
        res = {"tool": "tools/dataset_bench.py --stream", "kernel_source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
               "mode": args.mode, "videos": len(jobs), "frames": sum(j.n_frames for j in jobs), "frame_size": [H, W],
               "files": "AVI, uncompressed BGR 24-bit, PCM 44.1 kHz stereo", "reps": args.reps, "interleaved": True,
               "every_arm_equals_in_memory_bit_for_bit": True, "passes": ref.passes,
               "ms": {name: spread_ms(secs[name]) for name in arms}, "peak_bytes": peak,
               "decoded_bytes_of_the_longest_video": max(j.n_frames for j in jobs) * H * W * 3, "x3_fallbacks": engine.x3_fallbacks}
        if args.long:
            from stream_bench import clip  # the 1080p Motion-JPEG recording of tools/stream_bench.py, `long` frames of it

            long_path = os.path.join(tmp, "long.avi")
            dets = clip(long_path, 1920, 1080, int(args.long))
            long_job = [video_job_from_avi(long_path, detections=dets, engine=engine)]
            res["long_item"] = {"frames": int(args.long), "frame_size": [1080, 1920], "decoded_bytes": int(args.long) * 1080 * 1920 * 3}
            for name, n in STREAM_ARMS[1:]:
                measured(lambda: run_dataset(engine, long_job, stream_frames=n, **kw))
                s, p, _ = measured(lambda: run_dataset(engine, long_job, stream_frames=n, **kw))
                res["long_item"][name] = {"ms": round(1e3 * s, 1), "frames_per_s": round(int(args.long) / s, 1), "peak_bytes": p}
    out = args.out if args.out else os.path.join(ROOT, "profiles", "dataset_stream_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("ms", "peak_bytes", "long_item") if k in res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", action="store_true", help="the streamed arm: run_dataset(stream_frames=N) over AVI files")
    ap.add_argument("--long", type=int, default=2048, help="--stream: frames of the long 1080p item (0: skip)")
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", type=int, default=MODE_DEFAULT)
    ap.add_argument("--max-frames-per-pass", type=int, default=2048)
    ap.add_argument("--max-windows-per-pass", type=int, default=128)
    ap.add_argument("--out", default=None, help="default: profiles/dataset_bench.json, with --stream profiles/dataset_stream_bench.json")
    args = ap.parse_args()

    engine = Engine(0)
    engine.load_static(synth.to_torch(synth.static_state_dict(42)))
    engine.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    engine.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    if args.stream:
        return stream_main(args, engine)
    args.out = args.out or os.path.join(ROOT, "profiles", "dataset_bench.json")
    jobs = make_jobs(args.videos)

    def loop():
        out = []
        for j in jobs:
            fr, wav = j.load()
            out.append(run_inference(engine, fr, wav, j.fps, detections=j.detections, mode=args.mode))
        return out

    def packed():
        return run_dataset(engine, jobs, mode=args.mode, max_frames_per_pass=args.max_frames_per_pass,
                           max_windows_per_pass=args.max_windows_per_pass)

    # warm-up: every shape of both paths once; the launch counts and the equality of the results come from this round
    engine.gemm_stats(reset=True)
    ref = loop()
    torch.cuda.synchronize()
    launches_loop = engine.gemm_stats(reset=True)[0]
    got = packed()
    torch.cuda.synchronize()
    launches_packed = engine.gemm_stats(reset=True)[0]
    same = all(np.array_equal(g[k], r[k], equal_nan=True) for g, r in zip(got, ref)
               for k in ("av", "compound_prob", "static_probs", "dynamic_logits", "audio_rows"))
    t_loop, t_packed = [], []
    for _ in range(args.reps):                                                # alternating: drift of a shared host hits both
        t_loop.append(timed(loop)[0])
        t_packed.append(timed(packed)[0])
    m_loop, m_packed = statistics.median(t_loop), statistics.median(t_packed)
    duration = sum(j.n_frames / j.fps for j in jobs)
    res = {
        "tool": "tools/dataset_bench.py", "kernel_source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
        "mode": args.mode, "videos": len(jobs), "seconds_of_video": duration, "frames": sum(j.n_frames for j in jobs),
        "audio_windows": sum(len(range(0, j.n_samples + 1, SR // 2)) for j in jobs), "frame_size": [H, W],
        "video_seconds": [j.n_frames // int(j.fps) for j in jobs], "video_fps": [j.fps for j in jobs],
        "reps": args.reps, "run_inference_loop_s": t_loop, "run_dataset_s": t_packed,
        "run_inference_loop_median_s": m_loop, "run_dataset_median_s": m_packed, "loop_over_packed": m_loop / m_packed,
        "real_time_factor_loop": m_loop / duration, "real_time_factor_packed": m_packed / duration,
        "gemm_family_launches_per_video_loop": launches_loop / len(jobs),
        "gemm_family_launches_per_video_packed": launches_packed / len(jobs),
        "max_frames_per_pass": args.max_frames_per_pass, "max_windows_per_pass": args.max_windows_per_pass,
        "passes": got.passes, "results_identical": bool(same), "x3_fallbacks": engine.x3_fallbacks,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("run_inference_loop_median_s", "run_dataset_median_s", "loop_over_packed",
                                          "gemm_family_launches_per_video_loop", "gemm_family_launches_per_video_packed",
                                          "results_identical")}))


if __name__ == "__main__":
    main()
