"""Cost of the audio front end (Engine.resample: int16 stereo at 44.1 kHz -> float32 mono at 16 kHz in one launch).
Writes profiles/resample_bench.json.  `python tools/resample_bench.py [--iters 40] [--pairs 7] [--no-run-inference]`.

* per-call time between two HIP events around ONE call (warm, median): the kernel plus what the stream waits for the host's
  launch, for 30 s and 10 min of source audio; the same figure for a one-sample call of the same entry (conversion alone: one
  block, one thread) is the launch-cost floor of this path;
* stream time per call of `--burst` calls queued back to back between two events: what a call costs when launches overlap;
* compulsory bytes (source read once + output written once) over those times, beside the streaming-copy ceiling measured on
  this GPU in the same run (Engine.measure_ceilings);
* for context, the CPU restatement (tests/test_resample_cpu.py: float32 conv1d, torch threads as the environment sets them);
* run_inference on the 30 s video of bench.py with wav_sr=44100 (A) against the same call on the pre-resampled waveform (B),
  interleaved A/B: medians, their difference, and the run-to-run spread of each arm."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the CPU context figure runs the tests' restatement of torchaudio's resampler
# (tests/test_resample_cpu.py: sinc_resample_kernel, apply_sinc_resample_kernel, reference_mono); the run_inference arms use
# bench.py's scripted face track (scripted_detections), so that the video is the one `configs.run_inference` measures

from avcer_amd import run as arun  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd.audio_pipeline import resample_out_len, resample_plan  # noqa: E402
from avcer_amd.engine import MODE_F16X3, Engine  # noqa: E402

ORIG, NEW = 44100, 16000


def _per_call_us(fn, iters: int):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def _burst_us(fn, burst: int, reps: int = 5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(burst):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e3 / burst)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--no-run-inference", action="store_true")
    a = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    plan = resample_plan(ORIG, NEW)
    _, copy_tbs = eng.measure_ceilings()
    res = {"pair": [ORIG, NEW], "source": "int16 stereo, interleaved", "iters": a.iters, "burst": a.burst,
           "taps_per_phase": plan.span, "phases": plan.n, "measured_hbm_copy_tb_per_s": copy_tbs, "cases": {}}
    rng = np.random.default_rng(5)
    one = torch.zeros(1, 2, dtype=torch.int16, device=dev)
    floor = _per_call_us(lambda: eng.resample(one, NEW, NEW), a.iters)
    res["launch_floor_us"] = {"what": "one-sample call of the same entry (conversion alone, one block)", "per_call_median": floor[0],
                              "per_call_min": floor[1], "per_call_max": floor[2],
                              "burst_per_call": _burst_us(lambda: eng.resample(one, NEW, NEW), a.burst)}
    srcs = {}
    for name, seconds in (("30s", 30), ("10min", 600)):
        length = seconds * ORIG
        pcm = rng.integers(-32768, 32768, size=(length, 2), dtype=np.int16)
        src = torch.from_numpy(pcm).to(dev)
        srcs[name] = pcm
        n_out = resample_out_len(length, plan.o, plan.n)
        nbytes = length * 2 * 2 + n_out * 4
        med, lo, hi = _per_call_us(lambda: eng.resample(src, ORIG, NEW), a.iters)
        burst = _burst_us(lambda: eng.resample(src, ORIG, NEW), a.burst)
        res["cases"][name] = {"source_samples_per_channel": length, "n_out": n_out, "compulsory_bytes": nbytes,
                              "per_call_us_median": med, "per_call_us_min": lo, "per_call_us_max": hi, "burst_us_per_call": burst,
                              "tb_per_s_per_call": nbytes / (med * 1e-6) / 1e12, "tb_per_s_burst": nbytes / (burst * 1e-6) / 1e12,
                              "bytes_over_copy_ceiling_us": nbytes / (copy_tbs * 1e12) * 1e6}
        del src
    # context: the reference's arithmetic on the host
    from test_resample_cpu import apply_sinc_resample_kernel, reference_mono, sinc_resample_kernel

    cpu = {"torch_threads": torch.get_num_threads()}
    kern = sinc_resample_kernel(ORIG, NEW)
    apply_sinc_resample_kernel(reference_mono(srcs["30s"][:ORIG]), *kern)
    for name, pcm in srcs.items():
        t0 = time.perf_counter()
        mono = reference_mono(pcm)
        t1 = time.perf_counter()
        k = apply_sinc_resample_kernel(mono, *kern)
        cpu[name] = {"int16_to_mono_ms": (t1 - t0) * 1e3, "float32_conv1d_ms": (time.perf_counter() - t1) * 1e3, "n_out": int(k.numel())}
    res["cpu_restatement"] = cpu
    if not a.no_run_inference:
        from bench import scripted_detections

        eng.load_static(synth.to_torch(synth.static_state_dict(42)))
        eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
        eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))
        seconds, fps, h, w = 30, 25, 360, 640
        n = seconds * fps
        frames = torch.from_numpy(synth.video_frames(77, n, h, w)).to(dev)
        dets = scripted_detections(n, h, w)
        src = torch.from_numpy((srcs["30s"].astype(np.float32) * 0.3).astype(np.int16)).to(dev)
        wav16 = eng.resample(src, ORIG, NEW).clone()
        arms = {"A_wav_sr_44100": lambda: arun.run_inference(eng, frames, src, fps, detections=dets, mode=MODE_F16X3, wav_sr=ORIG),
                "B_pre_resampled": lambda: arun.run_inference(eng, frames, wav16, fps, detections=dets, mode=MODE_F16X3)}
        for fn in arms.values():
            fn()
            fn()
        ts = {k: [] for k in arms}
        for _ in range(a.pairs):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        ri = {"video": f"{seconds} s at {fps} fps, {w}x{h}, scripted face track, mode x3", "pairs": a.pairs}
        for k, v in ts.items():
            ri[k] = {"ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "stdev_ms": statistics.stdev(v)}
        ri["A_minus_B_median_ms"] = ri["A_wav_sr_44100"]["median_ms"] - ri["B_pre_resampled"]["median_ms"]
        ri["spread_ms"] = max(r["max_ms"] - r["min_ms"] for r in (ri["A_wav_sr_44100"], ri["B_pre_resampled"]))
        ri["difference_inside_spread"] = abs(ri["A_minus_B_median_ms"]) <= ri["spread_ms"]
        res["run_inference_ab"] = ri
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "resample_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
