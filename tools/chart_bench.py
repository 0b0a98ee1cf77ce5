"""Cost of the prediction timeline chart (avcer_amd/chart.py, csrc/chart.hip).  Writes profiles/chart_bench.json.
`python tools/chart_bench.py [--reps 5] [--frames 750,100000,4000000] [--charts 1,24] [--parent-json FILE]`.

Convention: `--reps` interleaved repetitions per comparison, median (min..max); every arm asserts identical file bytes before it is
timed.

(a) tables to file bytes, for T in `--frames` and V in `--charts` charts of the default picture (1200 x 200):
      cpu      chart_numpy + PIL Image.save on one thread, from tables on the host (where the CSV writers have them); an arm whose
               one call takes more than `--cpu-once-above-s` seconds is timed by that call alone (`cpu_repetitions` says so);
      device   chart.render + jpeg.encode_images(entropy="device") from tables on the device to file bytes on the host.
(b) the envelope launch alone (Engine.chart_series; device events around envelope + paint + the upload of the plan records): the
    bytes the envelope must read -- 4 series x sum T x 4 bytes -- over that time, beside the streaming-copy ceiling measured in the
    same run (Engine.measure_ceilings).
(c) `run_inference` on a 750-frame 640 x 360 clip with supplied detections: flag_save_plot_pred off against on.
`--parent-json`: the parent commit's timing of the same default call ({"default": [ms...]}, made by this tool's `--parent-arm FILE` with
the environment variable AVCER_BENCH_TREE naming a built checkout of the parent commit), copied into the result."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("AVCER_BENCH_TREE", ROOT))

from avcer_amd import run as arun  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd.engine import MODE_F16X3, Engine  # noqa: E402


def stats(v):
    return {"ms": [round(x, 4) for x in v], "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def event_ms(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def tables(T, V):
    """V class tables [4, T] that change every ~T/40 frames, as predictions do, each chart its own."""
    rng = np.random.default_rng(T + V)
    run = max(T // 40, 1)
    return [np.repeat(rng.integers(0, 7, (4, T // run + 1)), run, axis=1)[:, :T].astype(np.int32) for _ in range(V)]


def charts(eng, a, res):
    from PIL import Image

    from avcer_amd import chart, jpeg

    _, copy_tbs = eng.measure_ceilings()
    res["copy_ceiling_tb_per_s"] = copy_tbs
    res["charts"] = {}
    for T in a.frames:
        for V in a.charts:
            host = tables(T, V)
            plan = chart.chart_plan(T)
            dev = torch.from_numpy(np.concatenate(host, axis=1)).to(eng.device)
            rects = np.zeros((V, 5), dtype=np.int32)
            rects[:, 0], rects[:, 3], rects[:, 4] = np.arange(V), plan.width, plan.height

            def cpu():
                files = []
                for t in host:
                    b = io.BytesIO()
                    Image.fromarray(chart.chart_numpy(t, plan)).save(b, "JPEG", quality=95, subsampling=2)
                    files.append(b.getvalue())
                return files

            def device():
                return jpeg.encode_images(eng, chart.render(eng, dev, T=[T] * V, plan=plan), rects, quality=95, subsampling=2, entropy="device")

            def series():
                return eng.chart_series(dev, [plan] * V, out)

            first_ms, want = wall_ms(cpu)
            slow = first_ms > a.cpu_once_above_s * 1e3  # a CPU arm this slow is timed by that one call alone, and the row says so
            assert [bytes(f) for f in device()] == want, (T, V)                       # identical bytes before any timing
            out = torch.full((V, plan.height, plan.width, 3), 255, dtype=torch.uint8, device=eng.device)
            series()
            ts = {"cpu": [], "device": [], "series": []}
            for _ in range(a.reps):
                if not slow:
                    ts["cpu"].append(wall_ms(cpu)[0])
                ts["device"].append(wall_ms(device)[0])
                ts["series"].append(event_ms(series)[0])
            ts["cpu"] = ts["cpu"] or [first_ms]
            row = {"cpu_chart_numpy_pil_save_1_thread": stats(ts["cpu"]), "device_tables_to_file_bytes": stats(ts["device"]),
                   "chart_series_envelope_and_paint": stats(ts["series"]), "path": chart.PATH_NAMES[plan.path]}
            row["cpu_repetitions"] = len(ts["cpu"])
            must = 4 * T * V * 4
            tbs = must / (row["chart_series_envelope_and_paint"]["median_ms"] * 1e-3) / 1e12
            row["envelope_must_read_bytes"] = must
            row["envelope_tb_per_s"] = tbs
            row["fraction_of_copy_ceiling"] = tbs / copy_tbs
            row["cpu_over_device"] = row["cpu_chart_numpy_pil_save_1_thread"]["median_ms"] / row["device_tables_to_file_bytes"]["median_ms"]
            res["charts"][f"T={T} V={V}"] = row
            del dev, out


def load_models(eng):
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))


def clip(eng, n=750):
    frames = torch.from_numpy(synth.video_frames(77, n, 360, 640)).to(eng.device)
    wav = synth.waveforms(99, 1, int(n / 25 * 16000))[0]
    dets = [np.array([[200 + t % 5, 80, 360 + t % 5, 300, 0.99] + [0] * 10], dtype=np.float32) for t in range(n)]
    return frames, wav, dets


def default_call(eng, frames, wav, dets, **kw):
    return arun.run_inference(eng, frames, wav, 25, detections=dets, mode=MODE_F16X3, **kw)


def in_run_inference(eng, a, res):
    load_models(eng)
    frames, wav, dets = clip(eng)
    with tempfile.TemporaryDirectory() as root:
        arms = {"default": {}, "flag_save_plot_pred": dict(flag_save_plot_pred=True, path_save_results=root)}
        first = {k: default_call(eng, frames, wav, dets, **kw) for k, kw in arms.items()}
        assert all(np.array_equal(first["default"][m], first["flag_save_plot_pred"][m]) for m in ("av", "vs", "vd", "a"))
        ts = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, kw in arms.items():
                ts[k].append(wall_ms(lambda: default_call(eng, frames, wav, dets, **kw))[0])
    res["run_inference_750_frames_640x360"] = {k: stats(v) for k, v in ts.items()}


def parent_arm(eng, a):
    """The default call alone, with no use of anything this tool's tree adds: what runs from the parent's tree."""
    load_models(eng)
    frames, wav, dets = clip(eng)
    default_call(eng, frames, wav, dets)
    out = {"default": stats([wall_ms(lambda: default_call(eng, frames, wav, dets))[0] for _ in range(a.reps)])}
    print(json.dumps(out))
    with open(a.parent_arm, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=lambda s: [int(v) for v in s.split(",")], default=[750, 100000, 4000000])
    ap.add_argument("--charts", type=lambda s: [int(v) for v in s.split(",")], default=[1, 24])
    ap.add_argument("--cpu-once-above-s", type=float, default=10.0, help="a CPU arm slower than this is timed once, not --reps times")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--parent-arm", default=None, help="write the default call's timings alone to this file and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chart_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    if a.parent_arm:
        return parent_arm(eng, a)
    res = {"reps": a.reps, "convention": "interleaved repetitions, median (min..max), every arm asserts identical file bytes before it is timed"}
    charts(eng, a, res)
    in_run_inference(eng, a, res)
    if a.parent_json and os.path.exists(a.parent_json):
        with open(a.parent_json) as f:
            res["parent_commit_default_call"] = json.load(f)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
