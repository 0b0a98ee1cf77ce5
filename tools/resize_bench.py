"""Cost of the device resize (Engine.resize_frames, csrc/resize.hip) and of the detector on a smaller copy (detect_size=).
Writes profiles/resize_bench.json.  `python tools/resize_bench.py [--reps 5] [--frames 64] [--video-frames 256] [--skip-run-inference]
[--parent-json FILE]`.

Convention: `--reps` interleaved repetitions per comparison, median (min..max), every arm asserting the identical output.

(a) kernel alone: avcer_resize_frames on `--frames` frames, 1920x1080 -> 640x360 and 1280x720 -> 640x360, bilinear and lanczos, both
    forms, device events around the call; bytes read + written over that time beside the streaming-copy ceiling measured in the same
    run (Engine.measure_ceilings), and the fraction of that roof.
(b) against PIL: the same batch through Image.resize on one thread and on a 16-thread pool, host copies included on both sides (the
    device arm is timed from host frames to host result as well, beside its device-resident figure).
(c) in run_inference: `--video-frames` frames of 1920x1080 with the real detector on synthetic weights (ResNet-50 and MobileNet-0.25),
    detect_size=None against detect_size=(360, 640), interleaved.  Synthetic weights on noise frames give whatever boxes they give;
    a call that ends in the reference's "no face track" error is timed up to that error and marked, and the detector stage alone
    (detector.batch) is timed for both arms in any case.
`--parent-json`: a file with the parent commit's timing of the same detect_size=None call ({"r50": [ms...], "mnet": [ms...]}, made by
running this tool's `--parent-arm FILE` with the environment variable AVCER_BENCH_TREE naming a built checkout of the parent commit, so
that `avcer_amd` is imported from there), copied into the result to show the default did not move."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("AVCER_BENCH_TREE", ROOT))

from avcer_amd import face_tiles as ft  # noqa: E402
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


def kernel_and_pil(eng, a, res):
    from PIL import Image

    from avcer_amd import resize as rs

    pil = {"bilinear": Image.Resampling.BILINEAR, "lanczos": Image.Resampling.LANCZOS}
    _, copy_tbs = eng.measure_ceilings()
    res["measured_hbm_copy_tb_per_s"] = copy_tbs
    res["kernel"], res["against_pil"] = {}, {}
    for (h, w) in ((1080, 1920), (720, 1280)):
        host = synth.video_frames(7, a.frames, h, w)
        dev = torch.from_numpy(host).to(eng.device)
        nbytes = a.frames * 3 * (h * w + 360 * 640)
        for name in ("bilinear", "lanczos"):
            key = f"{w}x{h}->640x360 {name}"
            arms = {"fused": lambda: eng.resize_frames(dev, (360, 640), name, form=rs.FORM_FUSED),
                    "two_pass": lambda: eng.resize_frames(dev, (360, 640), name, form=rs.FORM_TWO_PASS)}
            want = arms["fused"]().cpu()
            assert torch.equal(arms["two_pass"]().cpu(), want)
            ts = {k: [] for k in arms}
            for _ in range(a.reps):
                for k, fn in arms.items():
                    ms, out = event_ms(fn)
                    ts[k].append(ms)
                    assert torch.equal(out.cpu(), want)
            row = {"frames": a.frames, "bytes_read_plus_written": nbytes, "chosen_form": eng.resize_form(h, 360, name)}
            for k, v in ts.items():
                row[k] = stats(v)
                row[k]["tb_per_s"] = nbytes / (row[k]["median_ms"] * 1e-3) / 1e12
                row[k]["fraction_of_copy_ceiling"] = row[k]["tb_per_s"] / copy_tbs
            res["kernel"][key] = row

            # (b) host to host: PIL on 1 and 16 threads against upload + kernel + download
            def one(i):
                return np.asarray(Image.fromarray(host[i]).resize((640, 360), pil[name]))

            def pil_1():
                return np.stack([one(i) for i in range(a.frames)])

            def pil_16():
                with ThreadPoolExecutor(16) as ex:
                    return np.stack(list(ex.map(one, range(a.frames))))

            def device():
                return eng.resize_frames(torch.from_numpy(host).to(eng.device), (360, 640), name).cpu().numpy()

            arms = {"pil_1_thread": pil_1, "pil_16_threads": pil_16, "device_host_to_host": device}
            ts = {k: [] for k in arms}
            for _ in range(a.reps):
                for k, fn in arms.items():
                    ms, out = wall_ms(fn)
                    ts[k].append(ms)
                    assert np.array_equal(out, want.numpy()), (key, k)
            row = {k: stats(v) for k, v in ts.items()}
            row["device_resident_median_ms"] = res["kernel"][key]["fused"]["median_ms"]
            row["device_beats"] = [k for k in ("pil_1_thread", "pil_16_threads") if row["device_host_to_host"]["median_ms"] < row[k]["median_ms"]]
            res["against_pil"][key] = row
        del dev


def detector_of(eng, which):
    sd = synth.to_torch(synth.retina_state_dict(42) if which == "r50" else synth.retina_mnet_state_dict(42))
    return ft.RetinaFacePredictor(eng, sd, threshold=0.8, mode=MODE_F16X3)


def load_models(eng):
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))


def run_inference_arm(eng, det, frames, wav, **kw):
    """(what ended the call, its records or None): the whole call, or the call up to the reference's own error."""
    try:
        out = arun.run_inference(eng, frames, wav, 25, detector=det, mode=MODE_F16X3, **kw)
        return "completed", out
    except (FileNotFoundError, ValueError) as e:
        return f"{type(e).__name__}: {e}"[:160], None


def in_run_inference(eng, a, res):
    load_models(eng)
    n = a.video_frames
    frames = torch.from_numpy(synth.video_frames(77, n, 1080, 1920)).to(eng.device)
    wav = synth.waveforms(99, 1, int(n / 25 * 16000))[0]
    res["run_inference"] = {"video": f"{n} frames of 1920x1080 at 25 fps, synthetic weights, mode x3"}
    for which in ("r50", "mnet"):
        det = detector_of(eng, which)
        arms = {"full_size": {}, "detect_size_360x640": {"detect_size": (360, 640)}}
        row, ends, ts, td = {}, {}, {k: [] for k in arms}, {k: [] for k in arms}
        for k, kw in arms.items():  # warm every shape
            ends[k], first = run_inference_arm(eng, det, frames, wav, **kw)
            row[k + "_first_records"] = None if first is None else int(len(first["records"]))
        wrapped = ft.ScaledDetector(det, (360, 640))
        for _ in range(a.reps):
            for k, kw in arms.items():
                ms, (end, _) = wall_ms(lambda: run_inference_arm(eng, det, frames, wav, **kw))
                assert end == ends[k], (end, ends[k])
                ts[k].append(ms)
                ms, _ = wall_ms(lambda: (wrapped if kw else det).batch(frames, rgb=False))
                td[k].append(ms)
        for k in arms:
            row[k] = dict(stats(ts[k]), ended=ends[k], detector_batch_alone=stats(td[k]))
        row["full_over_resized_run_inference"] = row["full_size"]["median_ms"] / row["detect_size_360x640"]["median_ms"]
        row["full_over_resized_detector_alone"] = (row["full_size"]["detector_batch_alone"]["median_ms"] /
                                                   row["detect_size_360x640"]["detector_batch_alone"]["median_ms"])
        res["run_inference"][which] = row


def parent_arm(eng, a):
    """The detect_size=None call alone, with no use of anything this tool's tree adds: what runs from the parent's tree."""
    load_models(eng)
    n = a.video_frames
    frames = torch.from_numpy(synth.video_frames(77, n, 1080, 1920)).to(eng.device)
    wav = synth.waveforms(99, 1, int(n / 25 * 16000))[0]
    out = {}
    for which in ("r50", "mnet"):
        det = detector_of(eng, which)
        end, _ = run_inference_arm(eng, det, frames, wav)
        ts = []
        for _ in range(a.reps):
            ms, (e2, _) = wall_ms(lambda: run_inference_arm(eng, det, frames, wav))
            assert e2 == end
            ts.append(ms)
        out[which] = dict(stats(ts), ended=end)
    print(json.dumps(out))
    with open(a.parent_arm, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--video-frames", type=int, default=256)
    ap.add_argument("--skip-run-inference", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--parent-arm", default=None, help="write the detect_size=None timings alone to this file and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    if a.parent_arm:
        return parent_arm(eng, a)
    res = {"reps": a.reps, "convention": "interleaved repetitions, median (min..max), every arm asserts the identical output"}
    kernel_and_pil(eng, a, res)
    if not a.skip_run_inference:
        in_run_inference(eng, a, res)
    if a.parent_json and os.path.exists(a.parent_json):
        with open(a.parent_json) as f:
            res["parent_commit_run_inference_full_size"] = json.load(f)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
