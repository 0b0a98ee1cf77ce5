"""Uncompressed BGR frames of an AVI file onto the device -> profiles/dib_bench.json.  One MI355X, one run, the arms interleaved and
repeated (--reps, 5); every figure is the median of the repetitions with (min .. max).  Every arm is checked to give identical
frames before it is timed.  No ratio is fixed in advance: the file records what was seen.

Per size (640 x 360, 1920 x 1080, and 1918 x 1080 whose rows are padded and fall on other alignments) and bit depth (24, 32):
  kernel alone   avcer_dib_frames on a pass of 64 frames whose bytes are resident, device events around 10 launches; time, GB/s read +
                 written (stride * H in, W * H * 3 out per frame) beside the copy ceiling Engine.measure_ceilings gives in this run.
  device path    dib.unpack_frames on the mapped file: chunks into pinned staging, one copy, the kernel (host clock to a synchronise).
  host path      what a host implementation does: mmap -> np.frombuffer -> flip / strip into pinned memory -> one copy to the device,
                 on one thread and on 16.
End to end (640 x 360 and 1920 x 1080, 64 frames, synthetic models, supplied detections): run.run_inference_file on the raw file and
on the Motion-JPEG file of the same frames, and the decode of each alone, to show where the time goes.
Parent commit (--parent DIR: a checkout of the parent commit with its library built): the Motion-JPEG call in child processes that
alternate between DIR and this tree; both series are recorded, and whether their medians differ by more than their spreads."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((640, 360), (1920, 1080), (1918, 1080))
PASS = 64

CHILD = r"""
import json, sys, time
import numpy as np, torch
from avcer_amd import synth
from avcer_amd import run as arun
from avcer_amd.engine import Engine, MODE_F16X3
path, n, w, h, calls = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
eng = Engine(0)
eng.load_static(synth.to_torch(synth.static_state_dict(42)))
eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))
dets = [np.array([[w // 4, h // 4, w // 2, 3 * h // 4, 0.99] + [0] * 10], dtype=np.float32) for _ in range(n)]
out = arun.run_inference_file(eng, path, detections=dets, mode=MODE_F16X3)
ts = []
for _ in range(calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = arun.run_inference_file(eng, path, detections=dets, mode=MODE_F16X3)
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t)
print("RESULT " + json.dumps({"seconds": ts, "av": out["av"].tolist()}))
"""


def stats(values, scale=1.0, digits=4):
    return {"median": round(statistics.median(values) * scale, digits), "min": round(min(values) * scale, digits),
            "max": round(max(values) * scale, digits)}


def pictures(w, h, count, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for _ in range(count):
        f, ph = rng.uniform(0.004, 0.03, (3, 2)), rng.uniform(0, 6.28, 3)
        img = np.stack([127 + 90 * np.sin(f[c, 0] * x + f[c, 1] * y + ph[c]) for c in range(3)], axis=-1) + rng.normal(0, 3.0, (h, w, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def timed(fn, dev):
    import torch

    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t, out


def host_arm(chunks, h, w, bits, bottom_up, host, dev, threads):
    view, row = host.numpy(), w * (bits // 8)

    def one(i):
        rows = np.frombuffer(chunks[i], dtype=np.uint8).reshape(h, -1)[:, :row].reshape(h, w, bits // 8)[:, :, :3]
        np.copyto(view[i], rows[::-1] if bottom_up else rows)

    if threads == 1:
        for i in range(len(chunks)):
            one(i)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(one, range(len(chunks))))
    return host.to(dev, non_blocking=True)


def child(tree, clip, n, w, h, calls):
    env = dict(os.environ, PYTHONPATH=tree)
    r = subprocess.run([sys.executable, "-c", CHILD, clip, str(n), str(w), str(h), str(calls)], cwd=tree, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        raise RuntimeError(f"the child in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}")
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=PASS, help="frames of every clip (a pass is 64)")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dib_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from PIL import Image

    from avcer_amd import avi, dib, synth
    from avcer_amd import run as arun
    from avcer_amd.engine import MODE_F16X3, Engine

    eng = Engine(0)
    dev = eng.device
    _, copy_tbs = eng.measure_ceilings()
    n = a.frames
    res = {"what": "uncompressed BGR AVI frames onto the device; median of the repetitions (min .. max)", "reps": a.reps, "frames": n,
           "frames_per_pass": PASS, "measured_hbm_copy_tb_per_s": copy_tbs, "sizes": {}, "end_to_end": {}}
    tmp = tempfile.mkdtemp()
    for w, h in SIZES:
        pics = [p[..., ::-1] for p in pictures(w, h, 8, seed=w)]
        frames = [pics[i % 8] for i in range(n)]
        for bits in (24, 32):
            path = os.path.join(tmp, f"raw_{w}x{h}_{bits}.avi")
            avi.write_avi_raw(path, frames, 25, pcm=np.zeros((44100 * n // 25, 2), dtype=np.int16), bits=bits, bottom_up=True, opendml=True)
            with avi.open_avi(path, opendml=True) as clip:
                assert (clip.codec, clip.bits, clip.n_frames) == ("DIB", bits, n)
                host = torch.empty(n, h, w, 3, dtype=torch.uint8, pin_memory=True)
                arms = {"device_path_unpack_frames": lambda: dib.unpack_frames(eng, clip.frames, h, w, bits, True),
                        "host_path_1_thread_plus_copy": lambda: host_arm(clip.frames, h, w, bits, True, host, dev, 1),
                        "host_path_16_threads_plus_copy": lambda: host_arm(clip.frames, h, w, bits, True, host, dev, 16)}
                want = torch.from_numpy(dib.unpack_numpy(clip.frames, h, w, bits, True)).to(dev)
                for k, fn in arms.items():  # warm-up, and identical frames before anything is timed
                    assert torch.equal(fn(), want), k
                # the kernel alone: the bytes of a pass resident, 2-byte aligned as in the file
                part = clip.frames[:min(PASS, n)]
                size = len(part[0])
                blob = np.concatenate([np.zeros(2, np.uint8)] + [np.frombuffer(c, dtype=np.uint8) for c in part])
                span = torch.from_numpy(blob).to(dev)[2:]
                table = torch.arange(len(part), dtype=torch.int64, device=dev) * size
                out = torch.empty(len(part), h, w, 3, dtype=torch.uint8, device=dev)
                assert torch.equal(eng.dib_frames(span, table, len(part), h, w, bits, True, out=out), want[:len(part)])
                times = {k: [] for k in arms}
                kernel = []
                for _ in range(a.reps):  # interleaved: what else runs on the host hits every arm alike
                    for k, fn in arms.items():
                        times[k].append(timed(fn, dev)[0])
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    for _ in range(10):
                        eng.dib_frames(span, table, len(part), h, w, bits, True, out=out)
                    ev[1].record()
                    torch.cuda.synchronize(dev)
                    kernel.append(ev[0].elapsed_time(ev[1]) * 1e-4)  # seconds per launch
                moved = len(part) * (size + h * w * 3)
                rate = [moved / t / 1e9 for t in kernel]
                entry = {"frames_per_s": {k: stats([n / t for t in ts], digits=1) for k, ts in times.items()},
                         "kernel_pass_of_64": {"ms": stats(kernel, 1e3), "bytes_read_plus_written": moved, "gb_per_s": stats(rate, digits=1),
                                               "share_of_measured_copy_ceiling": round(statistics.median(rate) / (copy_tbs * 1e3), 4) if copy_tbs else None}}
                res["sizes"][f"{w}x{h}_{bits}bit"] = entry
                print(f"{w}x{h} {bits} bit", json.dumps(entry), flush=True)
                del host, want, out, span
            os.remove(path)
    # end to end, and where the time goes
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    mjpeg_clip = None
    for w, h in SIZES[:2]:
        pics = pictures(w, h, 8, seed=w)
        pcm = np.zeros((44100 * n // 25, 2), dtype=np.int16)
        raw, mjpg = os.path.join(tmp, f"e2e_raw_{w}.avi"), os.path.join(tmp, f"e2e_mjpg_{w}.avi")
        avi.write_avi_raw(raw, [pics[i % 8][..., ::-1] for i in range(n)], 25, pcm=pcm, opendml=True)
        blobs = []
        for p in pics:
            buf = io.BytesIO()
            Image.fromarray(p).save(buf, "JPEG", quality=90, subsampling=2)
            blobs.append(buf.getvalue())
        avi.write_avi(mjpg, [blobs[i % 8] for i in range(n)], 25, pcm=pcm)
        dets = [np.array([[w // 4, h // 4, w // 2, 3 * h // 4, 0.99] + [0] * 10], dtype=np.float32) for _ in range(n)]

        def decode(path):
            with avi.open_avi(path, opendml=True) as f:
                return f.decode_frames(eng)

        arms = {"raw_run_inference_file": lambda: arun.run_inference_file(eng, raw, detections=dets, mode=MODE_F16X3),
                "mjpeg_run_inference_file": lambda: arun.run_inference_file(eng, mjpg, detections=dets, mode=MODE_F16X3),
                "raw_open_and_decode_alone": lambda: decode(raw), "mjpeg_open_and_decode_alone": lambda: decode(mjpg)}
        for fn in arms.values():
            fn()
        times = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                times[k].append(timed(fn, dev)[0])
        res["end_to_end"][f"{w}x{h}"] = {"frames": n, "ms": {k: stats(ts, 1e3, 2) for k, ts in times.items()},
                                          "file_bytes": {"raw": os.path.getsize(raw), "mjpeg": os.path.getsize(mjpg)}}
        print(f"end to end {w}x{h}", json.dumps(res["end_to_end"][f"{w}x{h}"]), flush=True)
        os.remove(raw)
        if mjpeg_clip is None:
            mjpeg_clip = (mjpg, w, h)
        else:
            os.remove(mjpg)
    if a.parent:
        path, w, h = mjpeg_clip
        series = {"parent": [], "this": []}
        same = None
        for _ in range(3):  # alternating child processes, 3 timed calls each
            for name, tree in (("parent", os.path.abspath(a.parent)), ("this", ROOT)):
                r = child(tree, path, n, w, h, 3)
                series[name].extend(r["seconds"])
                same = r["av"] if same is None else same
                assert r["av"] == same, "the parent commit and this tree predict differently"
        spread = max(max(v) - min(v) for v in series.values())
        diff = abs(statistics.median(series["parent"]) - statistics.median(series["this"]))
        res["parent_commit_mjpeg_run_inference_file"] = {
            "clip": f"{w}x{h}, {n} frames", "ms": {k: stats(v, 1e3, 2) for k, v in series.items()}, "median_difference_ms": round(diff * 1e3, 2),
            "largest_spread_ms": round(spread * 1e3, 2), "moved_beyond_the_spread": bool(diff > spread), "same_predictions": True}
        print("parent", json.dumps(res["parent_commit_mjpeg_run_inference_file"]), flush=True)
    os.remove(mjpeg_clip[0])
    os.rmdir(tmp)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
