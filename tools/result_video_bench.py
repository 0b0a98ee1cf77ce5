"""The result video, four ways, in one run -> profiles/result_video_bench.json.

The frames of a clip lie on the device (as jpeg.decode_frames leaves them) with one tracked face box and a prediction per frame.
Timed, interleaved and repeated, from there to the finished Motion-JPEG AVI file:
  (a) frames to the host, then per frame PIL's ImageDraw of annotate.layout's items, Image.save (quality 90, 4:2:0) and
      avi.write_avi, on one thread;
  (b) the same on a pool of 16 threads;
  (c) annotate.write_result_video with entropy="host";
  (d) annotate.write_result_video with entropy="device";
at 640 x 360 (750 frames) and 1920 x 1080 (256 frames).  Every arm ends with the file on disk and is timed with the host clock
(each ends in host work behind a device synchronise); the tool asserts that all arms write identical files.  Reported per arm:
frames/s of the median repetition and the spread (min, max).  avcer_annotate_frames alone is timed with device events on one pass
of 64 frames, with the bytes it touches beside the copy figure of Engine.measure_ceilings, and the time path_save_video adds to
run_inference_file is measured on the small clip.  No figure is fixed in advance: the file records what was seen."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from avi_bench import pictures  # noqa: E402

from avcer_amd import annotate as an  # noqa: E402
from avcer_amd import avi, synth  # noqa: E402
from avcer_amd import run as arun  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402

SIZES = ((640, 360, 750), (1920, 1080, 256))  # width, height, frames
DISTINCT = 16


def scene(w, h, n, seed=0):
    """A face box that drifts through the frame, a second track now and then, and a prediction per frame."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    bw, bh = w // 4, h // 2
    x0 = (w // 3 + (w // 5) * np.sin(t / 40.0)).astype(np.int64)
    y0 = (h // 4 + (h // 8) * np.cos(t / 55.0)).astype(np.int64)
    records = [[k, 0, x0[k], y0[k], x0[k] + bw, y0[k] + bh] for k in t]
    records += [[k, 1, w - w // 6, h // 10, w - w // 20, h // 3] for k in t[::3]]
    prob = rng.dirichlet(np.ones(7) * 0.7, size=n)
    return np.array(records, dtype=np.int64), prob.argmax(axis=1).astype(np.int32), prob


def pil_arm(frames_dev, items, masks, path, rate, pcm, threads):
    from PIL import Image, ImageDraw

    host = frames_dev.cpu().numpy()
    pil_masks = [Image.fromarray(m) for m in masks]
    first = np.searchsorted(items["frame"], np.arange(len(host) + 1))

    def one(i):
        im = Image.fromarray(np.ascontiguousarray(host[i][..., ::-1]))  # BGR frames; the colours below are reversed to match
        d = ImageDraw.Draw(im)
        for it in items[first[i]:first[i + 1]]:
            colour = tuple(int(c) for c in it["colour"][::-1])
            x0, y0, x1, y1, a = (int(it[k]) for k in ("x0", "y0", "x1", "y1", "arg"))
            if it["kind"] == an.OUTLINE:
                d.rectangle((x0, y0, x1, y1), outline=colour, width=a)
            elif it["kind"] == an.FILL:
                d.bitmap((x0, y0), Image.new("L", (x1 - x0 + 1, y1 - y0 + 1), a), fill=colour)
            else:
                m = pil_masks[int(it["mask"])]
                d.bitmap((x0, y0), m if a == 1 else m.resize((a * m.width, a * m.height), Image.NEAREST), fill=colour)
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=90, subsampling=2)
        return buf.getvalue()

    if threads == 1:
        blobs = [one(i) for i in range(len(host))]
    else:
        with ThreadPoolExecutor(threads) as pool:
            blobs = list(pool.map(one, range(len(host))))
    return avi.write_avi(path, blobs, rate, 1, pcm)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t, out


def spread(n, ts):
    return {"median": round(n / statistics.median(ts), 1), "min": round(n / max(ts), 1), "max": round(n / min(ts), 1)}


def kernel_alone(eng, frames, items, masks, copy_tbs):
    """avcer_annotate_frames on one pass of 64 frames, device events around the call (the upload of items and plan included)."""
    dev = eng.device
    k = min(64, int(frames.shape[0]))
    sel = items[items["frame"] < k]
    flat, table = an.pack_masks(masks)
    flat_d = torch.from_numpy(flat).to(dev)
    buf = frames[:k].clone()
    shape = (k,) + tuple(int(v) for v in frames.shape[1:])
    work, tiles = an.work_table(sel, table, k, int(frames.shape[1]), int(frames.shape[2]))
    for _ in range(3):
        eng.annotate(buf, sel, flat_d, table)
    ms = []
    for _ in range(20):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        eng.annotate(buf, sel, flat_d, table)
        ev[1].record()
        torch.cuda.synchronize(dev)
        ms.append(ev[0].elapsed_time(ev[1]))
    t = statistics.median(ms) * 1e-3
    # pixels some item covers: count them with a drawing whose every item is opaque white on black frames
    probe = sel.copy()
    probe["colour"] = 255
    cov = an.draw_numpy(np.zeros(shape, dtype=np.uint8), probe, [np.where(m > 0, 255, 0).astype(np.uint8) for m in masks])
    covered = int((cov > 0).any(axis=3).sum())
    moved = covered * 6  # 3 bytes read and 3 written per covered pixel; items and masks come from cache
    return {"frames": k, "items": int(len(sel)), "tiles_of_64x4_launched": int(tiles), "ms_median": round(t * 1e3, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "covered_pixels": covered, "bytes_touched": moved, "batch_bytes": int(buf.numel()),
            "share_of_batch_touched": round(moved / 2 / buf.numel(), 5), "touched_tb_per_s": round(moved / t / 1e12, 5),
            "measured_hbm_copy_tb_per_s": copy_tbs,
            "note": "host clock inside the events: item check, plan and one upload per call; the kernel touches covered pixels only, so "
                    "its rate against the copy ceiling says how little there is to move, not how well it is moved"}


def option_cost(eng, tmp, reps):
    """run_inference_file on a 640 x 360 clip of 125 frames with and without path_save_video, interleaved."""
    from PIL import Image

    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    w, h, n = 640, 360, 125
    blobs = []
    for img in pictures(w, h, DISTINCT, seed=3):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    pcm = (np.random.default_rng(1).normal(0, 3000, (44100 * n // 25, 2))).astype(np.int16)
    path = avi.write_avi(os.path.join(tmp, "in.avi"), [blobs[i % DISTINCT] for i in range(n)], 25, pcm=pcm)
    records, _, _ = scene(w, h, n)
    dets = [np.array([list(r[2:6]) + [0.99] + [0] * 10], dtype=np.float32) for r in records[records[:, 1] == 0]]
    out = os.path.join(tmp, "out.avi")
    plain = lambda: arun.run_inference_file(eng, path, detections=dets)
    video = lambda: arun.run_inference_file(eng, path, detections=dets, path_save_video=out)
    plain(), video()
    tp, tv = [], []
    for _ in range(reps):
        tp.append(timed(plain, eng.device)[0])
        tv.append(timed(video, eng.device)[0])
    os.remove(path), os.remove(out)
    return {"clip": f"{w}x{h}, {n} frames, 5 s of 44.1 kHz stereo", "seconds_without": round(statistics.median(tp), 4),
            "seconds_with_path_save_video": round(statistics.median(tv), 4), "seconds_added_median": round(statistics.median(tv) - statistics.median(tp), 4),
            "seconds_without_min_max": [round(min(tp), 4), round(max(tp), 4)], "seconds_with_min_max": [round(min(tv), 4), round(max(tv), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "result_video_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    _, copy_tbs = eng.measure_ceilings()
    res = {"what": "frames on the device -> drawn result video (Motion-JPEG AVI) on disk: frames/s, median of the repetitions (min, max)",
           "reps": a.reps, "frames_per_pass": 64, "quality": 90, "subsampling": "4:2:0", "measured_hbm_copy_tb_per_s": copy_tbs,
           "drawing": "annotate.layout: a box per record, a label on track 00 (backdrop, name mask, number mask)", "sizes": {}}
    tmp = tempfile.mkdtemp()
    for w, h, n in SIZES:
        n = max(8, int(n * a.scale))
        pics = pictures(w, h, DISTINCT, seed=w)
        frames = torch.from_numpy(np.stack([pics[i % DISTINCT][..., ::-1] for i in range(n)]).copy()).to(dev)
        records, pred, prob = scene(w, h, n)
        items, masks = an.layout(records, pred, prob, h, w)
        pcm = np.zeros((44100 * n // 25, 2), dtype=np.int16)
        paths = {k: os.path.join(tmp, f"{k}_{w}.avi") for k in ("pil_1_thread", "pil_16_threads", "device_entropy_host", "device_entropy_device")}
        arms = {
            "pil_1_thread": lambda: pil_arm(frames, items, masks, paths["pil_1_thread"], 25, pcm, 1),
            "pil_16_threads": lambda: pil_arm(frames, items, masks, paths["pil_16_threads"], 25, pcm, 16),
            "device_entropy_host": lambda: an.write_result_video(eng, frames, records, pred, prob, paths["device_entropy_host"], 25, pcm=pcm,
                                                                 entropy="host"),
            "device_entropy_device": lambda: an.write_result_video(eng, frames, records, pred, prob, paths["device_entropy_device"], 25, pcm=pcm,
                                                                   entropy="device"),
        }
        for fn in arms.values():  # warm-up of every arm at this shape
            fn()
        torch.cuda.synchronize(dev)
        files = {k: open(p, "rb").read() for k, p in paths.items()}
        assert all(v == files["pil_1_thread"] for v in files.values()), "the arms wrote different files"
        size = len(files["pil_1_thread"])
        del files
        times = {k: [] for k in arms}
        for _ in range(a.reps):  # interleaved: what else runs on the host hits every arm alike
            for k, fn in arms.items():
                times[k].append(timed(fn, dev)[0])
        entry = {"frames": n, "file_bytes": size, "items": int(len(items)), "arms_wrote_identical_files": True,
                 "frames_per_s": {k: spread(n, ts) for k, ts in times.items()},
                 "avcer_annotate_frames_pass_of_64": kernel_alone(eng, frames, items, masks, copy_tbs)}
        res["sizes"][f"{w}x{h}"] = entry
        for p in paths.values():
            os.remove(p)
        del frames
    res["run_inference_file_option"] = option_cost(eng, tmp, a.reps)
    os.rmdir(tmp)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
