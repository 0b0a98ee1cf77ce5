"""Frames of a Motion-JPEG AVI file onto the device, three ways, in one run -> profiles/avi_decode_bench.json.

The tool synthesises a clip (avi.write_avi of PIL-written frames: quality 90, 4:2:0, the standard Huffman tables), opens it with
avi.open_avi and times, interleaved and repeated:
  (a) a PIL decode loop into pinned memory, on one thread and on 16, followed by the host-to-device copy of the frames;
  (b) jpeg.decode_frames with entropy="host"   (Huffman decode on 16 host threads, pixels on the device);
  (c) jpeg.decode_frames with entropy="device" (headers on the host, everything else on the device);
at 640 x 360 (750 frames) and 1920 x 1080 (256 frames).  Every arm ends in a device synchronise and is timed with the host clock
around it (the arms are host loops that end in device work); avcer_jpeg_frames alone is timed with device events.  Reported per
arm: frames/s of the median repetition and the spread (min, max).  No ratio is fixed in advance: the file records what was seen.
It also records the write bandwidth avcer_jpeg_frames achieved on a pass of 64 frames beside the copy figure of
Engine.measure_ceilings, and checks once that the three arms give the same frames."""
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

from avcer_amd import avi, jpeg  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402

SIZES = ((640, 360, 750), (1920, 1080, 256))  # width, height, frames
DISTINCT = 16                                  # distinct pictures the clip cycles through (the encode is not what is measured)


def pictures(w, h, count, seed=0):
    """Photograph-like pictures: smooth colour fields, a few edges, sensor noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for k in range(count):
        f = rng.uniform(0.004, 0.03, (3, 2))
        ph = rng.uniform(0, 6.28, 3)
        img = np.stack([127 + 90 * np.sin(f[c, 0] * x + f[c, 1] * y + ph[c]) for c in range(3)], axis=-1)
        for _ in range(6):  # rectangles: hard edges
            x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
            img[y0:y0 + int(rng.integers(8, h // 2)), x0:x0 + int(rng.integers(8, w // 2))] += rng.uniform(-60, 60, 3)
        img += rng.normal(0, 3.0, img.shape)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def synthesise(path, w, h, n):
    from PIL import Image

    blobs = []
    for img in pictures(w, h, DISTINCT, seed=w):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    pcm = np.zeros((44100 * n // 25, 2), dtype=np.int16)
    avi.write_avi(path, [blobs[i % DISTINCT] for i in range(n)], 25, pcm=pcm)
    return sum(len(blobs[i % DISTINCT]) for i in range(n)) / n


def pil_arm(frames, host, dev, threads):
    from PIL import Image

    view = host.numpy()

    def one(i):
        with Image.open(io.BytesIO(frames[i])) as img:
            np.copyto(view[i], np.asarray(img.convert("RGB")))

    if threads == 1:
        for i in range(len(frames)):
            one(i)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(one, range(len(frames))))
    return host.to(dev, non_blocking=True)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avi_decode_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    _, copy_tbs = eng.measure_ceilings()
    res = {"what": "frames of a Motion-JPEG AVI file onto the device: frames/s, median of the repetitions (min, max)",
           "reps": a.reps, "host_threads": jpeg.host_threads(0), "frames_per_pass": 64, "measured_hbm_copy_tb_per_s": copy_tbs,
           "clip": "PIL-written frames, quality 90, 4:2:0, standard Huffman tables, %d distinct pictures cycled" % DISTINCT, "sizes": {}}
    tmp = tempfile.mkdtemp()
    for w, h, n in SIZES:
        n = max(8, int(n * a.scale))
        path = os.path.join(tmp, f"clip_{w}x{h}.avi")
        mean_bytes = synthesise(path, w, h, n)
        with avi.open_avi(path) as clip:
            assert (clip.width, clip.height, clip.n_frames) == (w, h, n)
            host = torch.empty(n, h, w, 3, dtype=torch.uint8, pin_memory=True)
            arms = {
                "pil_1_thread_plus_copy": lambda: pil_arm(clip.frames, host, dev, 1),
                "pil_16_threads_plus_copy": lambda: pil_arm(clip.frames, host, dev, 16),
                "decode_frames_entropy_host": lambda: jpeg.decode_frames(eng, clip.frames, h, w, bgr=False, entropy="host")[0],
                "decode_frames_entropy_device": lambda: jpeg.decode_frames(eng, clip.frames, h, w, bgr=False, entropy="device")[0],
            }
            # warm-up of every arm at this shape, and the one check that they agree
            outs = {k: fn() for k, fn in arms.items()}
            torch.cuda.synchronize(dev)
            same = all(torch.equal(outs["pil_1_thread_plus_copy"], v) for v in outs.values())
            del outs
            times = {k: [] for k in arms}
            for _ in range(a.reps):  # interleaved: what else runs on the host hits every arm alike
                for k, fn in arms.items():
                    times[k].append(timed(fn, dev)[0])
            entry = {"frames": n, "mean_frame_bytes": round(mean_bytes), "arms_agree_bit_for_bit": bool(same), "frames_per_s": {}}
            for k, ts in times.items():
                entry["frames_per_s"][k] = {"median": round(n / statistics.median(ts), 1), "min": round(n / max(ts), 1),
                                            "max": round(n / min(ts), 1)}
            # avcer_jpeg_frames alone, on one pass of 64 frames: device events around the call (inverse DCT, size check, pixels)
            part = clip.frames[:min(64, n)]
            c_dev, d_dev, used, _ = jpeg._to_device(eng, part, 0)
            out = torch.empty(len(part), h, w, 3, dtype=torch.uint8, device=dev)
            for _ in range(3):
                eng.jpeg_frames(c_dev, d_dev, len(part), used, h, w, bgr=True, out=out)
            ms = []
            for _ in range(20):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                eng.jpeg_frames(c_dev, d_dev, len(part), used, h, w, bgr=True, out=out)
                ev[1].record()
                torch.cuda.synchronize(dev)
                ms.append(ev[0].elapsed_time(ev[1]))
            t = statistics.median(ms) * 1e-3
            wrote = out.numel()
            moved = wrote + used * (128 + 64 + 64)  # + coefficients read, planes written and read once (chroma rows are re-read from cache)
            entry["avcer_jpeg_frames_pass_of_64"] = {
                "ms_median": round(t * 1e3, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "frame_bytes_written": wrote, "write_tb_per_s": round(wrote / t / 1e12, 4),
                "bytes_moved_at_least": moved, "traffic_tb_per_s": round(moved / t / 1e12, 4),
                "share_of_measured_copy_ceiling": round(moved / t / 1e12 / copy_tbs, 4) if copy_tbs else None,
                "note": "the call's three kernels together (inverse DCT into planes, size check, pixels); the ceiling is a copy's read + write rate"}
            res["sizes"][f"{w}x{h}"] = entry
            del host, out, c_dev, d_dev
        os.remove(path)
    os.rmdir(tmp)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
