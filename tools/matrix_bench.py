"""Cost of the matrix figures (avcer_amd/figures.py: host-built item lists, avcer_annotate_frames, the JPEG encoder).  Writes
profiles/matrix_bench.json.  `python tools/matrix_bench.py [--reps 5] [--figures 1,24]`.

Convention: `--reps` interleaved repetitions per comparison, median (min..max); every arm asserts identical file bytes before it is
timed.

(a) matrices on the host to file bytes, for V in `--figures` figures of 800 x 600, 7 x 7 "conf" and 3 x 7 "weights":
      cpu      figures.matrix_numpy + PIL Image.save(quality=95, subsampling=2) on one thread;
      device   figures.batch_items + render + jpeg.encode_images(entropy="device"): the plans are made once outside the timing in
               BOTH arms (they hold the labels' and the title's masks), everything that depends on the values is inside.
(b) the annotate.draw call alone (device events around avcer_annotate_frames and the upload of its items and launch plan), with
    the item count per figure: a thread walks ALL items of its frame in order, so this is the number that could argue for a
    dedicated paint kernel; beside it the host's share, figures.batch_items alone (wall clock)."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import annotate as an  # noqa: E402
from avcer_amd import evaluate, figures, jpeg  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402


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


def matrices(kind, V):
    """V matrices as a scored dataset gives them: counts of some thousand frames with a strong diagonal / Dirichlet weights."""
    rng = np.random.default_rng(V)
    if kind == "conf":
        return [rng.integers(0, 4000, (7, 7)).astype(np.int64) + np.diag(rng.integers(5000, 40000, 7)) for _ in range(V)]
    return [rng.dirichlet(np.ones(3), 7).T.copy() for _ in range(V)]


def plans_for(kind, V):
    if kind == "conf":
        return [figures.matrix_plan(7, 7, "conf", labels=evaluate.EMO, title=f"Audio-Video fusion. ABAW. UAR = {40 + v}.25%") for v in range(V)]
    labels = (["VS", "VD", "A"], ["Ne", "An", "Di", "Fe", "Ha", "Sa", "Su"])
    return [figures.matrix_plan(3, 7, "weights", labels=labels, title=f"Weights for audio and video modality fusion {v}") for v in range(V)]


def bench(eng, a, res):
    from PIL import Image

    res["figures"] = {}
    for kind in ("conf", "weights"):
        for V in a.figures:
            values, plans = matrices(kind, V), plans_for(kind, V)
            rects = np.zeros((V, 5), dtype=np.int32)
            rects[:, 0], rects[:, 3], rects[:, 4] = np.arange(V), 800, 600

            def cpu():
                files = []
                for v, p in zip(values, plans):
                    b = io.BytesIO()
                    Image.fromarray(figures.matrix_numpy(v, p)).save(b, "JPEG", quality=95, subsampling=2)
                    files.append(b.getvalue())
                return files

            def device():
                return jpeg.encode_images(eng, figures.render(eng, values, plans), rects, quality=95, subsampling=2, entropy="device")

            items, masks = figures.batch_items(values, plans)
            flat, table = an.pack_masks(masks)
            flat_d = torch.from_numpy(flat).to(eng.device)
            canvas = torch.full((V, 600, 800, 3), 255, dtype=torch.uint8, device=eng.device)

            def draw():
                return an.draw(eng, canvas, items, (flat_d, table))

            want = cpu()
            assert [bytes(f) for f in device()] == want, (kind, V)  # identical bytes before any timing
            draw()
            ts = {"cpu": [], "device": [], "draw": [], "items": []}
            for _ in range(a.reps):
                ts["cpu"].append(wall_ms(cpu)[0])
                ts["device"].append(wall_ms(device)[0])
                ts["draw"].append(event_ms(draw)[0])
                ts["items"].append(wall_ms(lambda: figures.batch_items(values, plans))[0])
            row = {"cpu_matrix_numpy_pil_save_1_thread": stats(ts["cpu"]), "device_matrices_to_file_bytes": stats(ts["device"]),
                   "annotate_draw_alone_device_events": stats(ts["draw"]), "host_batch_items_alone": stats(ts["items"]),
                   "items_per_figure": len(items) / V, "masks_in_the_shared_buffer": len(masks), "mask_bytes": int(len(flat))}
            row["cpu_over_device"] = row["cpu_matrix_numpy_pil_save_1_thread"]["median_ms"] / row["device_matrices_to_file_bytes"]["median_ms"]
            res["figures"][f"{kind} V={V}"] = row
            del canvas, flat_d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--figures", type=lambda s: [int(v) for v in s.split(",")], default=[1, 24])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    res = {"reps": a.reps, "picture": "800 x 600", "convention": "interleaved repetitions, median (min..max), every arm asserts identical file "
           "bytes before it is timed; matrices on the host to file bytes on the host"}
    bench(eng, a, res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
