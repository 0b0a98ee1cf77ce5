"""Cost of writing JPEG face crops: PIL's encoder, one core and a 16-thread pool, against jpeg.encode_images (HIP forward pass +
host Huffman pass at 1 / 4 / 16 threads, and with entropy="device": the Huffman pass on the device too, 1 host thread;
avcer_amd/jpeg.py), on one machine, in one process, arms alternating within every repeat.  Input: --files
synthetic 200 x 200 crops with the content of tools/jpeg_bench.py, quality 95, 4:2:0; every arm encodes to memory (no file is
written).  Writes profiles/jpeg_entropy_bench.json (profiles/jpeg_encode_bench.json is the run from before the device coder).
`python tools/jpeg_encode_bench.py [--files 2048] [--repeats 5] [--out profiles/jpeg_entropy_bench.json]`."""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import jpeg  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402

THREADS = (1, 4, 16)


def make_crops(n: int) -> np.ndarray:
    """tools/jpeg_bench.py write_crops, kept in memory: smooth content plus noise (file sizes of photographs)."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:200, 0:200]
    out = np.empty((n, 200, 200, 3), dtype=np.uint8)
    for i in range(n):
        ph = rng.uniform(0, 6.28, 6)
        a = np.stack([np.sin(xx / (23.0 + 5 * c) + ph[c]) * 60 + np.cos(yy / (31.0 - 4 * c) + ph[3 + c]) * 50 + 128 for c in range(3)], axis=2)
        out[i] = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
    return out


def pil_one(img) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=95)  # the call of heatmaps.write_heatmaps
    return b.getvalue()


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stages(eng, src, rects, threads: int) -> dict:
    """The device arm taken apart: plan and descriptor copy, the kernel and the copy of the coefficients to the host (device
    events), the host pass (host clock)."""
    n = len(rects)
    desc, blocks = jpeg.plan(eng.lib, [(200, 200)] * n, 95, 2)
    d_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(eng.device)
    r_dev = torch.from_numpy(rects).to(eng.device)
    host = torch.empty(64 * blocks, dtype=torch.int16, pin_memory=True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    torch.cuda.synchronize()
    ev[0].record()
    coeffs = eng.jpeg_forward(src, r_dev, d_dev, n, blocks)
    ev[1].record()
    host.copy_(coeffs, non_blocking=True)
    ev[2].record()
    torch.cuda.synchronize()
    out = np.empty(jpeg.HEADER_BYTES * n + 64 * blocks, dtype=np.uint8)
    t0 = time.perf_counter()
    offsets, need = jpeg.write_batch(eng.lib, host.numpy(), desc, out, threads, eng.ctx)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert (desc["status"] == jpeg.OK).all()
    return {"kernel_ms": ev[0].elapsed_time(ev[1]), "d2h_ms": ev[1].elapsed_time(ev[2]), "host_huffman_ms": host_ms,
            "coefficient_bytes": 128 * blocks, "file_bytes": int(need)}


def pack_stages(eng, src, rects) -> dict:
    """The device-entropy arm taken apart (device events): the forward kernel, avcer_jpeg_pack alone, the copy of the files to the
    host; and what crosses to the host: offsets, statuses and the files."""
    n = len(rects)
    desc, blocks = jpeg.plan(eng.lib, [(200, 200)] * n, 95, 2)
    d_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(eng.device)
    r_dev = torch.from_numpy(rects).to(eng.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    ev[0].record()
    coeffs = eng.jpeg_forward(src, r_dev, d_dev, n, blocks)
    ev[1].record()
    out, offsets, status, need = eng.jpeg_pack(coeffs, d_dev, n, blocks, jpeg.HEADER_BYTES * n + 40 * blocks)
    ev[2].record()
    torch.cuda.synchronize()
    pack_ms = ev[1].elapsed_time(ev[2])
    total = int(offsets[-1])  # waits, as encode_images does
    assert not status.any().item() and total == int(need)
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    ev[2].record()
    host.copy_(out[:total], non_blocking=True)
    ev[3].record()
    torch.cuda.synchronize()
    return {"kernel_ms": ev[0].elapsed_time(ev[1]), "pack_ms": pack_ms, "d2h_ms": ev[2].elapsed_time(ev[3]),
            "host_bytes": total + 8 * (n + 2) + 4 * n}


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_entropy_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    crops = make_crops(a.files)
    src = torch.from_numpy(crops).to(eng.device)
    rects = np.array([(i, 0, 0, 200, 200) for i in range(a.files)], dtype=np.int32)
    res = {"files": a.files, "size": "200x200, quality 95, 4:2:0", "repeats": a.repeats, "threads_swept": list(THREADS),
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "output": "bytes in memory, no file written"}
    pool = ThreadPoolExecutor(16)
    # same bytes first
    ref = [pil_one(c) for c in crops]
    res["bytes_identical"] = bool(jpeg.encode_images(eng, src, rects) == ref and list(pool.map(pil_one, crops)) == ref and
                                  jpeg.encode_images(eng, src, rects, entropy="device") == ref)
    assert res["bytes_identical"]
    res["mean_file_bytes"] = sum(len(b) for b in ref) / a.files
    t = {"pil_loop": [], "pil_pool16": [], **{f"device_{k}": [] for k in THREADS}, "device_entropy_1": []}
    parts = {k: [] for k in THREADS}
    pack_parts = []
    for k in THREADS:  # warm-up of every arm
        jpeg.encode_images(eng, src, rects, threads=k)
        stages(eng, src, rects, k)
    jpeg.encode_images(eng, src, rects, threads=1, entropy="device")
    pack_stages(eng, src, rects)
    for _ in range(a.repeats):
        t["pil_loop"].append(wall(lambda: [pil_one(c) for c in crops]))
        t["pil_pool16"].append(wall(lambda: list(pool.map(pil_one, crops))))
        for k in THREADS:
            t[f"device_{k}"].append(wall(lambda: jpeg.encode_images(eng, src, rects, threads=k)))
            parts[k].append(stages(eng, src, rects, k))
        t["device_entropy_1"].append(wall(lambda: jpeg.encode_images(eng, src, rects, threads=1, entropy="device")))
        pack_parts.append(pack_stages(eng, src, rects))
    pool.shutdown()
    res["encode_ms"] = {k: {"median": med(v), "min": min(v), "max": max(v)} for k, v in t.items()}
    res["files_per_s"] = {k: a.files / (med(v) / 1e3) for k, v in t.items()}
    res["device_arm_parts_ms"] = {str(k): {f: med([p[f] for p in parts[k]]) for f in ("kernel_ms", "d2h_ms", "host_huffman_ms")} for k in THREADS}
    res["device_entropy_parts_ms"] = {f: med([p[f] for p in pack_parts]) for f in ("kernel_ms", "pack_ms", "d2h_ms")}
    res["host_bytes_per_file"] = {"host_entropy": parts[THREADS[0]][0]["coefficient_bytes"] / a.files,
                                  "device_entropy": pack_parts[0]["host_bytes"] / a.files}
    p0 = parts[THREADS[-1]][0]
    res["coefficient_bytes"], res["pixel_bytes"], res["file_bytes"] = p0["coefficient_bytes"], int(crops.size), p0["file_bytes"]
    res["d2h_gb_per_s"] = p0["coefficient_bytes"] / (med([p["d2h_ms"] for p in parts[THREADS[-1]]]) * 1e-3) / 1e9
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
