"""Cost of reading a folder of JPEG face crops: the PIL loop of video_pipeline.read_face_dir against read_face_dir_device (host
entropy pass + HIP pixel pass, avcer_amd/jpeg.py), on one machine, in one process, arms alternating within every repeat.
Input: --files synthetic 200 x 200 crops, quality 95, 4:2:0, smooth content plus noise (file sizes of photographs).  Writes
profiles/jpeg_decode_bench.json.  `python tools/jpeg_bench.py [--files 2048] [--frames 750] [--repeats 5]`.
Then (or alone, with --unpack) the same folder read with entropy="device" (avcer_jpeg_unpack: Huffman decoding on the device)
against entropy="host", at 1 and 16 host threads, same crops, same process, arms alternating within every repeat, and the
device-entropy arm taken apart; writes profiles/jpeg_unpack_bench.json with the subsequence length used."""
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

from avcer_amd import jpeg, synth, video_pipeline  # noqa: E402
from avcer_amd.engine import MODE_F16X3, Engine  # noqa: E402

THREADS = (1, 4, 16)


def write_crops(folder: str, n: int) -> float:
    from PIL import Image

    os.makedirs(folder)
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:200, 0:200]
    total = 0
    for i in range(n):
        ph = rng.uniform(0, 6.28, 6)
        a = np.stack([np.sin(xx / (23.0 + 5 * c) + ph[c]) * 60 + np.cos(yy / (31.0 - 4 * c) + ph[3 + c]) * 50 + 128 for c in range(3)], axis=2)
        a = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
        path = os.path.join(folder, f"{i:06d}.jpg")
        Image.fromarray(a).save(path, "JPEG", quality=95, subsampling=2)
        total += os.path.getsize(path)
    return total / n


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stages(eng, blobs, threads: int) -> dict:
    """The device arm taken apart: host entropy pass (host clock), the two copies and the two kernels (device events)."""
    st = eng.__dict__.setdefault("_jpeg_staging", jpeg._Staging())
    n = len(blobs)
    st.reserve(sum(len(b) for b in blobs) // 8, n)
    desc = st.desc.numpy()[:jpeg.DESC.itemsize * n].view(jpeg.DESC)
    t0 = time.perf_counter()
    jpeg.entropy_batch(eng.lib, blobs, st.coeffs.numpy(), desc, threads, eng.ctx)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert (desc["status"] == jpeg.OK).all()
    used = int((desc["coef_block"] + desc["n_blocks"]).max())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tiles = torch.empty(n, 224, 224, 3, dtype=torch.uint8, device=eng.device)
    torch.cuda.synchronize()
    ev[0].record()
    c = st.coeffs[:64 * used].to(eng.device, non_blocking=True)
    d = st.desc[:jpeg.DESC.itemsize * n].to(eng.device, non_blocking=True)
    ev[1].record()
    _, flags = eng.jpeg_tiles(c, d, n, used, out=tiles)
    ev[2].record()
    torch.cuda.synchronize()
    assert not flags.any().item()
    return {"host_entropy_ms": host_ms, "h2d_ms": ev[0].elapsed_time(ev[1]), "kernels_ms": ev[1].elapsed_time(ev[2]),
            "coefficient_bytes": 128 * used, "blocks": used}


def med(xs):
    return statistics.median(xs)


UNPACK_THREADS = (1, 16)
DEFAULT_SUB_BITS = 512  # csrc/jpeg_sync_dev.h DEFAULT_SUB_BITS


def unpack_stages(eng, blobs, threads: int) -> dict:
    """The entropy="device" arm taken apart: scan_batch (host clock), the one copy, avcer_jpeg_unpack, the pixel kernels (device
    events)."""
    n = len(blobs)
    st = eng.__dict__.setdefault("_jpeg_staging", jpeg._Staging())
    cap_bytes, cap_tabs = sum(len(b) for b in blobs) + 16 * n, jpeg.TABS_ROOM
    at_scan = jpeg.DESC.itemsize * n
    at_tabs = at_scan + jpeg.SCAN.itemsize * n
    at_data = at_tabs + jpeg.TAB.itemsize * cap_tabs
    wire = st.reserve_wire(at_data + cap_bytes).numpy()
    desc, scan = wire[:at_scan].view(jpeg.DESC), wire[at_scan:at_tabs].view(jpeg.SCAN)
    t0 = time.perf_counter()
    n_tabs, need_bytes, need_blocks = jpeg.scan_batch(eng.lib, blobs, wire[at_data:at_data + cap_bytes], desc, scan,
                                                      wire[at_tabs:at_data].view(jpeg.TAB), threads, eng.ctx)
    scan_ms = (time.perf_counter() - t0) * 1e3
    assert (desc["status"] == jpeg.OK).all()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    tiles = torch.empty(n, 224, 224, 3, dtype=torch.uint8, device=eng.device)
    torch.cuda.synchronize()
    ev[0].record()
    w = st.wire[:at_data + need_bytes].to(eng.device, non_blocking=True)
    ev[1].record()
    c, status = eng.jpeg_unpack(w[at_data:], w[at_scan:at_tabs], w[at_tabs:at_data], n_tabs, w[:at_scan], n, need_blocks)
    ev[2].record()
    _, flags = eng.jpeg_tiles(c, w[:at_scan], n, need_blocks, out=tiles)
    ev[3].record()
    torch.cuda.synchronize()
    assert not flags.any().item() and not status.any().item()
    return {"scan_batch_ms": scan_ms, "h2d_ms": ev[0].elapsed_time(ev[1]), "unpack_ms": ev[1].elapsed_time(ev[2]),
            "pixel_kernels_ms": ev[2].elapsed_time(ev[3]), "wire_bytes": at_data + need_bytes, "coefficient_bytes": 128 * need_blocks}


def unpack_bench(eng, path: str, blobs, files: int, repeats: int) -> dict:
    res = {"files": files, "size": "200x200, quality 95, 4:2:0", "repeats": repeats, "threads_swept": list(UNPACK_THREADS),
           "sub_bits_default": DEFAULT_SUB_BITS, "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "mean_file_bytes": sum(len(b) for b in blobs) / len(blobs)}
    a, _ = video_pipeline.read_face_dir_device(eng, path, files)
    b, _ = video_pipeline.read_face_dir_device(eng, path, files, entropy="device")
    res["tiles_bit_identical"] = bool(torch.equal(a, b))
    arms = [(e, k) for k in UNPACK_THREADS for e in ("host", "device")]
    t = {f"{e}_{k}": [] for e, k in arms}
    parts = {k: [] for k in UNPACK_THREADS}
    for e, k in arms:  # warm-up of every arm
        video_pipeline.read_face_dir_device(eng, path, files, threads=k, entropy=e)
    for k in UNPACK_THREADS:
        unpack_stages(eng, blobs, k)
    for _ in range(repeats):
        for e, k in arms:
            t[f"{e}_{k}"].append(wall(lambda: video_pipeline.read_face_dir_device(eng, path, files, threads=k, entropy=e)))
        for k in UNPACK_THREADS:
            parts[k].append(unpack_stages(eng, blobs, k))
    res["read_face_dir_ms"] = {k: {"median": med(v), "min": min(v), "max": max(v)} for k, v in t.items()}
    res["files_per_s"] = {k: files / (med(v) / 1e3) for k, v in t.items()}
    names = ("scan_batch_ms", "h2d_ms", "unpack_ms", "pixel_kernels_ms")
    res["device_entropy_parts_ms"] = {str(k): {f: med([p[f] for p in parts[k]]) for f in names} for k in UNPACK_THREADS}
    res["device_entropy_parts_share"] = {str(k): {f: res["device_entropy_parts_ms"][str(k)][f] / sum(res["device_entropy_parts_ms"][str(k)].values())
                                                  for f in names} for k in UNPACK_THREADS}
    res["bytes_over_pcie_per_file"] = {"device": parts[1][0]["wire_bytes"] / files,
                                       "host": (parts[1][0]["coefficient_bytes"] + jpeg.DESC.itemsize * files) / files}
    res["unpack_files_per_s"] = files / (res["device_entropy_parts_ms"]["16"]["unpack_ms"] / 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=750)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--unpack", action="store_true", help="only the entropy=\"device\" comparison (profiles/jpeg_unpack_bench.json)")
    a = ap.parse_args()
    if a.unpack:
        eng = Engine(0)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "clip")
            write_crops(os.path.join(path, "00"), a.files)
            blobs = [video_pipeline._read_blob(os.path.join(path, "00", f"{i:06d}.jpg")) for i in range(a.files)]
            res = unpack_bench(eng, path, blobs, a.files, a.repeats)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "jpeg_unpack_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res, indent=1))
        return
    eng = Engine(0)
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    res = {"files": a.files, "size": "200x200, quality 95, 4:2:0", "repeats": a.repeats, "threads_swept": list(THREADS),
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clip")
        res["mean_file_bytes"] = write_crops(os.path.join(path, "00"), a.files)
        blobs = [video_pipeline._read_blob(os.path.join(path, "00", f"{i:06d}.jpg")) for i in range(a.files)]
        # same bits first
        ref, _ = video_pipeline.read_face_dir(path, a.files)
        got, _ = video_pipeline.read_face_dir_device(eng, path, a.files)
        res["tiles_bit_identical"] = bool((got.cpu().numpy() == ref).all())
        t = {"pil": [], **{f"device_{k}": [] for k in THREADS}}
        parts = {k: [] for k in THREADS}
        for k in THREADS:  # warm-up of every arm
            video_pipeline.read_face_dir_device(eng, path, a.files, threads=k)
            stages(eng, blobs, k)
        for _ in range(a.repeats):
            t["pil"].append(wall(lambda: video_pipeline.read_face_dir(path, a.files)))
            for k in THREADS:
                t[f"device_{k}"].append(wall(lambda: video_pipeline.read_face_dir_device(eng, path, a.files, threads=k)))
                parts[k].append(stages(eng, blobs, k))
        res["read_face_dir_ms"] = {k: {"median": med(v), "min": min(v), "max": max(v)} for k, v in t.items()}
        res["files_per_s"] = {k: a.files / (med(v) / 1e3) for k, v in t.items()}
        res["device_arm_parts_ms"] = {str(k): {f: med([p[f] for p in parts[k]]) for f in ("host_entropy_ms", "h2d_ms", "kernels_ms")}
                                      for k in THREADS}
        p0 = parts[THREADS[-1]][0]
        # kernel A reads the coefficients and writes one byte per coefficient; kernel B reads at most those planes and writes the tiles
        moved = p0["coefficient_bytes"] + 2 * 64 * p0["blocks"] + a.files * 224 * 224 * 3
        _, hbm_tbs = eng.measure_ceilings()
        k_ms = med([p["kernels_ms"] for p in parts[THREADS[-1]]])
        res["kernels"] = {"bytes_moved_upper_bound": moved, "ms": k_ms, "achieved_tb_per_s": moved / (k_ms * 1e-3) / 1e12,
                          "hbm_copy_ceiling_tb_per_s": hbm_tbs, "share_of_ceiling": moved / (k_ms * 1e-3) / 1e12 / hbm_tbs}
        res["h2d_gb_per_s"] = p0["coefficient_bytes"] / (med([p["h2d_ms"] for p in parts[THREADS[-1]]]) * 1e-3) / 1e9
        # end to end: one video of --frames frames
        e2e = {"pil": [], "device": []}
        for decode in e2e:
            video_pipeline.preprocess_video_and_predict(eng, path, tmp, 25, a.frames, mode=MODE_F16X3, decode=decode)
        frames, present = video_pipeline.read_face_dir_device(eng, path, a.frames)
        models = []
        for _ in range(a.repeats):
            for decode in e2e:
                e2e[decode].append(wall(lambda: video_pipeline.preprocess_video_and_predict(eng, path, tmp, 25, a.frames, mode=MODE_F16X3,
                                                                                           decode=decode)))
            models.append(wall(lambda: [x.cpu() for x in video_pipeline.visual_forward(eng, frames, present, 25, MODE_F16X3)]))
        res["end_to_end"] = {"frames": a.frames, "fps": 25, "models_ms": med(models),
                             **{f"{k}_ms": med(v) for k, v in e2e.items()},
                             **{f"{k}_share_outside_models": 1.0 - med(models) / med(v) for k, v in e2e.items()}}
        unpack = unpack_bench(eng, path, blobs, a.files, a.repeats)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(ROOT, "profiles", "jpeg_unpack_bench.json"), "w") as f:
        json.dump(unpack, f, indent=1)
    print(json.dumps(res, indent=1))
    print(json.dumps(unpack, indent=1))


if __name__ == "__main__":
    main()
