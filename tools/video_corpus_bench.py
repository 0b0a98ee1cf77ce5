"""A corpus of face folders: a loop of `preprocess_video_and_predict(decode="device")` against one `run_video_corpus` call, on one GPU
with synthetic weights.

    python tools/video_corpus_bench.py [--folders 64] [--reps 5] [--out profiles/video_corpus_bench.json]

64 folders of 1 to 12 s at 25 and 30 frames per second, long and short interleaved, every frame with a crop; one crop size per folder,
60 to 200 px a side, quality 95, 4:2:0, smooth content plus noise (file sizes of photographs), written to a temporary directory
with PIL.  Arms: run_video_corpus with entropy "host" and "device", and the per-folder loop.  The packed arms end with ONE copy of all
tables to the host, since the per-folder call returns host arrays.  Every arm is first held to the loop's tables, bit for bit (that
run is its warm-up), then the arms are timed interleaved, `reps` times each, wall clock around a device synchronisation: median
(min..max) ms.  Also recorded: the library's GEMM-family launches per folder in both arms, the pass sizes, and the packed call taken
apart, each part run on its own -- reading the files, reading + decoding them into the tile buffer, the models on resident tiles."""
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

from avcer_amd import build, jpeg, synth  # noqa: E402
from avcer_amd import video_corpus as vc  # noqa: E402
from avcer_amd.engine import MODE_DEFAULT, Engine  # noqa: E402
from avcer_amd.video_pipeline import _DevicePlan, _tables, preprocess_video_and_predict  # noqa: E402


def write_corpus(root: str, n_folders: int):
    from PIL import Image

    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:200, 0:200]
    pool = []
    for _ in range(48):
        ph = rng.uniform(0, 6.28, 6)
        a = np.stack([np.sin(xx / (23.0 + 5 * c) + ph[c]) * 60 + np.cos(yy / (31.0 - 4 * c) + ph[3 + c]) * 50 + 128 for c in range(3)], axis=2)
        pool.append(np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8))
    seconds = [1 + (11 * k) // max(n_folders - 1, 1) for k in range(n_folders)]
    seconds = [seconds[(7 * k) % n_folders] for k in range(n_folders)]        # long and short folders interleaved
    folders, total = [], 0
    for k, s in enumerate(seconds):
        fps = 25 if k % 2 == 0 else 30
        w, h = int(rng.integers(60, 201)), int(rng.integers(60, 201))
        path = os.path.join(root, f"video_{k:02d}")
        os.makedirs(os.path.join(path, "00"))
        for i in range(s * fps):
            file = os.path.join(path, "00", vc.frame_name(i))
            Image.fromarray(pool[(i + 5 * k) % len(pool)][:h, :w]).save(file, "JPEG", quality=95, subsampling=2)
            total += os.path.getsize(file)
        folders.append(vc.FaceFolder(f"video_{k:02d}", path, fps, s * fps))
    return folders, seconds, total


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return {"median": round(statistics.median(ms), 2), "min": round(min(ms), 2), "max": round(max(ms), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folders", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", type=int, default=MODE_DEFAULT)
    ap.add_argument("--max-frames-per-pass", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_corpus_bench.json"))
    args = ap.parse_args()

    engine = Engine(0)
    engine.load_static(synth.to_torch(synth.static_state_dict(42)))
    engine.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    with tempfile.TemporaryDirectory() as tmp:
        folders, seconds, file_bytes = write_corpus(tmp, args.folders)
        kw = dict(mode=args.mode, max_frames_per_pass=args.max_frames_per_pass)

        def loop():
            return [preprocess_video_and_predict(engine, f.path, "", f.fps, f.total_frames, False, args.mode, decode="device") for f in folders]

        def packed(entropy):
            res = vc.run_video_corpus(engine, folders, entropy=entropy, **kw)
            rows = torch.cat([torch.cat([r["static_probs"], r["dynamic_logits"]], dim=1) for r in res]).cpu().numpy()
            return res, rows

        arms = {"run_video_corpus_entropy_host": lambda: packed("host"), "run_video_corpus_entropy_device": lambda: packed("device"),
                "preprocess_video_and_predict_loop": loop}
        # warm-up, the launch counts, and the condition of every timing: the packed arms' tables are the loop's, bit for bit
        engine.gemm_stats(reset=True)
        ref = loop()
        torch.cuda.synchronize()
        launches = {"preprocess_video_and_predict_loop": engine.gemm_stats(reset=True)[0] / len(folders)}
        want = np.concatenate([np.concatenate([stat, dyn], axis=1) for dyn, stat in ref])
        passes = None
        for name in list(arms)[:2]:
            res, rows = arms[name]()
            torch.cuda.synchronize()
            launches[name] = engine.gemm_stats(reset=True)[0] / len(folders)
            assert rows.shape == want.shape and np.array_equal(rows, want), f"{name}: tables differ from the per-folder loop's"
            passes = res.passes
        assert engine.x3_fallbacks == 0, "a range-contract repeat would be timed as if it were the call"
        ms = {name: [] for name in arms}
        for _ in range(args.reps):                                            # interleaved: drift of a shared host hits every arm
            for name, fn in arms.items():
                ms[name].append(wall(fn)[0])
        # the packed call taken apart (entropy="host" and "device"): files, files + decode, the models on resident tiles
        plan = vc.corpus_plan(folders, args.max_frames_per_pass)
        queue = torch.empty((max(plan.passes), 224, 224, 3), dtype=torch.uint8, device=engine.device)

        def cuts():
            at = 0
            for n in plan.passes:
                yield at, n
                at += n

        def read_all():
            return [vc.read_files(plan.files[a:a + n]) for a, n in cuts()]

        def read_decode(entropy):
            for a, n in cuts():
                vc.decode_pass(engine, vc.read_files(plan.files[a:a + n]), queue[:n], "device", entropy)

        def models():
            """The static passes over whatever the buffer holds, the set's LSTM call and the table gathers: the call without its files."""
            outs = [engine.static_forward(queue[:n], args.mode)[1:] for _, n in cuts()]
            _tables(engine, _DevicePlan(engine, None, None, plan.host), torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]),
                    int(plan.frame_off[-1]), args.mode)

        parts = {"read_files_ms": [], "read_and_decode_entropy_host_ms": [], "read_and_decode_entropy_device_ms": [], "models_and_tables_ms": []}
        for _ in range(args.reps):
            parts["models_and_tables_ms"].append(wall(models)[0])
            parts["read_files_ms"].append(wall(read_all)[0])
            parts["read_and_decode_entropy_host_ms"].append(wall(lambda: read_decode("host"))[0])
            parts["read_and_decode_entropy_device_ms"].append(wall(lambda: read_decode("device"))[0])
        assert engine.x3_fallbacks == 0
    med = {k: statistics.median(v) for k, v in parts.items()}
    whole = {e: statistics.median(ms[f"run_video_corpus_entropy_{e}"]) for e in ("host", "device")}
    split = {e: {"read_files_ms": round(med["read_files_ms"], 2),
                 "decode_ms": round(med[f"read_and_decode_entropy_{e}_ms"] - med["read_files_ms"], 2),
                 "models_and_tables_ms": round(med["models_and_tables_ms"], 2), "whole_call_ms": round(whole[e], 2)} for e in ("host", "device")}
    m_loop = statistics.median(ms["preprocess_video_and_predict_loop"])
    res = {"tool": "tools/video_corpus_bench.py", "kernel_source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
           "mode": args.mode, "folders": len(folders), "folder_seconds": seconds, "folder_fps": [f.fps for f in folders],
           "files": plan.n_tiles, "mean_file_bytes": round(file_bytes / plan.n_tiles, 1), "crops": "60..200 px a side, quality 95, 4:2:0",
           "seconds_of_video": sum(seconds), "reps": args.reps, "interleaved": True, "every_arm_equals_the_loop_bit_for_bit": True,
           "max_frames_per_pass": args.max_frames_per_pass, "passes": passes, "host_threads": jpeg.host_threads(0),
           "ms": {name: spread(v) for name, v in ms.items()},
           "packed_over_loop": {e: round(whole[e] / m_loop, 3) for e in whole},
           "gemm_family_launches_per_folder": {k: round(v, 2) for k, v in launches.items()},
           "packed_call_parts": {**{k: spread(v) for k, v in parts.items()}, "split": split,
                                 "note": "parts measured on their own, one after the other, each behind a device synchronisation; in the call "
                                         "a reader thread fetches the next pass and the host's entropy pass overlaps the device's CNN on the "
                                         "pass before, so the parts add up to more than the call"},
           "x3_fallbacks": engine.x3_fallbacks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("files", "ms", "packed_over_loop", "gemm_family_launches_per_folder", "passes")}))
    print(json.dumps(res["packed_call_parts"]["split"]))


if __name__ == "__main__":
    main()
