"""Cost of the fusion weight search on the GPU (avcer_amd/weight_search.py, csrc/search.hip) at the reference's own
configurations, on synthetic tables of 300 000 frames.  Writes profiles/weight_search_bench.json.
`python tools/weight_search_bench.py [--frames 300000] [--iters 10] [--cpu-candidates 8]`.

* configurations: 10 000 Dirichlet candidates at M = 3 (get_pred_av.py:352, data/utils.py:138), the 98^2 grid at M = 2
  (get_pred_video.py:362) and the 10^3 grid at M = 3 (get_pred_av.py:354), C = 7;
* `kernel_ms`: time between two HIP events around ONE Engine.weight_search_counts call on device-resident inputs (warm,
  median / min / max of --iters): the two memsets and the kernel;
* `search_ms`: synchronised wall clock of weight_search.search (tables and candidates from host memory, counts back, metrics and
  selection on the host), warm, median of --iters: what a caller waits for;
* f64 operations per second over kernel_ms, counting M * C multiplies and (M - 1) * C adds per candidate-frame pair and nothing
  else (the argmax and the counters are not counted);
* beside it, counts_numpy on the first --cpu-candidates candidates on this host (one process, numpy as the environment threads
  it), scaled to the whole candidate list: context, measured on a stated fraction, not a gate.
No time is gated: the capability is new and has nothing to be compared with."""
from __future__ import annotations

import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import synth  # noqa: E402
from avcer_amd import weight_search as ws  # noqa: E402
from avcer_amd.build import source_hash  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402

C = 7


def _kernel_ms(fn, iters: int):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return ts


def _wall_ms(fn, iters: int):
    fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def _summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-candidates", type=int, default=8)
    a = ap.parse_args()
    eng = Engine(0)
    np.random.seed(42)
    configs = {
        "dirichlet_10000_m3": (3, ws.dirichlet_weights(10000, 3, C)),
        "grid_98x98_m2": (2, ws.grid_weights(np.arange(0.01, 0.5, 0.005), 2, C)),
        "grid_10x10x10_m3": (3, ws.grid_weights(np.arange(0.01, 0.5, 0.05), 3, C)),
    }
    res = {"frames": a.frames, "classes": C, "iters": a.iters, "kernel_source_hash": source_hash(),
           "gpu": torch.cuda.get_device_name(0), "host": {"machine": platform.machine(), "cpus_usable": len(os.sched_getaffinity(0)),
                                                         "numpy": np.__version__},
           "cases": {}}
    for name, (m, weights) in configs.items():
        labels, tables = synth.fusion_tables(300 + m, a.frames, m, C)
        w = weights.shape[0]
        p = eng._dev(tables, torch.float64)
        lab = eng._dev(labels, torch.int32)
        wt = eng._dev(weights, torch.float64)
        kernel = _summary(_kernel_ms(lambda: eng.weight_search_counts(p, lab, wt), a.iters))
        search = _summary(_wall_ms(lambda: ws.search(eng, labels, list(tables), weights), a.iters))
        r = ws.search(eng, labels, list(tables), weights)
        k = min(a.cpu_candidates, w)
        t0 = time.perf_counter()
        cpu_tp, cpu_pred = ws.counts_numpy(tables, labels, weights[:k])
        cpu_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(cpu_tp, r.tp[:k]) and np.array_equal(cpu_pred, r.pred[:k])
        ops = float(w) * a.frames * (2 * m - 1) * C
        res["cases"][name] = {
            "models": m, "candidates": w, "candidate_frame_pairs": w * a.frames, "f64_ops": ops,
            "kernel_ms": kernel, "search_ms": search, "f64_tflops_over_kernel_median": ops / (kernel["median"] * 1e-3) / 1e12,
            "best_index": r.best_index, "best_metric": r.best_metric,
            "cpu_counts_numpy": {"candidates_measured": k, "fraction_of_candidates": k / w, "ms": cpu_ms, "ms_per_candidate": cpu_ms / k,
                                 "scaled_to_all_candidates_s": cpu_ms / k * w / 1e3, "counts_equal_gpu": True},
        }
        print(name, json.dumps(res["cases"][name]), flush=True)
        del p, lab, wt
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "weight_search_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
