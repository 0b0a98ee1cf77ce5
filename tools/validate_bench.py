"""Cost of validating audio checkpoints (avcer_amd/validate.py): 8 synthetic checkpoints over a corpus of 64 files of 2 to 12 s at
16 kHz, AFEW-style windows (every 2 s, 4 s long).  Writes profiles/validate_bench.json.
`python tools/validate_bench.py [--files 64] [--checkpoints 8] [--reps 5] [--copy-to FILE]`.

Arms, run interleaved --reps times on the same build, median (min..max) of the synchronised wall clock, state dicts and host
waveforms in, the per-epoch table out, every arm asserting the same numbers (the four scores exactly; the loss within 1e-4
relative: the loop's torch loss is float32, as the reference's is, the device's float64):
  * device   ONE validate.validate_checkpoints call: per checkpoint Engine.load_audio, run_corpus (planned once, waveforms uploaded
             once), one avcer_window_losses launch, the confusion launch, one fetch
  * loop     what a caller had to write before: per checkpoint Engine.load_audio and run_corpus, the logits fetched, torch-CPU
             CrossEntropyLoss per batch and sklearn's four scores on one thread
Beside them the loss launch alone between two HIP events.  Nothing is gated and no ratio is promised: the figures are what they are."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import audio_corpus as ac  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd import validate as va  # noqa: E402
from avcer_amd.build import source_hash  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402

SR, MAX_W, BSZ = 16000, 4, 64


def main():
    from sklearn import metrics as sk

    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--checkpoints", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copy-to", default=None, help="write the result to this path as well")
    args = ap.parse_args()
    torch.set_num_threads(1)
    engine = Engine(0)
    rng = np.random.default_rng(3)
    lens = rng.integers(2 * SR, 12 * SR + 1, args.files)
    labels = list(ac.AFEW_TO_ABAW)
    files = [(f"f{k:03d}.wav", synth.waveforms(100 + k, 1, int(n))[0]) for k, n in enumerate(lens)]
    tables = [ac.afew_windows(int(n), labels[k % len(labels)]) for k, n in enumerate(lens)]
    n_win = sum(len(t) for t in tables)
    checkpoints = [(k + 1, synth.to_torch(synth.audio_state_dict(42 + k))) for k in range(args.checkpoints)]
    weights = va.class_weights(rng.integers(40, 900, 8))
    names = ("recall", "precision", "f1", "accuracy")

    def device():
        return va.validate_checkpoints(engine, checkpoints, files, tables, weights=weights, batch_size=BSZ, metrics=names)[0]

    def loop():
        ce = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(weights), label_smoothing=0.2)
        rows = []
        for epoch, sd in checkpoints:
            engine.load_audio(sd)
            res = ac.run_corpus(engine, files, tables, SR, MAX_W)
            logits, y = res.logits.cpu(), torch.from_numpy(res.targets.astype(np.int64))
            running = sum(ce(logits[i:i + BSZ], y[i:i + BSZ]).item() * BSZ for i in range(0, len(y), BSZ))
            pred = torch.softmax(logits, dim=-1).numpy().argmax(axis=1)
            kw = dict(average="macro", zero_division=np.nan)
            rows.append({"epoch": epoch, "devel_loss": running / -(-len(y) // BSZ), "devel_recall": sk.recall_score(res.targets, pred, **kw),
                         "devel_precision": sk.precision_score(res.targets, pred, **kw), "devel_f1": sk.f1_score(res.targets, pred, **kw),
                         "devel_accuracy": sk.accuracy_score(res.targets, pred)})
        return rows

    def same(a, b):
        return all(x["epoch"] == y["epoch"] and abs(x["devel_loss"] - y["devel_loss"]) <= 1e-4 * abs(y["devel_loss"]) and
                   all(x[f"devel_{m}"] == y[f"devel_{m}"] for m in names) for x, y in zip(a, b))

    arms = {"device": device, "loop": loop}
    want = device()  # warm-up, and the table every arm must give (the loop's loss is float32: 1e-4 relative)
    assert same(loop(), want)
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert same(got, want), name

    res = ac.run_corpus(engine, files, tables, SR, MAX_W)
    loss_ms = []
    for i in range(args.reps + 2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        va.window_losses(engine, res.logits, res.targets, "ce", weights, 0.2, 0.0, BSZ)
        e[1].record()
        torch.cuda.synchronize()
        if i >= 2:
            loss_ms.append(e[0].elapsed_time(e[1]))

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}

    result = {
        "what": "validation of audio checkpoints, state dicts and host waveforms to the per-epoch table", "files": args.files,
        "checkpoints": args.checkpoints, "windows": int(n_win), "seconds_of_audio": float(lens.sum() / SR), "batch_size": BSZ,
        "reps": args.reps, "interleaved": True, "arms": {k: summary(v) for k, v in times.items()},
        "device_over_loop": statistics.median(times["device"]) / statistics.median(times["loop"]),
        "loss_launch": dict(summary(loss_ms), note="one launch, the weight and target copies and four allocations included: launch-bound"),
        "table": want, "gpu": torch.cuda.get_device_name(0), "kernel_source_hash": source_hash(),
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for path in [os.path.join(ROOT, "profiles", "validate_bench.json")] + ([args.copy_to] if args.copy_to else []):
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
