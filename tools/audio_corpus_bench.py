"""Cost of the audio model over a corpus (avcer_amd/audio_corpus.py): 64 files of 2 to 12 s at 16 kHz, AFEW-style windows (every 2 s,
4 s long), synthetic weights.  Writes profiles/audio_corpus_bench.json.
`python tools/audio_corpus_bench.py [--files 64] [--reps 5] [--windows-per-pass 128] [--copy-to FILE]`.

Arms, run interleaved --reps times on the same build, median (min..max) of the synchronised wall clock, host waveforms in, window
logits on the device out, every arm asserting the same bits in every row:
  * packed     ONE audio_corpus.run_corpus call: one sample buffer, passes of --windows-per-pass windows, one vote launch, one
               guarded range-contract read
  * per_file   what a caller had to write before: per file one guarded Engine.audio_chunks + Engine.audio_forward call on that
               file's windows
Beside them the vote kernel alone between two HIP events.  Nothing is gated and no ratio is promised: the figures are what they are."""
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
from avcer_amd.build import source_hash  # noqa: E402
from avcer_amd.engine import MODE_DEFAULT, Engine  # noqa: E402

SR, MAX_W = 16000, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows-per-pass", type=int, default=128)
    ap.add_argument("--copy-to", default=None, help="write the result to this path as well")
    args = ap.parse_args()
    engine = Engine(0)
    engine.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    rng = np.random.default_rng(3)
    lens = rng.integers(2 * SR, 12 * SR + 1, args.files)
    labels = list(ac.AFEW_TO_ABAW)
    files = [(f"f{k:03d}.wav", synth.waveforms(100 + k, 1, int(n))[0]) for k, n in enumerate(lens)]
    tables = [ac.afew_windows(int(n), labels[k % len(labels)]) for k, n in enumerate(lens)]
    n_win = sum(len(t) for t in tables)

    def packed():
        return ac.run_corpus(engine, files, tables, SR, MAX_W, windows_per_pass=args.windows_per_pass).logits

    def per_file():
        out = []
        for (_, wav), tab in zip(files, tables):
            cuts = [ac.window_samples(a, b, SR, MAX_W, tab.kind) for a, b in zip(tab.start_t, tab.end_t)]
            starts = np.asarray([min(a, len(wav)) for a, _ in cuts], np.int64)
            ends = np.asarray([min(b, len(wav)) for _, b in cuts], np.int64)
            dev = torch.from_numpy(wav).to(engine.device)
            out.append(engine.guarded(MODE_DEFAULT, lambda m: engine.audio_forward(
                engine.audio_chunks(dev, starts, ends, MAX_W * SR, "constant"), normalize=True, mode=m)))
        return torch.cat(out)

    arms = {"packed": packed, "per_file": per_file}
    want = packed().cpu().numpy().view(np.uint32)  # warm-up, and the rows every arm must give
    per_file()
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want), name

    res = ac.run_corpus(engine, files, tables, SR, MAX_W, windows_per_pass=args.windows_per_pass)
    vote_ms = []
    for i in range(args.reps + 2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        engine.window_votes(res.logits, res.targets, res.file_off)
        e[1].record()
        torch.cuda.synchronize()
        if i >= 2:
            vote_ms.append(e[0].elapsed_time(e[1]))

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}

    result = {
        "what": "audio model over a corpus, host waveforms to window logits", "files": args.files, "windows": int(n_win),
        "seconds_of_audio": float(lens.sum() / SR), "windows_per_pass": args.windows_per_pass, "passes": list(res.passes),
        "reps": args.reps, "interleaved": True, "arms": {k: summary(v) for k, v in times.items()},
        "packed_over_per_file": statistics.median(times["packed"]) / statistics.median(times["per_file"]),
        "vote_kernel": dict(summary(vote_ms), note="one launch, the offset copy and five allocations included: launch-bound"),
        "x3_fallbacks": int(engine.x3_fallbacks), "gpu": torch.cuda.get_device_name(0), "kernel_source_hash": source_hash(),
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for path in [os.path.join(ROOT, "profiles", "audio_corpus_bench.json")] + ([args.copy_to] if args.copy_to else []):
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
