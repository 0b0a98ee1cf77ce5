"""Cost of the waveform augmentations (avcer_amd/augment.py, csrc/augment.hip) on the corpus of tools/audio_corpus_bench.py: 64 files
of 2 to 12 s at 16 kHz, AFEW-style windows of 4 s, synthetic weights.  Writes profiles/augment_bench.json.
`python tools/augment_bench.py [--files 64] [--reps 5] [--windows-per-pass 128] [--copy-to FILE]`.

Run interleaved --reps times on the same build, median (min..max):
  * kernel        avcer_wave_augment alone on all windows of the corpus in one call, between two HIP events, per kind (all polarity,
                  all gain, all noise) and with the reference's mix; beside it the bytes it moves (compulsory: a sample read and
                  written once; kind 2 reads it twice more for the deviation) and a device-to-device copy of the same buffer in
                  the same run, the ceiling of anything that reads and writes every sample once
  * host          what the reference's __getitem__ pays per window, on ONE thread (torch.set_num_threads(1)): WhiteNoise.forward's
                  operations -- torch.std, np.random.normal, the float32 cast, the add -- on every window of the corpus
  * draw_plan     the host draws of the plan for all windows
  * run_corpus    the synchronised wall clock of audio_corpus.run_corpus with transform=None and with the default AugmentSpec
Nothing is gated and no ratio is promised: the figures are what they are."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import audio_corpus as ac  # noqa: E402
from avcer_amd import augment as ag  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd.build import source_hash  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402

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
    spec = ag.AugmentSpec(seed=0)
    win = MAX_W * SR

    plain = ac.run_corpus(engine, files, tables, SR, MAX_W, windows_per_pass=args.windows_per_pass)   # warm-up
    n = int(plain.starts.shape[0])
    base = np.repeat(np.cumsum([0] + [len(w) for _, w in files])[:-1], np.diff(plain.file_off))
    wav_all = torch.from_numpy(np.concatenate([w for _, w in files])).to(engine.device)
    chunks0 = engine.audio_chunks(wav_all, plain.starts + base, plain.ends + base, win, "constant")
    host_windows = chunks0.cpu()
    mixed = ag.draw_plan(spec, n)
    plans = {"polarity": ag.make_plan(np.full(n, 1)), "gain": ag.make_plan(np.full(n, 3), gain_db=mixed.gain_db),
             "noise": ag.make_plan(np.full(n, 2), u=mixed.u, key=mixed.key), "mixed": mixed}
    reads = {"polarity": 1, "gain": 1, "noise": 3}
    work = chunks0.clone()
    other = torch.empty_like(work)

    def timed(fn):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn()
        e[1].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1])

    def host_noise():
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            random.seed(0)
            np.random.seed(0)
            t0 = time.perf_counter()
            for w in range(n):
                audio = host_windows[w:w + 1]
                std = torch.std(audio).numpy()
                noise_std = random.uniform(1e-4 * std, 5e-3 * std)
                noise = np.random.normal(0.0, noise_std, size=audio.shape).astype(np.float32)
                audio + torch.Tensor(noise)
            return (time.perf_counter() - t0) * 1e3
        finally:
            torch.set_num_threads(threads)   # the run_corpus arms that follow keep torch's host pool as they found it

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def corpus(transform):
        return lambda: ac.run_corpus(engine, files, tables, SR, MAX_W, windows_per_pass=args.windows_per_pass, transform=transform)

    for name, plan in plans.items():    # warm-up
        ag.augment(engine, work, plan)
    corpus(spec)()
    times = {f"kernel_{k}": [] for k in plans}
    times.update({"copy": [], "host_noise": [], "draw_plan": [], "run_corpus_plain": [], "run_corpus_transform": []})
    for _ in range(args.reps):
        for name, plan in plans.items():
            work.copy_(chunks0)
            recs = plan.records()
            times[f"kernel_{name}"].append(timed(lambda: engine.wave_augment(work, recs, plan.min_snr, plan.max_snr)))
        times["copy"].append(timed(lambda: other.copy_(work)))
        times["host_noise"].append(host_noise())
        t0 = time.perf_counter()
        ag.draw_plan(spec, n)
        times["draw_plan"].append((time.perf_counter() - t0) * 1e3)
        times["run_corpus_plain"].append(wall(corpus(None)))
        times["run_corpus_transform"].append(wall(corpus(spec)))

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}

    nbytes = float(n * win * 4)
    kernels = {}
    for k in plans:
        s = summary(times[f"kernel_{k}"])
        if k in reads:
            s["bytes_read"], s["bytes_written"] = reads[k] * nbytes, nbytes
            s["tb_per_s"] = (reads[k] + 1) * nbytes / (s["median_ms"] * 1e-3) / 1e12
        else:
            s["kinds"] = {str(c): int((mixed.kind == c).sum()) for c in (1, 2, 3)}
        kernels[k] = s
    copy = summary(times["copy"])
    copy["tb_per_s"] = 2 * nbytes / (copy["median_ms"] * 1e-3) / 1e12
    result = {
        "what": "waveform augmentation of a corpus's windows: the kernel alone, the reference's host operations, run_corpus with and without",
        "files": args.files, "windows": n, "samples_per_window": win, "windows_per_pass": args.windows_per_pass, "reps": args.reps,
        "interleaved": True, "kernel": kernels, "copy_ceiling": dict(copy, note="torch copy_ of the same [windows, win] f32 buffer, device to device"),
        "host_white_noise_one_thread": dict(summary(times["host_noise"]), note="torch.std, np.random.normal, astype, add per window; "
                                            "every window, where RandomChoice sends a third of them there"),
        "draw_plan": summary(times["draw_plan"]),
        "run_corpus": {"plain": summary(times["run_corpus_plain"]), "transform": summary(times["run_corpus_transform"])},
        "plain_timed_against_parent_commit": False,
        "x3_fallbacks": int(engine.x3_fallbacks), "gpu": torch.cuda.get_device_name(0), "kernel_source_hash": source_hash(),
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for path in [os.path.join(ROOT, "profiles", "augment_bench.json")] + ([args.copy_to] if args.copy_to else []):
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
