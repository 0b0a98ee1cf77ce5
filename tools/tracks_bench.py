"""run.run_inference with `tracks=`: what the visual models and the fusion on every face track cost inside one call, against the K
separate calls a user of track 00 alone has to make -> profiles/tracks_bench.json.

One GPU, the synthetic models of the test suite (avcer_amd.synth), 750 frames of 640 x 360 on the device with 30 s of sound, supplied
detections of K = 1, 2 and 4 faces present throughout (no detector weights are needed; every arm does the same work behind them).
Arms, `--reps` interleaved repetitions each, seconds per call as median (min..max):

  none       tracks=None: today's call, track 00 alone
  zero       tracks=[0]: the same track through the per-track path
  all        tracks="all": K tracks in one call
  separate   K calls of tracks=None, each given ONE face's detections alone: the only way to the same tables without `tracks`
             (every call pays for the tracker, the crops and the whole audio branch again)

Every arm ASSERTS, at every repetition and before its time is recorded, that its track tables equal the first call's bit for bit
where they overlap (track 00), and `separate` that each of its calls equals `all`'s track of that face: a run whose arms disagree
stops with the arm and K named and writes no file.  Two conditions are read off the file: `zero` is not slower than `none` beyond the spread (their ranges overlap), and
`all` is faster than `separate` for K >= 2.
"""
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

from avcer_amd import run as arun  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd.engine import MODE_F16X3, Engine  # noqa: E402

W, H, FPS = 640, 360, 25
TABLES = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits")


def faces(k: int, n: int):
    """Per face its detections over n frames: a 120 x 150 box in its own quarter of the width, drifting by a pixel per frame."""
    out = []
    for j in range(k):
        x, y = 20 + 150 * j, 40 + 30 * (j % 2)
        out.append([np.array([[x + t % 9, y + t % 5, x + t % 9 + 120, y + t % 5 + 150, 0.99 - 0.01 * j] + [0] * 10], dtype=np.float32)
                    for t in range(n)])
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def same(a, b):
    return all(np.array_equal(a[key], b[key], equal_nan=True) for key in TABLES)


def spread(secs):
    return {"median": round(statistics.median(secs), 4), "min": round(min(secs), 4), "max": round(max(secs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=750)
    ap.add_argument("--faces", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_bench.json"))
    args = ap.parse_args()
    eng = Engine(0)
    eng.load_static(synth.to_torch(synth.static_state_dict(42)))
    eng.load_dynamic(synth.to_torch(synth.dynamic_state_dict(42)))
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    n = args.frames
    gen = torch.Generator(device="cpu").manual_seed(7)
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=gen).to(eng.device)
    wav = torch.from_numpy(synth.waveforms(3, 1, 16000 * n // FPS)[0]).to(eng.device)
    res = {"what": "run.run_inference, seconds per call: median of the interleaved repetitions (min, max)", "reps": args.reps, "frames": n,
           "size": f"{W}x{H}", "fps": FPS, "mode": "F16X3", "detections": "supplied; K faces present on every frame", "faces": {}}

    def call(dets, **kw):
        return arun.run_inference(eng, frames, wav, FPS, detections=dets, mode=MODE_F16X3, **kw)

    for k in args.faces:
        per_face = faces(k, n)
        dets = [np.concatenate([per_face[j][t] for j in range(k)]) for t in range(n)]
        arms = {"none": lambda: call(dets), "zero": lambda: call(dets, tracks=[0]), "all": lambda: call(dets, tracks="all"),
                "separate": lambda: [call(per_face[j]) for j in range(k)]}
        first = call(dets)                                                              # warm-up, and what the arms are held to
        for fn in arms.values():
            fn()
        secs = {name: [] for name in arms}
        for rep in range(args.reps):
            for name, fn in arms.items():
                s, out = timed(fn)
                # a time is recorded only for an arm that computed the same tables: arms that disagree did different work
                where = f"K={k}, arm {name!r}, repetition {rep}"
                if name == "separate":
                    assert same(out[0], first), f"{where}: face 0 alone differs from track 00 of the first call"
                    for j in range(k):
                        assert same(out[j], whole["tracks"][j]), f'{where}: face {j} alone differs from track {j:02d} of tracks="all"'
                else:
                    assert same(out, first), f"{where}: the top-level tables differ from the first call's"
                    assert "tracks" not in out or same(out["tracks"][0], first), f"{where}: track 00 differs from the first call's tables"
                if name == "all":
                    assert sorted(out["tracks"]) == list(range(k)), f"{where}: tracks {sorted(out['tracks'])}, not 0..{k - 1}"
                    whole = out
                secs[name].append(s)
        entry = {"seconds": {name: spread(secs[name]) for name in arms}, "tables_agree_bit_for_bit": {name: True for name in arms}}
        # not slower beyond the spread of the repetitions: the fastest `zero` is no slower than the slowest `none`
        entry["zero_not_slower_than_none_beyond_spread"] = bool(entry["seconds"]["zero"]["min"] <= entry["seconds"]["none"]["max"])
        entry["all_over_separate"] = round(entry["seconds"]["all"]["median"] / entry["seconds"]["separate"]["median"], 4)
        entry["all_over_none"] = round(entry["seconds"]["all"]["median"] / entry["seconds"]["none"]["median"], 4)
        res["faces"][str(k)] = entry
        print(json.dumps({str(k): entry}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
