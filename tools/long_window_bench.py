#!/usr/bin/env python3
"""Time of the audio model on windows of 4, 8, 16, 30 and 100 s (199 .. 4999 tokens), ExprModelV3 and ExprModelV1, x3 and fp32, and
an interleaved A/B of the streaming attention kernels (avcer_attention_long) against the whole-head ones (avcer_attention) at 199
and 256 tokens.  Writes profiles/long_window_bench.json; there is no speed gate on it (no earlier number exists past 256 tokens):
the file is the record.

    python tools/long_window_bench.py [--reps 5] [--out profiles/long_window_bench.json]

Per length one call of one pass's worth of windows (max(1, 128 * 256 / tokens), at most 8), synthetic weights and waveforms; the
median of `reps` calls after one warm-up call, timed with events on the stream."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import build, synth  # noqa: E402
from avcer_amd.audio_pipeline import window_tokens  # noqa: E402
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine  # noqa: E402

SECONDS = (4, 8, 16, 30, 100)
MODES = (("x3", MODE_F16X3), ("fp32", MODE_FP32))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def model_rows(reps):
    rows = []
    for name, sd in (("ExprModelV3", synth.audio_state_dict(42)), ("ExprModelV1", synth.audio_v1_state_dict(44))):
        eng = Engine(0)
        eng.load_audio(sd, max_tokens=5000)
        for sec in SECONDS:
            t = sec * 16000
            tokens = window_tokens(t)
            n = min(8, max(1, 128 * 256 // tokens))
            wav = torch.from_numpy(synth.waveforms(900 + sec, n, t)).to(eng.device)
            for mname, mode in MODES:
                med, ms = timed(lambda: eng.audio_forward(wav, True, mode), reps)
                assert torch.isfinite(eng.audio_forward(wav, True, mode)).all()
                rows.append({"model": name, "mode": mname, "seconds": sec, "tokens": tokens, "windows": n, "ms_per_call": med,
                             "ms_per_window": med / n, "ms_per_second_of_audio": med / n / sec, "calls_ms": ms})
                print(rows[-1], flush=True)
        eng.close()
    return rows


def attention_ab(reps):
    """The two kernels in turn on the same tensors, 16 heads x 64, 128 windows (one pass of the forward): [present, long] per call"""
    eng = Engine(0)
    rows = []
    for tokens in (199, 256):
        n, heads, d = 128, 16, 64
        qkv = torch.randn(n, tokens, 3 * heads * d, device=eng.device)
        for form, ik, ok, x, out in (("x3", 0, 2, qkv, torch.empty(n, tokens, 2 * heads * d, dtype=torch.int16, device=eng.device)),
                                     ("fp32", 0, 0, qkv, torch.empty(n, tokens, heads * d, device=eng.device)),
                                     ("bf16", 1, 1, qkv.bfloat16(), torch.empty(n, tokens, heads * d, dtype=torch.bfloat16, device=eng.device))):
            a_ms, b_ms = [], []
            for i in range(reps + 1):
                for fn, acc in ((eng.attention, a_ms), (eng.attention_long, b_ms)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(x, out, n, tokens, heads, d, 0.125, ik, ok)
                    e1.record()
                    e1.synchronize()
                    if i:
                        acc.append(e0.elapsed_time(e1))
            rows.append({"tokens": tokens, "form": form, "windows": n, "heads": heads, "head_dim": d,
                         "present_ms": statistics.median(a_ms), "long_ms": statistics.median(b_ms),
                         "long_over_present": statistics.median(b_ms) / statistics.median(a_ms)})
            print(rows[-1], flush=True)
    eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_window_bench.json"))
    a = ap.parse_args()
    res = {"tool": "tools/long_window_bench.py", "kernel_source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
           "reps": a.reps, "attention_ab_interleaved": attention_ab(a.reps), "windows": model_rows(a.reps)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
