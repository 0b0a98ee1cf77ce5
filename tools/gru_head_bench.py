"""Cost of the GRU head (ExprModelV1): the in-kernel recurrence per step, beside the LSTM's launch pair per step, and the whole
model beside ExprModelV3.  Writes profiles/gru_head_bench.json.  `python tools/gru_head_bench.py [--iters 20]`.

(a) avcer_gru_layer alone (Engine.gru_layer; the f32 form is exactly the model's launch, the x3 form adds the split and the
    fragment copy of W_hh in front of it -- two small launches the model does once per load, so (a) in x3 is an upper bound):
    time between two events around one warm call, median / min / max of --iters, divided by the steps; n = 1, 16, 128 windows,
    S = 99 and 199, both arithmetic modes;
(b) in the same process, the existing LSTM (avcer_dynamic_forward_mode, unchanged code) at the same n: its call time over its
    18 recurrent steps (2 layers x 9 steps with a contraction + a cell launch; the two projections and 2 first cells ride along):
    the yardstick for one launch pair per step;
(c) whole ExprModelV1 forward beside whole ExprModelV3 forward (unchanged code) at 1 and 128 windows of 2 s and 4 s, x3 mode;
(d) the MFMA launch counts of both (profile families).
Nothing here is a pass / fail figure."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import synth  # noqa: E402
from avcer_amd.build import source_hash  # noqa: E402
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine  # noqa: E402

MODES = (("fp32", MODE_FP32), ("x3", MODE_F16X3))


def _call_us(fn, iters: int, warm: int = 3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_head_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_head_bench: needs the GPU (no CPU fallback: a CPU time says nothing about this kernel)")
    eng = Engine(0)
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": source_hash(), "iters": a.iters,
           "gru_layer": [], "lstm": [], "whole_model": [], "launches": {}}

    # (a) the recurrence alone
    w = torch.from_numpy(synth.uniform(1, "w", (768, 256), -1 / 16, 1 / 16)).cuda()
    b = torch.from_numpy(synth.uniform(1, "b", (768,), -1 / 16, 1 / 16)).cuda()
    for n in (1, 16, 128):
        for s in (99, 199):
            xp = torch.from_numpy(synth.centered(2, "xp", (n, s, 768), 0.6)).cuda()
            for mname, mode in MODES:
                t = _call_us(lambda: eng.gru_layer(xp, w, b, mode=mode), a.iters)
                t.update(n=n, steps=s, mode=mname, us_per_step=t["median_us"] / s)
                res["gru_layer"].append(t)
                print("gru_layer", t)

    # (b) the LSTM's launch pair per step, same process
    eng.load_dynamic(synth.dynamic_state_dict(42))
    for n in (1, 16, 128):
        win = torch.from_numpy(synth.centered(3, "win", (n, 10, 512), 1.0)).cuda()
        for mname, mode in MODES:
            t = _call_us(lambda: eng.dynamic_forward(win, mode=mode), a.iters)
            t.update(n=n, mode=mname, recurrent_steps=18, us_per_recurrent_step=t["median_us"] / 18)
            res["lstm"].append(t)
            print("lstm", t)

    # (c) whole models, (d) launch counts
    sds = {"ExprModelV1": synth.audio_v1_state_dict(44), "ExprModelV3": synth.audio_state_dict(42)}
    for name, sd in sds.items():
        eng.load_audio(sd)
        for seconds in (2, 4):
            for n in (1, 128):
                wav = torch.from_numpy(synth.waveforms(5, n, 16000 * seconds)).cuda()
                t = _call_us(lambda: eng.audio_forward(wav, True, MODE_F16X3), max(5, a.iters // 2))
                t.update(model=name, windows=n, seconds=seconds, mode="x3")
                res["whole_model"].append(t)
                print("whole", t)
            wav = torch.from_numpy(synth.waveforms(5, 1, 16000 * seconds)).cuda()
            eng.profile_enable(True)
            eng.audio_forward(wav, True, MODE_F16X3)
            fam = eng.profile_read_families()
            eng.profile_enable(False)
            res["launches"][f"{name}_{seconds}s"] = {k: v[1] for k, v in fam.items() if v[1]}
    print("launches", res["launches"])
    eng.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
