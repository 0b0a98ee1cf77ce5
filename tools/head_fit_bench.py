"""Cost of fitting the audio classifier head (avcer_amd/head_fit.py): n = 20 000 feature rows of F = 1024, C = 8 classes, batches of
64, 10 epochs -- 3 130 dependent Adam steps a run --, the reference's recipe (weighted cross entropy with label smoothing 0.2,
mixup, lr 1e-4, CosineAnnealingWarmRestarts).  Writes profiles/head_fit_bench.json.
`python tools/head_fit_bench.py [--rows 20000] [--epochs 10] [--reps 5] [--copy-to FILE]`.

Arms, run interleaved --reps times on the same build, median (min..max) of the synchronised wall clock, features on the device
and host tables in, the weights of every epoch on the device out:
  * fit_1, fit_16, fit_256   ONE head_fit.fit_heads call of K = 1, 16, 256 runs (seeds differ): the host checks of the tables, their
                             upload and one avcer_head_fit launch of K workgroups
  * torch_1                  one run as a torch loop on the same GPU: index_select, the mixup, nn.Linear, CrossEntropyLoss, backward,
                             torch.optim.Adam and the scheduler's step per iteration, the batch losses kept on the device (no .item())
Beside them the avcer_head_fit launch alone between two HIP events.  Before anything is timed every arm must meet the tolerance of
tests/test_gpu_head_fit.py against head_fit_numpy on a prefix (--check-rows rows, 2 epochs): 4 x the deviation of a float32 torch CPU
run from the float64 one.  Nothing is gated and no ratio is promised: the figures are what they are."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import head_fit_cases as cases  # noqa: E402
from avcer_amd import head_fit as hf  # noqa: E402
from avcer_amd import validate as va  # noqa: E402
from avcer_amd.build import source_hash  # noqa: E402
from avcer_amd.engine import Engine  # noqa: E402

F, C, BSZ, ALPHA = 1024, 8, 64, 0.3


def make_runs(k, n, epochs, weights, rng):
    bound = 1.0 / np.sqrt(F)
    runs = []
    for seed in range(k):
        lam, index = hf.make_mixup(n, epochs, BSZ, ALPHA, seed)
        runs.append(hf.HeadRun(w0=rng.uniform(-bound, bound, (C, F)).astype(np.float32), b0=rng.uniform(-bound, bound, C).astype(np.float32),
                               order=hf.make_order(n, epochs, seed), weights=weights, mix_lam=lam, mix_index=index))
    return runs


def torch_loop(x_all, y_all, run, epochs, first_epoch=1):
    """One run on the device tensors x_all [n, F], y_all [n]: (w_hist, b_hist, batch_loss) as device tensors."""
    dev = x_all.device
    n = x_all.shape[0]
    iters = -(-n // BSZ)
    lin = torch.nn.Linear(F, C).to(dev)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(run.w0))
        lin.bias.copy_(torch.from_numpy(run.b0))
    loss = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(run.weights).to(dev), label_smoothing=run.label_smoothing)
    opt = torch.optim.Adam(lin.parameters(), lr=run.lr, betas=run.betas, eps=run.eps)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=run.t0, eta_min=run.eta_min)
    order, index = torch.from_numpy(run.order).to(dev), torch.from_numpy(run.mix_index.astype(np.int64)).to(dev)
    lam_all = torch.from_numpy(run.mix_lam).to(dev)
    w_hist, b_hist = torch.empty(epochs, C, F, device=dev), torch.empty(epochs, C, device=dev)
    batch_loss = torch.empty(epochs, iters, device=dev)
    for e in range(epochs):
        for i in range(iters):
            rows = order[e, i * BSZ:(i + 1) * BSZ]
            x, y = x_all[rows], y_all[rows]
            lam, idx = lam_all[e, i], index[e, i * BSZ:i * BSZ + rows.shape[0]]
            hot = torch.nn.functional.one_hot(y, C)
            x = lam * x + (1 - lam) * x[idx]
            y = (lam * hot + (1 - lam) * hot[idx]).argmax(1)
            opt.zero_grad()
            value = loss(lin(x), y)
            value.backward()
            opt.step()
            sched.step(first_epoch + e + i / iters)
            batch_loss[e, i] = value.detach()
        w_hist[e], b_hist[e] = lin.weight.detach(), lin.bias.detach()
    return w_hist, b_hist, batch_loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=640)
    ap.add_argument("--copy-to", default=None, help="write the result to this path as well")
    args = ap.parse_args()
    engine = Engine(0)
    rng = np.random.default_rng(11)
    n = args.rows
    feats = (rng.standard_normal((n, F)) * 0.5).astype(np.float32)
    targets = rng.integers(0, C, n)
    weights = va.class_weights(rng.integers(40, 900, C))
    x_dev, y_dev = torch.from_numpy(feats).to(engine.device), torch.from_numpy(targets).to(engine.device)

    # ---- every arm against the statement on a prefix, at the GPU test's tolerance
    m = min(args.check_rows, n)
    check_runs = make_runs(2, m, 2, weights, rng)
    want = hf.head_fit_numpy(feats[:m], targets[:m], check_runs, 2, BSZ)
    devs = [cases.deviation(cases.torch_fit(feats[:m], targets[:m].astype(np.int64), r, BSZ, torch.float32, epochs=2), w) for r, w in zip(check_runs, want)]
    tol = [max(4.0 * d, max(devs)) for d in devs]
    fit = hf.fit_heads(engine, x_dev[:m], targets[:m], check_runs, 2, BSZ)
    checked = {"rows": m, "epochs": 2, "f32_dev": devs, "tolerance": tol}
    checked["fit_heads"] = [cases.deviation([fit.w_hist[k].cpu().numpy(), fit.b_hist[k].cpu().numpy(), fit.batch_loss[k].cpu().numpy()], want[k])
                            for k in range(2)]
    checked["torch_loop"] = [cases.deviation([t.cpu().numpy() for t in torch_loop(x_dev[:m], y_dev[:m], check_runs[k], 2)], want[k]) for k in range(2)]
    print(json.dumps(checked))
    for arm in ("fit_heads", "torch_loop"):
        assert all(d <= t for d, t in zip(checked[arm], tol)), (arm, checked[arm], tol)

    runs = make_runs(256, n, args.epochs, weights, rng)
    arms = {f"fit_{k}": (lambda k=k: hf.fit_heads(engine, x_dev, targets, runs[:k], args.epochs, BSZ)) for k in (1, 16, 256)}
    arms["torch_1"] = lambda: torch_loop(x_dev, y_dev, runs[0], args.epochs)
    for fn in arms.values():   # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)

    launch = {}
    for k in (1, 16, 256):
        pk = hf._pack(feats.shape, targets, runs[:k], args.epochs, BSZ, 1)
        tables = [torch.from_numpy(np.ascontiguousarray(v)).to(engine.device) for v in (pk.targets, pk.class_w, pk.w0, pk.b0, pk.order, pk.mix_lam, pk.mix_index)]
        ms = []
        for i in range(args.reps + 1):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            engine.head_fit(x_dev, tables[0], pk.hyper, *tables[1:5], tables[5], tables[6], args.epochs, BSZ)
            e[1].record()
            torch.cuda.synchronize()
            if i >= 1:
                ms.append(e[0].elapsed_time(e[1]))
        launch[f"fit_{k}"] = ms

    def summary(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}

    steps = args.epochs * -(-n // BSZ)
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {
        "what": "fitting the audio classifier head: features on the device and host tables to the weights of every epoch",
        "rows": n, "features": F, "classes": C, "batch_size": BSZ, "epochs": args.epochs, "steps_per_run": steps, "reps": args.reps,
        "interleaved": True, "arms": {k: summary(v) for k, v in times.items()},
        "launch_alone": {k: dict(summary(v), us_per_step=statistics.median(v) * 1e3 / steps) for k, v in launch.items()},
        "torch_1_over_fit_1": med["torch_1"] / med["fit_1"],
        "runs_per_second": {k: int(k.split("_")[1]) / (med[k] * 1e-3) for k in ("fit_1", "fit_16", "fit_256")},
        "torch_runs_per_second": 1.0 / (med["torch_1"] * 1e-3),
        "checked_against_head_fit_numpy": checked, "gpu": torch.cuda.get_device_name(0), "kernel_source_hash": source_hash(),
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for path in [os.path.join(ROOT, "profiles", "head_fit_bench.json")] + ([args.copy_to] if args.copy_to else []):
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
