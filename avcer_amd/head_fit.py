"""Fit the audio classifier head on the device: the train phase of the reference's NetTrainer.run for the last layer.

    head_fit_numpy      the statement: NetTrainer.iterate_model (net_trainer.py:357-467) with mixup_data (574-604) and the losses,
                        torch.optim.Adam and CosineAnnealingWarmRestarts of train_c_audio.py:236-260, for `feature_downsample`
                        (Linear F -> C) alone, in numpy float64
    augmented_views     the features of a corpus under V draws of the reference's waveform augmentation (avcer_amd/augment.py),
                        f32 [V, n, F]; head_fit_numpy and fit_heads take them, HeadRun.view says which view an epoch reads
    fit_heads           the same on the device: K runs -- seeds, rates, losses, mixup settings -- in ONE avcer_head_fit launch,
                        one workgroup a run (csrc/head_fit.hip)
    make_order / make_mixup   the random draws of a run, made on the host
    select              the devel phase for every run and epoch: avcer_head_apply, validate.window_losses, validate.measures,
                        validate.best_epoch
    write_checkpoint    the trainer's epoch_N.pth with the fitted head in a base checkpoint's place

The chain is audio_corpus.extract_features (or augmented_views) -> fit_heads -> select -> write_checkpoint ->
validate.validate_checkpoints.

Where this departs from the reference, on purpose: the reference trains the conv tail, tl1 / tl2 and the last 2-4 wav2vec2 blocks
too, in train mode with dropout, and mixes WAVEFORMS.  Here everything below `feature_downsample` is frozen and in eval mode -- its
output is extracted once (per augmented view, where the windows are augmented) --, and mixup mixes FEATURE rows.  This is linear
probing of the reference's model with the reference's recipe; nothing in the inference routes calls it.

The random numbers are not torch's: `make_order` and `make_mixup` draw from numpy's Generator, so a run here does not repeat the
batches DataLoader(shuffle=True) and np.random.beta / torch.randperm would deal under the same seed.  The tables are arguments:
whoever has torch's draws can pass them.

Epochs are numbered as NetTrainer.run numbers them, from `first_epoch` = 1: the scheduler is stepped with that number
(`scheduler.step(epoch + idx / iters)`, net_trainer.py:437) and the stats rows and checkpoints carry it."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import validate
from .validate import FOCAL_CLIP, LOSS_KINDS, LOSS_MAX_CLASSES

HYPER = 12             # include/avcer_hip.h AVCER_HEAD_HYPER
MAX_BATCH = 256        # AVCER_HEAD_MAX_BATCH
MAX_FEATURES = 1024    # AVCER_HEAD_MAX_FEATURES
MAX_STATE = 16384      # AVCER_HEAD_MAX_STATE


@dataclass
class HeadRun:
    """One run of a sweep.  w0 [C, F], b0 [C]: the starting head; order int64 [epochs, n]: per epoch a permutation of the rows,
    what DataLoader(shuffle=True) would deal; mix_lam f32 [epochs, n_batches] and mix_index int32 [epochs, n] (per batch a
    permutation of the positions inside that batch): mixup_data's lam and index per batch, both or neither."""
    w0: object = None
    b0: object = None
    order: object = None
    kind: str = "ce"
    weights: object = None
    label_smoothing: float = 0.2
    gamma: float = 0.0
    lr: float = 1e-4
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    t0: int = 10
    eta_min: float = 1e-4
    mix_lam: object = None
    mix_index: object = None
    view: object = None    # int [epochs]: which table of feats [V, n, F] epoch e takes its rows from; None: e % V


class HeadFitRun(NamedTuple):
    """What head_fit_numpy returns per run: w_hist f64 [epochs, C, F], b_hist f64 [epochs, C] (the state at the end of every
    epoch), batch_loss f64 [epochs, n_batches], epoch_loss f64 [epochs] (sum(loss_b * batch_size) / n_batches)."""
    w_hist: np.ndarray
    b_hist: np.ndarray
    batch_loss: np.ndarray
    epoch_loss: np.ndarray


class HeadFit(NamedTuple):
    """What fit_heads returns, on the device: w_hist f32 [K, epochs, C, F], b_hist f32 [K, epochs, C], batch_loss f32 [K, epochs,
    n_batches], epoch_loss f64 [K, epochs]; first_epoch: the number of epoch 0."""
    w_hist: object
    b_hist: object
    batch_loss: object
    epoch_loss: object
    first_epoch: int


class _Packed(NamedTuple):
    n: int
    f: int
    c: int
    epochs: int
    bsz: int
    n_batches: int
    targets: np.ndarray      # int32 [n]
    hyper: np.ndarray        # f64 [K, HYPER]
    class_w: np.ndarray      # f32 [K, C]
    w0: np.ndarray           # f32 [K, C, F]
    b0: np.ndarray           # f32 [K, C]
    order: np.ndarray        # int32 [K, epochs, n]
    mix_lam: Optional[np.ndarray]     # f32 [K, epochs, n_batches]
    mix_index: Optional[np.ndarray]   # int32 [K, epochs, n]
    views: Optional[int] = None       # V of feats [V, n, F]; None: feats [n, F]
    view: Optional[np.ndarray] = None  # int32 [K, epochs], with `views`


def _is_int(v, lo: int) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and v >= lo


def _pack(feats_shape, targets, runs: Sequence[HeadRun], epochs, batch_size, first_epoch) -> _Packed:
    """Every argument check of head_fit_numpy and fit_heads, before any work, and the runs as the tables avcer_head_fit takes."""
    if len(feats_shape) not in (2, 3) or min(feats_shape[:-1]) < 1:
        raise ValueError(f"features [n, F] or [V, n, F] with n >= 1 (and V >= 1) expected, got {tuple(feats_shape)}")
    views = int(feats_shape[0]) if len(feats_shape) == 3 else None
    n, f = int(feats_shape[-2]), int(feats_shape[-1])
    if not _is_int(epochs, 1):
        raise ValueError(f"epochs must be an integer >= 1, got {epochs!r}")
    if not _is_int(batch_size, 1) or batch_size > MAX_BATCH:
        raise ValueError(f"batch_size must be an integer in 1 .. {MAX_BATCH}, got {batch_size!r}")
    if not _is_int(first_epoch, 0):
        raise ValueError(f"first_epoch must be an integer >= 0, got {first_epoch!r}")
    runs = list(runs)
    if not runs:
        raise ValueError("no runs")
    epochs, bsz = int(epochs), int(batch_size)
    n_batches = -(-n // bsz)
    if runs[0].w0 is None or np.ndim(runs[0].w0) != 2:
        raise ValueError("run 0: w0 [C, F] expected")
    c = int(np.shape(runs[0].w0)[0])
    if f % 64 or not 64 <= f <= MAX_FEATURES or c * f > MAX_STATE:
        raise ValueError(f"{f} features, {c} classes: F a multiple of 64 up to {MAX_FEATURES}, C * F <= {MAX_STATE}")
    sizes = np.minimum(n, (np.arange(n_batches) + 1) * bsz) - np.arange(n_batches) * bsz
    t = None
    hyper = np.zeros((len(runs), HYPER))
    class_w = np.ones((len(runs), c), np.float32)
    w0, b0 = np.zeros((len(runs), c, f), np.float32), np.zeros((len(runs), c), np.float32)
    order = np.zeros((len(runs), epochs, n), np.int32)
    any_mix = any(r.mix_lam is not None or r.mix_index is not None for r in runs)
    mix_lam = np.ones((len(runs), epochs, n_batches), np.float32) if any_mix else None
    mix_index = np.zeros((len(runs), epochs, n), np.int32) if any_mix else None
    identity = np.arange(n, dtype=np.int64)
    view = None if views is None else np.tile(np.arange(epochs, dtype=np.int32) % views, (len(runs), 1))
    for k, r in enumerate(runs):
        if r.view is not None:
            vw = np.asarray(r.view)
            if views is None:
                raise ValueError(f"run {k}: view comes with features [V, n, F]")
            if vw.shape != (epochs,) or not np.issubdtype(vw.dtype, np.integer) or vw.min() < 0 or vw.max() >= views:
                raise ValueError(f"run {k}: view, integers [{epochs}] in 0 .. {views - 1}, expected, got {vw.dtype} {vw.shape}"
                                 + (f" in [{vw.min()}, {vw.max()}]" if vw.size and np.issubdtype(vw.dtype, np.integer) else ""))
            view[k] = vw
        kind, t, w = validate._check_loss(c, targets, r.kind, r.weights, r.label_smoothing, r.gamma, bsz)
        if t.shape[0] != n:
            raise ValueError(f"{n} feature rows and {t.shape[0]} targets")
        if len(tuple(r.betas)) != 2:
            raise ValueError(f"run {k}: betas (beta1, beta2) expected, got {r.betas!r}")
        scalars = {"lr": r.lr, "beta1": r.betas[0], "beta2": r.betas[1], "eps": r.eps, "eta_min": r.eta_min}
        for name, v in scalars.items():
            if not math.isfinite(float(v)):
                raise ValueError(f"run {k}: {name} must be finite, got {v!r}")
        if not (0.0 <= float(r.betas[0]) < 1.0 and 0.0 <= float(r.betas[1]) < 1.0) or float(r.eps) < 0.0:
            raise ValueError(f"run {k}: betas in [0, 1) and eps >= 0 expected, got {r.betas!r}, {r.eps!r}")
        if not _is_int(r.t0, 1):
            raise ValueError(f"run {k}: t0 must be an integer >= 1, got {r.t0!r}")
        if w is not None:
            if not np.isfinite(w).all():
                raise ValueError(f"run {k}: class weights must be finite")
            class_w[k] = w
        a, b = np.asarray(r.w0), None if r.b0 is None else np.asarray(r.b0)
        if a.shape != (c, f) or b is None or b.shape != (c,):
            raise ValueError(f"run {k}: w0 [{c}, {f}] and b0 [{c}] expected, got {a.shape} and {None if b is None else b.shape}")
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            raise ValueError(f"run {k}: w0 and b0 must be finite")
        w0[k], b0[k] = a, b
        o = None if r.order is None else np.asarray(r.order)
        if o is None or o.shape != (epochs, n) or not np.issubdtype(o.dtype, np.integer):
            raise ValueError(f"run {k}: order, integers [{epochs}, {n}], expected, got {None if o is None else (o.dtype, o.shape)}")
        if not (np.sort(o.astype(np.int64), axis=1) == identity[None, :]).all():
            raise ValueError(f"run {k}: every order[e] must be a permutation of 0 .. {n - 1}")
        order[k] = o
        if (r.mix_lam is None) != (r.mix_index is None):
            raise ValueError(f"run {k}: mix_lam and mix_index come together")
        if r.mix_lam is not None:
            lam, idx = np.asarray(r.mix_lam, dtype=np.float32), np.asarray(r.mix_index)
            if lam.shape != (epochs, n_batches) or idx.shape != (epochs, n) or not np.issubdtype(idx.dtype, np.integer):
                raise ValueError(f"run {k}: mix_lam [{epochs}, {n_batches}] and integer mix_index [{epochs}, {n}] expected, got "
                                 f"{lam.shape} and {idx.dtype} {idx.shape}")
            if not ((lam >= 0.0) & (lam <= 1.0)).all():   # a NaN fails both comparisons
                raise ValueError(f"run {k}: every mix_lam must lie in [0, 1]")
            full = n // bsz   # the whole batches in one sort, the short one behind them
            for i, part in ((0, idx[:, :full * bsz].reshape(epochs, full, bsz)), (full, idx[:, full * bsz:].reshape(epochs, 1, n - full * bsz))):
                wrong = (np.sort(part.astype(np.int64), axis=2) != identity[None, None, :part.shape[2]]).any(axis=(0, 2))
                if wrong.any():
                    i += int(np.argmax(wrong))
                    raise ValueError(f"run {k}: mix_index must be a permutation of 0 .. {sizes[i] - 1} inside batch {i}")
            mix_lam[k], mix_index[k] = lam, idx
        hyper[k, :11] = (kind, float(r.label_smoothing), float(r.gamma), float(r.lr), float(r.betas[0]), float(r.betas[1]),
                         float(r.eps), float(r.t0), float(r.eta_min), 0.0 if r.mix_lam is None else 1.0, float(first_epoch))
    return _Packed(n, f, c, epochs, bsz, n_batches, t, hyper, class_w, w0, b0, order, mix_lam, mix_index, views, view)


# ------------------------------------------------------------------------------------------------ the statement
def loss_and_grad(logits: np.ndarray, y: np.ndarray, kind: int, w: np.ndarray, label_smoothing: float, gamma: float):
    """One batch: (the batch loss as validate.losses_numpy has it, its gradient with respect to the logits [n_b, C]), float64.
    CE:          loss = (1 - eps) * A / U + (eps / C) * G / U with A = sum_i w[y_i] q[i, y_i], G = sum_i sum_k w[k] q[i, k], U = sum_i
                 w[y_i], q = -log_softmax;  dq[i, k] / dz[i, j] = p[i, j] - [k == j], hence
                 grad[i, j] = ((1 - eps) * w[y_i] * (p[i, j] - [j == y_i]) + (eps / C) * (sum(w) * p[i, j] - w[j])) / U
    soft focal:  loss = sum_i w[y_i] (1 - pc_i)^gamma (-log pc_i) / n_b, pc_i = clip(p[i, y_i], 1e-7, 1 - 1e-7); the other classes
                 add +-0 and have no gradient;  with D_i = w[y_i] (gamma (1 - pc_i)^(gamma - 1) log pc_i - (1 - pc_i)^gamma / pc_i)
                 inside the clip and 0 outside, and dp[i, y_i] / dz[i, j] = p[i, y_i] ([j == y_i] - p[i, j]):
                 grad[i, j] = D_i * p[i, y_i] * ([j == y_i] - p[i, j]) / n_b"""
    nb, c = logits.shape
    rows = np.arange(nb)
    d = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=1)
    p = e / s[:, None]
    hot = np.zeros((nb, c))
    hot[rows, y] = 1.0
    wy = w[y]
    if kind == LOSS_KINDS["ce"]:
        keep, smooth = 1.0 - label_smoothing, label_smoothing / c
        q = -(d - np.log(s)[:, None])
        big_a, big_g, big_u = (wy * q[rows, y]).sum(), (q * w[None, :]).sum(), wy.sum()
        loss = keep * (big_a / big_u) + smooth * (big_g / big_u)
        grad = (keep * (wy[:, None] * (p - hot)) + smooth * (w.sum() * p - w[None, :])) / big_u
    else:
        py = p[rows, y]
        pc = np.minimum(np.maximum(py, FOCAL_CLIP), 1.0 - FOCAL_CLIP)
        one, lp = 1.0 - pc, np.log(pc)
        fo = np.ones(nb) if gamma == 0 else one * one if gamma == 2 else np.power(one, gamma)
        df = np.zeros(nb) if gamma == 0 else 2.0 * one if gamma == 2 else gamma * np.power(one, gamma - 1.0)
        loss = ((wy * fo) * -lp).sum() / nb
        big_d = np.where((py >= FOCAL_CLIP) & (py <= 1.0 - FOCAL_CLIP), wy * (df * lp - fo / pc), 0.0)
        grad = ((big_d * py)[:, None] * (hot - p)) / nb
    return float(loss), grad


def mix_batch(x32: np.ndarray, y: np.ndarray, lam, index: np.ndarray):
    """mixup_data (net_trainer.py:595-604) on one batch of feature rows: x = lam * x + (1 - lam) * x[index] in float32, as torch
    computes it with its FloatTensor lam; the label is the argmax of the mixed one-hot rows, the first maximum of a tie."""
    lam = np.float32(lam)
    onem = np.float32(1.0) - lam
    x = lam * x32 + onem * x32[index]
    y2 = y[index]
    return x, np.where(lam > onem, y, np.where(lam < onem, y2, np.minimum(y, y2)))


def cosine_lr(lr: float, eta_min: float, t0: int, at: float) -> float:
    """CosineAnnealingWarmRestarts(T_0=t0, T_mult=1, eta_min).step(at): the rate behind it."""
    t_cur = at % t0 if at >= t0 else at
    return eta_min + (lr - eta_min) * (1.0 + math.cos(math.pi * t_cur / t0)) / 2.0


def head_fit_numpy(feats, targets, runs: Sequence[HeadRun], epochs: int, batch_size: int = 64, first_epoch: int = 1) -> list:
    """The specification of avcer_head_fit (include/avcer_hip.h) in numpy float64: per run a HeadFitRun.  feats [n, F] (read as
    float32, the features' format), targets [n] in [0, C).  Per iteration: the batch order[e, i * B : (i + 1) * B] (the last may
    be short), mixup if the run has it, logits = x W^T + b, the loss and its gradient (loss_and_grad), one Adam step with torch's
    formula, and the scheduler's rate for the next iteration (cosine_lr at first_epoch + e + i / iters).  ValueError before any
    work: shapes, targets outside [0, C), an order[e] that is no permutation of 0 .. n-1, a mix_index that is no permutation
    inside a batch, a mix_lam outside [0, 1], non-finite hyper-parameters.
    feats [V, n, F]: V views of the same n windows (augmented_views); epoch e of a run takes its rows, mixup partners included,
    from feats[run.view[e]] (default e % V) -- targets, order and the mixup tables do not change with the view.  A view outside
    0 .. V-1 raises ValueError.  [1, n, F] is [n, F]."""
    x_all = np.asarray(feats, dtype=np.float32)
    pk = _pack(x_all.shape, targets, runs, epochs, batch_size, first_epoch)
    x_views = x_all if pk.views is not None else x_all[None]
    y_all = pk.targets.astype(np.int64)
    out = []
    for k, r in enumerate(runs):
        kind, ls, gamma, lr0, beta1, beta2, eps, t0, eta_min, mix = pk.hyper[k, :10]
        cw = pk.class_w[k].astype(np.float64)
        w, b = pk.w0[k].astype(np.float64), pk.b0[k].astype(np.float64)
        mw, vw, mb, vb = np.zeros_like(w), np.zeros_like(w), np.zeros_like(b), np.zeros_like(b)
        w_hist, b_hist = np.zeros((pk.epochs,) + w.shape), np.zeros((pk.epochs,) + b.shape)
        batch_loss, epoch_loss = np.zeros((pk.epochs, pk.n_batches)), np.zeros(pk.epochs)
        lr, step = lr0, 0
        for e in range(pk.epochs):
            running = 0.0
            x_all = x_views[0 if pk.view is None else pk.view[k, e]]
            for i in range(pk.n_batches):
                rows = pk.order[k, e, i * pk.bsz:(i + 1) * pk.bsz].astype(np.int64)
                x32, y = x_all[rows], y_all[rows]
                if mix:
                    x32, y = mix_batch(x32, y, pk.mix_lam[k, e, i], pk.mix_index[k, e, i * pk.bsz:i * pk.bsz + rows.shape[0]].astype(np.int64))
                x = x32.astype(np.float64)
                loss, g = loss_and_grad(x @ w.T + b[None, :], y, int(kind), cw, ls, gamma)
                batch_loss[e, i] = loss
                running += loss * pk.bsz                     # net_trainer.py:441: the nominal size for the short batch too
                step += 1
                step_size = lr / (1.0 - beta1 ** step)
                bc2 = math.sqrt(1.0 - beta2 ** step)
                for p, m, v, grad in ((w, mw, vw, g.T @ x), (b, mb, vb, g.sum(axis=0))):
                    m += (1.0 - beta1) * (grad - m)
                    v *= beta2
                    v += (1.0 - beta2) * grad * grad
                    p -= step_size * (m / (np.sqrt(v) / bc2 + eps))
                lr = cosine_lr(lr0, eta_min, int(t0), first_epoch + e + i / pk.n_batches)
            w_hist[e], b_hist[e] = w, b
            epoch_loss[e] = running / pk.n_batches           # :460
        out.append(HeadFitRun(w_hist, b_hist, batch_loss, epoch_loss))
    return out


# ------------------------------------------------------------------------------------------------ the draws
def make_order(n: int, epochs: int, seed: int) -> np.ndarray:
    """int64 [epochs, n]: one permutation of the rows per epoch from numpy's Generator(PCG64(seed)) -- not torch's stream: these
    are not the batches DataLoader(shuffle=True) deals under torch.manual_seed(seed)."""
    if not _is_int(n, 1) or not _is_int(epochs, 1):
        raise ValueError(f"make_order: n and epochs must be integers >= 1, got {n!r}, {epochs!r}")
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.stack([rng.permutation(int(n)) for _ in range(int(epochs))]).astype(np.int64)


def make_mixup(n: int, epochs: int, batch_size: int, alpha: float, seed: int):
    """(mix_lam f32 [epochs, n_batches], mix_index int32 [epochs, n]): per batch lam ~ Beta(alpha, alpha) (1 for alpha <= 0, as
    mixup_data has it) and a permutation of the positions inside the batch, from numpy's Generator(PCG64(seed)) -- not the stream
    np.random.beta and torch.randperm draw from."""
    if not _is_int(n, 1) or not _is_int(epochs, 1) or not _is_int(batch_size, 1):
        raise ValueError(f"make_mixup: n, epochs and batch_size must be integers >= 1, got {n!r}, {epochs!r}, {batch_size!r}")
    if not math.isfinite(float(alpha)):
        raise ValueError(f"make_mixup: alpha must be finite, got {alpha!r}")
    rng = np.random.Generator(np.random.PCG64(seed))
    n, bsz = int(n), int(batch_size)
    n_batches = -(-n // bsz)
    lam = np.ones((epochs, n_batches), np.float32)
    index = np.zeros((epochs, n), np.int32)
    for e in range(int(epochs)):
        for i in range(n_batches):
            nb = min(bsz, n - i * bsz)
            if alpha > 0:
                lam[e, i] = rng.beta(alpha, alpha)
            index[e, i * bsz:i * bsz + nb] = rng.permutation(nb)
    return lam, index


# ------------------------------------------------------------------------------------------------ device calls
def augmented_views(engine, files, windows, views: int, spec, sr: int = 16000, max_w_len: int = 4, mode: Optional[int] = None,
                    windows_per_pass: int = 128):
    """The features of a training corpus under `views` draws of the waveform augmentation: f32 [views, n, F] on the device.  View
    v is audio_corpus.run_corpus(features=True, transform=spec with seed + v): the reference augments a window afresh every time
    it is dealt (train_c_audio.py:112-119); here an epoch picks one of V extracted views (HeadRun.view).  ValueError before any
    work: views < 1, a spec that is no augment.AugmentSpec, what run_corpus refuses."""
    import dataclasses

    import torch

    from . import audio_corpus, augment

    if isinstance(views, bool) or not isinstance(views, (int, np.integer)) or views < 1:
        raise ValueError(f"views must be an integer >= 1, got {views!r}")
    if not isinstance(spec, augment.AugmentSpec):
        raise ValueError(f"augmented_views: spec is an augment.AugmentSpec, got {type(spec).__name__}")
    plan = audio_corpus.plan_corpus(engine, files, windows, sr, max_w_len, windows_per_pass)
    return torch.stack([audio_corpus.run_corpus(engine, files, windows, sr, max_w_len, mode, windows_per_pass, features=True, plan=plan,
                                                transform=dataclasses.replace(spec, seed=int(spec.seed) + v)).features
                        for v in range(int(views))])


def fit_heads(engine, feats, targets, runs: Sequence[HeadRun], epochs: int, batch_size: int = 64, first_epoch: int = 1) -> HeadFit:
    """head_fit_numpy on the device, all runs in one launch (Engine.head_fit): feats [n, F] -- a device tensor, the `features` of
    audio_corpus.run_corpus, stays where it is --, targets [n] host integers.  The tables of the runs are checked on the host
    (ValueError as head_fit_numpy raises them, before anything is launched) and uploaded once.  Returns a HeadFit of device
    tensors; nothing synchronises with the host.  feats [V, n, F] and HeadRun.view: as head_fit_numpy takes them
    (avcer_head_fit_views; [n, F] goes through avcer_head_fit as before)."""
    pk = _pack(tuple(feats.shape), targets, runs, epochs, batch_size, first_epoch)
    w_hist, b_hist, batch_loss, epoch_loss = engine.head_fit(feats, pk.targets, pk.hyper, pk.class_w, pk.w0, pk.b0, pk.order,
                                                             pk.mix_lam, pk.mix_index, pk.epochs, pk.bsz, view=pk.view)
    return HeadFit(w_hist, b_hist, batch_loss, epoch_loss, int(first_epoch))


def select(engine, fit: HeadFit, dev_feats, dev_targets, c_names, metrics: Sequence[str] = ("recall", "precision", "f1", "accuracy"),
           kind: Optional[str] = "ce", weights=None, label_smoothing: float = 0.2, gamma: float = 0.0, batch_size: int = 64,
           phase: str = "devel"):
    """The devel phase of NetTrainer.run for every run and epoch of `fit`: ONE Engine.head_apply launch gives the logits of the
    devel features [m, F] under all K * epochs heads; per head validate.window_losses (`kind` None: the reference's 0.0),
    Engine.window_votes' softmax rows and validate.measures; per run validate.best_epoch with its strict `>`.
    Returns [(stats, best)] per run: stats = the rows validate.stats_csv takes, {"epoch", f"{phase}_loss", f"{phase}_{metric}"
    ...} with the trainer's epoch numbers (fit.first_epoch + e)."""
    metrics = tuple(metrics)
    unknown = [m for m in metrics if m not in validate.SCORES]
    if unknown or not metrics:
        raise ValueError(f"metric {unknown[0]!r}: one of {validate.SCORES}" if unknown else "select: no metric")
    k_runs, epochs, c, f = (int(v) for v in fit.w_hist.shape)
    if len(c_names) != c:
        raise ValueError(f"{len(c_names)} class names for heads of {c} classes")
    t = np.asarray(dev_targets).reshape(-1)
    if kind is not None:
        validate._check_loss(c, t, kind, weights, label_smoothing, gamma, batch_size)
    logits = engine.head_apply(dev_feats, fit.w_hist.reshape(k_runs * epochs, c, f), fit.b_hist.reshape(k_runs * epochs, c))
    m = int(logits.shape[1])
    out = []
    for r in range(k_runs):
        stats = []
        for e in range(epochs):
            lg = logits[r * epochs + e]
            lost = None if kind is None else validate.window_losses(engine, lg, t, kind, weights, label_smoothing, gamma, batch_size)
            probs = engine.window_votes(lg, t.astype(np.int32), [0, m])[0]
            perf = validate.measures(engine, t, probs, c_names, metrics)
            row = {"epoch": fit.first_epoch + e, f"{phase}_loss": 0.0 if lost is None else float(lost.epoch.item())}
            row.update({f"{phase}_{name}": perf[name] for name in metrics})
            stats.append(row)
        out.append((stats, validate.best_epoch(stats, phase, metrics)))
    return out


def write_checkpoint(base, w, b, epoch: int, path) -> str:
    """The trainer's checkpoint (net_trainer.py:273-285) {"epoch": epoch, "model_state_dict": ...} with feature_downsample.weight
    / .bias replaced by w [C, F] / b [C]: `base` is a state dict (bare or wrapped, as Engine.load_audio takes it) or the path
    of one; every other tensor is written as it is.  Engine.load_audio and validate.validate_checkpoints read the file unchanged.
    ValueError: a base without that layer or with a head of another shape."""
    import torch

    from .packing import _unwrap

    sd = dict(_unwrap(validate._state_dict(base)))
    def as_tensor(v):
        return v.detach().cpu() if hasattr(v, "detach") else torch.from_numpy(np.ascontiguousarray(v))

    w, b = as_tensor(w).to(torch.float32), as_tensor(b).to(torch.float32)
    if "feature_downsample.weight" not in sd or "feature_downsample.bias" not in sd:
        raise ValueError("write_checkpoint: the base has no feature_downsample layer")
    shapes = tuple(sd["feature_downsample.weight"].shape), tuple(sd["feature_downsample.bias"].shape)
    if (tuple(w.shape), tuple(b.shape)) != shapes:
        raise ValueError(f"write_checkpoint: a head of shapes {tuple(w.shape)}, {tuple(b.shape)} behind a base of {shapes[0]}, {shapes[1]}")
    sd["feature_downsample.weight"], sd["feature_downsample.bias"] = w.contiguous(), b.contiguous()
    sd = {k: (v if hasattr(v, "detach") else torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items()}
    path = os.fspath(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({"epoch": int(epoch), "model_state_dict": sd}, path)
    return path
