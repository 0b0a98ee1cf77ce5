"""Validate audio checkpoints on a labelled corpus: the validation half of the reference's NetTrainer.

    class_weights                train_c_audio.py:236-242: max(counts) / counts as float32
    window_losses                the loss bookkeeping of NetTrainer.iterate_model (net_trainer.py:391-465) over
                                 torch.nn.CrossEntropyLoss(weight, label_smoothing) or the SoftFocalLoss of loss/loss.py:125-137
                                 behind its one-hot wrapper: per row, per DataLoader batch, per epoch
    ccc / v_score / a_score / va_score   utils/accuracy_utils.py:124-223
    measures                     NetTrainer.calc_metrics (net_trainer.py:537-572) over accuracy_utils' recall / precision / f1 /
                                 accuracy (sklearn, average="macro", zero_division=nan) and conf_matrix
    validate_checkpoints         the devel / test phase of NetTrainer.run (net_trainer.py:198-335) for a list of saved epochs: the
                                 corpus pass, the loss, the measures, stats.csv, the best epoch and its confusion figure

Everything per window runs in libavcer_hip.so.  The logits stay where audio_corpus.run_corpus left them: ONE avcer_window_losses
launch (csrc/losses.hip) gives the row, batch and epoch losses in float64, the confusion matrix is counted by the
avcer_eval_confusion launch evaluate.score uses, and the host turns its C x C counts into sklearn's figures.  One host
synchronisation per checkpoint behind the corpus pass: the fetch of the counts and of the two epoch figures.

Where the reference is odd, so is this:
  * the epoch loss is sum_b(loss_b * batch_size) / n_batches: the short last batch is multiplied by the full batch size too
    (net_trainer.py:441,460).  `Losses.epoch` is that figure; `Losses.mean`, the row-weighted mean, is what it was meant to be;
  * with class weights the batch loss of the cross entropy divides by the batch's sum of target weights, as torch's
    reduction="mean" does, so a batch's loss is not the mean of its row losses;
  * the best epoch starts from a score of 0 and moves on a strict `>`: of two equal scores the first epoch stays, and a run
    that never scores above 0 has the best epoch 0;
  * a macro average runs over the classes that occur as a target or as a prediction, and leaves out those whose own figure is
    undefined (a recall without targets, a precision without predictions): sklearn's zero_division=nan.

`losses_numpy` and `ccc_numpy` state the two kernels in numpy float64, in the kernels' own order of additions, for the tests and
tools/validate_bench.py; they are statements of the arithmetic, not a CPU path of the product."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import evaluate
from .audio_corpus import majority_voting, plan_corpus, run_corpus, votes_numpy

LOSS_KINDS = {"ce": 0, "soft_focal": 1}   # include/avcer_hip.h AVCER_LOSS_CE, AVCER_LOSS_SOFT_FOCAL
LOSS_MAX_CLASSES = 16                     # AVCER_LOSS_MAX_CLASSES
FOLD = 256                                # threads of a block of csrc/losses.hip: the shape of every sum
SCORES = ("recall", "precision", "f1", "accuracy")   # what a stats.csv column can hold
MEASURES = SCORES + ("conf_matrix",)
FOCAL_CLIP = 1e-7                         # loss.py:130
C_NAMES = {7: evaluate.EMO, 8: evaluate.EMO + ("Other",)}


class Losses(NamedTuple):
    """row f64 [n], batch f64 [ceil(n / batch_size)], epoch: the reference's epoch loss, mean: the row-weighted mean of the batch
    losses.  numpy values from losses_numpy, device tensors (epoch and mean 0-d) from window_losses."""
    row: object
    batch: object
    epoch: object
    mean: object


def class_weights(counts) -> np.ndarray:
    """train_c_audio.py:236-242: the class weights of the trainer's loss from the train set's label counts,
    float32(max(counts) / counts)."""
    counts = np.asarray(counts)
    if counts.ndim != 1 or counts.size < 1 or not (counts > 0).all():
        raise ValueError(f"class_weights: one positive count per class, got {counts!r}")
    return (counts.max() / counts).astype(np.float32)


def _check_loss(c: int, targets, kind, weights, label_smoothing, gamma, batch_size):
    """What both loss calls refuse, before any work: (kind number, targets int32 [n], weights float32 [c] or None)."""
    if kind not in LOSS_KINDS:
        raise ValueError(f"loss {kind!r}: one of {tuple(LOSS_KINDS)}")
    if not 2 <= c <= LOSS_MAX_CLASSES:
        raise ValueError(f"{c} classes: the losses take 2 .. {LOSS_MAX_CLASSES}")
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1], got {label_smoothing!r}")
    if not 0.0 <= float(gamma) < float("inf"):
        raise ValueError(f"gamma must be a finite number >= 0, got {gamma!r}")
    t = np.asarray(targets).reshape(-1)
    if t.size == 0:
        raise ValueError("no windows: a loss needs at least one")
    if not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() >= c:
        unlabelled = " (-1: an unlabelled window, -2: a corpus without labels)" if t.min() < 0 else ""
        raise ValueError(f"a loss needs every target in [0, {c}), got {t.dtype} in [{t.min()}, {t.max()}]{unlabelled}")
    w = None
    if weights is not None:
        w = weights.detach().cpu().numpy() if hasattr(weights, "detach") else np.asarray(weights)
        w = w.astype(np.float32).reshape(-1)
        if w.shape[0] != c:
            raise ValueError(f"{w.shape[0]} class weights for {c} classes")
    return LOSS_KINDS[kind], t.astype(np.int32), w


# ------------------------------------------------------------------------------------------------ the kernels, stated in numpy
def _fold(values: np.ndarray) -> np.ndarray:
    """block_fold of csrc/losses.hip over the last axis: thread t of 256 adds its items t, t + 256, .. one after the other from
    0.0, the partial sums fold in halves.  An item that is not there adds 0.0 here, which changes no bit of a sum that began at 0.0."""
    m = values.shape[-1]
    rounds = max(1, -(-m // FOLD))
    grid = np.zeros(values.shape[:-1] + (rounds * FOLD,))
    grid[..., :m] = values
    grid = grid.reshape(values.shape[:-1] + (rounds, FOLD))
    acc = np.zeros(values.shape[:-1] + (FOLD,))
    for r in range(rounds):
        acc = acc + grid[..., r, :]
    d = FOLD // 2
    while d >= 1:
        acc = acc[..., :d] + acc[..., d:2 * d]
        d //= 2
    return acc[..., 0]


def _by_batch(values: np.ndarray, n_batches: int, width: int) -> np.ndarray:
    out = np.zeros(n_batches * width)
    out[:values.shape[0]] = values
    return out.reshape(n_batches, width)


def losses_numpy(logits, targets, kind: str = "ce", weights=None, label_smoothing: float = 0.2, gamma: float = 0.0,
                 batch_size: int = 64) -> Losses:
    """avcer_window_losses (include/avcer_hip.h) in numpy float64, operation by operation and sum by sum in the kernel's order;
    numpy's exp and log and the device's may differ in the last place.  logits [n, c], targets [n] in [0, c), weights [c] or
    None.  ValueError as validate_checkpoints raises them."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    if x.ndim != 2:
        raise ValueError(f"logits [n, c] expected, got {x.shape}")
    n, c = x.shape
    k, y, w = _check_loss(c, targets, kind, weights, label_smoothing, gamma, batch_size)
    if y.shape[0] != n:
        raise ValueError(f"{n} rows of logits and {y.shape[0]} targets")
    w = np.ones(c) if w is None else w.astype(np.float64)
    keep, smooth = 1.0 - float(label_smoothing), float(label_smoothing) / float(c)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        d = x - x.max(axis=1, keepdims=True)
        e = np.exp(d)
        s = e[:, 0].copy()
        for j in range(1, c):
            s = s + e[:, j]
        wy = w[y]
        if k == LOSS_KINDS["ce"]:
            l = np.log(s)
            q = -(d - l[:, None])
            a = wy * q[rows, y]
            g = w[0] * q[:, 0]
            for j in range(1, c):
                g = g + w[j] * q[:, j]
            row = keep * a + smooth * g
        else:
            p = np.minimum(np.maximum(e[rows, y] / s, FOCAL_CLIP), 1.0 - FOCAL_CLIP)
            one = 1.0 - p
            f = np.ones(n) if gamma == 0 else one * one if gamma == 2 else np.power(one, float(gamma))
            a = (wy * f) * -np.log(p)
            g = np.zeros(n)
            row = a
        bsz = int(batch_size)
        n_batches = -(-n // bsz)
        width = min(bsz, n)
        sizes = np.minimum(n, (np.arange(n_batches) + 1) * bsz) - np.arange(n_batches) * bsz
        big_a, big_g, big_u = (_fold(_by_batch(v, n_batches, width)) for v in (a, g, wy))
        if k == LOSS_KINDS["ce"]:
            batch = keep * (big_a / big_u) + smooth * (big_g / big_u)
        else:
            batch = big_a / sizes.astype(np.float64)
        epoch = _fold(batch * float(bsz)) / float(n_batches)
        mean = _fold(batch * sizes.astype(np.float64)) / float(n)
    return Losses(row, batch, float(epoch), float(mean))


def ccc_numpy(targets, predicts) -> float:
    """avcer_ccc (include/avcer_hip.h) in numpy float64, its sums in the kernel's order: accuracy_utils.ccc_score
    (accuracy_utils.py:124-152).  A constant series gives 0 / 0 = NaN as there."""
    t = np.asarray(targets, dtype=np.float64).reshape(-1)
    p = np.asarray(predicts, dtype=np.float64).reshape(-1)
    if t.shape != p.shape or t.size < 1:
        raise ValueError(f"ccc: two series of one length >= 1, got {t.size} and {p.size}")
    n = float(t.size)
    with np.errstate(all="ignore"):
        mt, mp = _fold(t) / n, _fold(p) / n
        vy, vx = t - mt, p - mp
        sxy, sxx, syy = _fold(vx * vy), _fold(vx * vx), _fold(vy * vy)
        cor = sxy / (np.sqrt(sxx) * np.sqrt(syy))
        sdt, sdp = np.sqrt(syy / n), np.sqrt(sxx / n)
        return float(((2.0 * cor) * sdt) * sdp / ((sdt * sdt + sdp * sdp) + (mt - mp) * (mt - mp)))


# ------------------------------------------------------------------------------------------------ device calls
def window_losses(engine, logits, targets, kind: str = "ce", weights=None, label_smoothing: float = 0.2, gamma: float = 0.0,
                  batch_size: int = 64) -> Losses:
    """The losses of a corpus's window logits in one launch (Engine.window_losses): logits [n, c] -- a device tensor stays where
    it is --, targets [n] host integers in [0, c), weights [c] or None.  The `Losses` hold device tensors; nothing synchronises
    with the host.  ValueError, before anything is launched: what validate_checkpoints lists."""
    if len(logits.shape) != 2:
        raise ValueError(f"logits [n, c] expected, got {tuple(logits.shape)}")
    n, c = int(logits.shape[0]), int(logits.shape[1])
    k, y, w = _check_loss(c, targets, kind, weights, label_smoothing, gamma, batch_size)
    if y.shape[0] != n:
        raise ValueError(f"{n} rows of logits and {y.shape[0]} targets")
    row, batch, epoch = engine.window_losses(logits, y, w, k, float(label_smoothing), float(gamma), int(batch_size))
    return Losses(row, batch, epoch[0], epoch[1])


def ccc(engine, targets, predicts):
    """accuracy_utils.ccc_score on the device (Engine.ccc): a float64 [1] device tensor."""
    return engine.ccc(targets, predicts)


def _va_column(engine, table, j: int):
    import torch

    t = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.stack(table) if isinstance(table, list) else np.asarray(table))
    if t.dim() != 3 or t.shape[2] != 2:
        raise ValueError(f"a valence / arousal table is [n, t, 2], got {tuple(t.shape)}")
    return t.to(device=engine.device, dtype=torch.float64).contiguous()[:, :, j].reshape(-1)   # a view: every second element


def v_score(engine, targets, predicts):
    """accuracy_utils.v_score: the CCC of column 0 of two [n, t, 2] tables, read in place with stride 2."""
    return engine.ccc(_va_column(engine, targets, 0), _va_column(engine, predicts, 0))


def a_score(engine, targets, predicts):
    """accuracy_utils.a_score: column 1."""
    return engine.ccc(_va_column(engine, targets, 1), _va_column(engine, predicts, 1))


def va_score(engine, targets, predicts):
    """accuracy_utils.va_score: 0.5 * (v_score + a_score)."""
    return 0.5 * (v_score(engine, targets, predicts) + a_score(engine, targets, predicts))


# ------------------------------------------------------------------------------------------------ measures
def confusion(engine, targets, probs, c: int) -> np.ndarray:
    """accuracy_utils.conf_matrix: the counts of (target, argmax of the row of `probs`) as int64 [c, c], counted by
    Engine.eval_confusion, the launch behind evaluate.score.  That launch takes rows of 7 columns and labels 0 .. 6:
      c <= 7   the rows are widened to 7 columns with -inf, which no argmax picks: one launch on the float64 rows;
      c == 8   the argmax is taken by Engine.window_votes on the float32 rows (the first maximum, as np.argmax), and the classes
               are counted in two blocks of 7: four launches on one-hot rows, a row counting in the block pair it falls in.
    Targets outside [0, c) are refused: sklearn would average over their classes too."""
    import torch

    t = np.asarray(targets).reshape(-1)
    if t.size == 0:
        raise ValueError("measures: no rows")
    if not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() >= c:
        raise ValueError(f"measures: every target must lie in [0, {c}), got {t.dtype} in [{t.min()}, {t.max()}]")
    p = probs if isinstance(probs, torch.Tensor) else torch.as_tensor(np.asarray(probs))
    if p.dim() != 2 or int(p.shape[1]) != c or int(p.shape[0]) != t.size:
        raise ValueError(f"measures: {t.size} targets and rows {tuple(p.shape)} for {c} classes")
    if not 2 <= c <= 8:
        raise ValueError(f"measures: {c} classes, 2 .. 8 are counted")
    lab = engine._dev(t.astype(np.int32), torch.int32)
    if c <= 7:
        rows = engine._dev(p, torch.float64)
        if c < 7:
            rows = torch.cat([rows, torch.full((t.size, 7 - c), -np.inf, dtype=torch.float64, device=rows.device)], dim=1)
        _, cm = engine.eval_confusion(rows[None], lab, want_pred=False)
        return cm.cpu().numpy()[:c, :c].astype(np.int64)
    pred = engine.window_votes(engine._dev(p, torch.float32), lab, [0, t.size])[1].to(torch.int64)
    cells = torch.arange(7, device=pred.device)
    blocks = []
    for a in (0, 7):
        for b in (0, 7):
            inside = (lab >= a) & (lab < a + 7) & (pred >= b) & (pred < b + 7)
            onehot = ((pred - b)[:, None] == cells[None, :]).to(torch.float64)
            blocks.append(engine.eval_confusion(onehot[None], torch.where(inside, lab - a, torch.full_like(lab, -1)), want_pred=False)[1])
    blocks = torch.stack(blocks).cpu().numpy().astype(np.int64)
    cm = np.zeros((14, 14), dtype=np.int64)
    cm[:7, :7], cm[:7, 7:], cm[7:, :7], cm[7:, 7:] = blocks
    return cm[:c, :c]


def measures_from_cm(cm, metrics: Sequence[str] = MEASURES) -> dict:
    """calc_metrics from the confusion matrix, each figure as sklearn 1.7's precision_recall_fscore_support(average="macro",
    zero_division=nan) and accuracy_score give it: per class recall = tp / targets, precision = tp / predictions, f1 = 2 tp /
    (targets + predictions), NaN where the denominator is 0; the macro average is np.nanmean over the classes that occur as a
    target or as a prediction (NaN when every one of them is NaN); accuracy = hits / rows."""
    cm = np.asarray(cm, dtype=np.int64)
    unknown = [m for m in metrics if m not in MEASURES]
    if unknown:
        raise ValueError(f"metric {unknown[0]!r}: one of {MEASURES}")
    tp, support, pred = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    present = (support + pred) > 0

    def macro(num, den):
        with np.errstate(all="ignore"):
            v = np.where(den == 0, np.nan, num / np.where(den == 0, 1, den))[present]
        return float("nan") if v.size == 0 or np.isnan(v).all() else float(np.nanmean(v))

    values = {"recall": lambda: macro(tp.astype(np.float64), support.astype(np.float64)),
              "precision": lambda: macro(tp.astype(np.float64), pred.astype(np.float64)),
              "f1": lambda: macro(2.0 * tp.astype(np.float64), support.astype(np.float64) + pred.astype(np.float64)),
              "accuracy": lambda: float(tp.sum() / cm.sum()) if cm.sum() else float("nan"),
              "conf_matrix": lambda: cm}
    return {m: values[m]() for m in metrics}


def measures(engine, targets, probs, c_names, metrics: Sequence[str] = MEASURES) -> dict:
    """NetTrainer.calc_metrics with accuracy_utils' functions: {name: value} for `metrics` in the caller's order, the names being
    the functions' `__name__`s -- "recall" (the UAR), "precision", "f1" (macro, zero_division=nan), "accuracy", "conf_matrix"
    (int64 [c, c], c = len(c_names)).  targets [n] host integers in [0, c), probs [n, c] (a device tensor stays where it is): the
    predicted class is the first maximum of a row (proba_to_class_num).  The counting runs on the device (`confusion`)."""
    unknown = [m for m in metrics if m not in MEASURES]
    if unknown:
        raise ValueError(f"metric {unknown[0]!r}: one of {MEASURES}")
    return measures_from_cm(confusion(engine, targets, probs, len(c_names)), metrics)


# ------------------------------------------------------------------------------------------------ the table and the best epoch
def best_epoch(stats: Sequence[dict], phase: str, metrics: Sequence[str]) -> dict:
    """max_perf[phase] of NetTrainer.run (net_trainer.py:189-247): {"epoch": 0, "performance": {first metric: 0}} until an epoch's
    first metric is above the best so far (strict `>`: of equal scores the first epoch stays, a NaN never wins); then that
    epoch and all its metrics."""
    main = metrics[0]
    best = {"epoch": 0, "performance": {main: 0}}
    for row in stats:
        if row[f"{phase}_{main}"] > best["performance"][main]:
            best = {"epoch": row["epoch"], "performance": {m: row[f"{phase}_{m}"] for m in metrics}}
    return best


def _cell(v) -> str:
    if isinstance(v, (bool, np.bool_)):
        return str(bool(v))
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    v = float(v)
    return "" if v != v else repr(v)


def stats_csv(stats: Sequence[dict]) -> bytes:
    """`pd.DataFrame(stats).to_csv(sep=";", index=False)` (net_trainer.py:319-334) for rows of one key order, as bytes: the
    header, then one line per epoch; an integer as it is, a float by its shortest repr, a NaN as an empty cell."""
    if not stats:
        raise ValueError("stats_csv: no rows")
    cols = list(stats[0])
    if any(list(r) != cols for r in stats):
        raise ValueError("stats rows must hold the same keys in the same order")
    ints = {c: all(isinstance(r[c], (int, np.integer)) and not isinstance(r[c], (bool, np.bool_)) for r in stats) for c in cols}
    lines = [";".join(cols)] + [";".join(_cell(r[c] if ints[c] else float(r[c])) for c in cols) for r in stats]
    return ("\n".join(lines) + "\n").encode()


def _state_dict(entry):
    """A checkpoint as Engine.load_audio takes it: a state dict (bare or the trainer's {"model_state_dict": ...}) or the path of
    an `epoch_N.pth` file."""
    if isinstance(entry, (str, os.PathLike)):
        import torch

        return torch.load(os.fspath(entry), map_location="cpu", weights_only=False)
    return entry


def _classes(sd) -> int:
    from .packing import _unwrap

    return int(_unwrap(sd)["feature_downsample.weight"].shape[0])


def validate_checkpoints(engine, checkpoints, files, windows, phase: str = "devel", loss: Optional[str] = "ce", weights=None,
                         label_smoothing: float = 0.2, gamma: float = 0.0, batch_size: int = 64,
                         metrics: Sequence[str] = ("recall", "precision", "f1", "accuracy"), group: Optional[str] = None,
                         log_dir=None, save_figures: bool = False, max_tokens: Optional[int] = None, c_names=None, sr: int = 16000,
                         max_w_len: int = 4, mode: Optional[int] = None, windows_per_pass: int = 128, figure_dir=None):
    """The validation phase of NetTrainer.run for saved epochs.  checkpoints: [(epoch, state dict or path of epoch_N.pth)];
    files, windows: the labelled corpus as audio_corpus.run_corpus takes it (`sr`, `max_w_len`, `mode`, `windows_per_pass` too).
    Per checkpoint: Engine.load_audio (`max_tokens` as there), ONE run_corpus over the set -- planned once, the waveforms uploaded
    once --, window_losses on its logits (`loss`: "ce" with `label_smoothing`, "soft_focal" with `gamma`, None: no loss, the
    column holds the reference's 0.0; `weights`: class_weights(...) or None) and `measures` on its probabilities; with
    group="majority" the scores are per FILE, on what audio_corpus.majority_voting returns (group_predicts_fn), the loss stays
    per window as in the reference.
    Returns (stats, best): stats = [{"epoch", f"{phase}_loss", f"{phase}_{metric}" ...}] in the order of `checkpoints`, the loss
    being the reference's epoch loss (Losses.epoch); best = best_epoch(stats, phase, metrics).
    log_dir: stats.csv is written there (stats_csv).  save_figures: the confusion matrix of every epoch that improved the best
    score is drawn (figures.write_conf_matrices, all in one call behind the loop) as `epoch_{e}_{phase}_{score}.jpg` -- the
    reference's name with .jpg for its .svg -- titled "Confusion Matrix. {phase}. UAR = {:.3f}%", into `figure_dir` (default:
    log_dir); the paths come back as best["figures"].  c_names: the class names (default: the 7 or 8 of the audio models).
    ValueError before any launch: a target outside [0, C) when a loss is asked for (-1, an unlabelled window, is refused by
    name), an empty window set, batch_size < 1, an unknown loss, metric or group, weights whose length is not C, no checkpoints,
    save_figures without a directory; and whatever plan_corpus refuses."""
    import torch

    checkpoints = list(checkpoints)
    metrics = tuple(metrics)
    if not checkpoints:
        raise ValueError("validate_checkpoints: no checkpoints")
    if loss is not None and loss not in LOSS_KINDS:
        raise ValueError(f"loss {loss!r}: one of {tuple(LOSS_KINDS)} or None")
    unknown = [m for m in metrics if m not in SCORES]
    if unknown or not metrics:
        raise ValueError(f"metric {unknown[0]!r}: one of {SCORES}" if unknown else "validate_checkpoints: no metric")
    if group not in (None, "majority"):
        raise ValueError(f"group {group!r}: None or \"majority\"")
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")
    figure_dir = log_dir if figure_dir is None else figure_dir
    if save_figures and figure_dir is None:
        raise ValueError("save_figures needs log_dir or figure_dir")
    all_targets = np.concatenate([np.asarray(t.expr).reshape(-1) for t in windows]) if len(windows) else np.zeros(0, np.int64)
    if all_targets.size == 0:
        raise ValueError("validate_checkpoints: the window set is empty")
    first = _state_dict(checkpoints[0][1])
    c = _classes(first)
    names = tuple(c_names) if c_names is not None else C_NAMES.get(c, tuple(str(k) for k in range(c)))
    if len(names) != c:
        raise ValueError(f"{len(names)} class names for a model of {c} classes")
    if loss is not None:
        _check_loss(c, all_targets, loss, weights, label_smoothing, gamma, batch_size)
    elif weights is not None and len(weights) != c:
        raise ValueError(f"{len(weights)} class weights for {c} classes")

    load = {} if max_tokens is None else {"max_tokens": max_tokens}
    on_device = []
    for entry in files:   # uploaded once: run_corpus takes device tensors as they are
        wav = entry[1]
        wav = wav if torch.is_tensor(wav) else torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32) if len(entry) == 2 or entry[2] is None
                                                                 else np.ascontiguousarray(wav))
        on_device.append((entry[0], wav.to(engine.device)) + tuple(entry[2:]))
    stats, plan, figures_due = [], None, []
    top = 0
    for k, (epoch, entry) in enumerate(checkpoints):
        sd = first if k == 0 else _state_dict(entry)
        if _classes(sd) != c:
            raise ValueError(f"epoch {epoch}: a model of {_classes(sd)} classes behind one of {c}")
        engine.load_audio(sd, **load)
        if plan is None:
            plan = plan_corpus(engine, on_device, windows, sr, max_w_len, windows_per_pass)
        res = run_corpus(engine, on_device, windows, sr, max_w_len, mode, windows_per_pass, plan=plan)
        lost = None if loss is None else window_losses(engine, res.logits, res.targets, loss, weights, label_smoothing, gamma, batch_size)
        if group == "majority":
            t, p, _ = majority_voting(engine, res.logits, res.targets, res.file_off, names=res.names)
            perf = measures(engine, np.asarray(t, dtype=np.int64), np.stack(p), names, metrics + ("conf_matrix",))
        else:
            perf = measures(engine, res.targets, res.probs, names, metrics + ("conf_matrix",))
        cm = perf.pop("conf_matrix")
        row = {"epoch": epoch, f"{phase}_loss": 0.0 if lost is None else float(lost.epoch.item())}
        row.update({f"{phase}_{m}": perf[m] for m in metrics})
        stats.append(row)
        score = perf[metrics[0]]
        if score > top:
            top = score
            if save_figures:
                figures_due.append((cm, os.path.join(os.fspath(figure_dir), f"epoch_{epoch}_{phase}_{score}.jpg"),
                                    "Confusion Matrix. {0}. UAR = {1:.3f}%".format(phase, score * 100)))
    best = best_epoch(stats, phase, metrics)
    if log_dir is not None:
        os.makedirs(os.fspath(log_dir), exist_ok=True)
        with open(os.path.join(os.fspath(log_dir), "stats.csv"), "wb") as f:
            f.write(stats_csv(stats))
    if save_figures:
        from . import figures

        best["figures"] = figures.write_conf_matrices(engine, [f[0] for f in figures_due], list(names), [f[1] for f in figures_due],
                                                      [f[2] for f in figures_due]) if figures_due else []
    return stats, best


# ------------------------------------------------------------------------------------------------ the CPU stand-in of the tests
class NumpyEngine(evaluate.NumpyEngine):
    """The Engine entries this module calls, answered by the numpy statements on CPU tensors: what the CPU tests hand to
    `measures`, `window_losses` and `ccc` in an Engine's place.  Never chosen by the product."""

    def window_votes(self, logits, targets, file_off, out=None):
        import torch

        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in votes_numpy(np.asarray(logits), np.asarray(targets), file_off))

    def window_losses(self, logits, targets, weights=None, kind=0, label_smoothing=0.2, gamma=0.0, batch_size=64):
        import torch

        name = {v: k for k, v in LOSS_KINDS.items()}[kind]
        out = losses_numpy(np.asarray(logits), np.asarray(targets), name, weights, label_smoothing, gamma, batch_size)
        return torch.from_numpy(out.row), torch.from_numpy(out.batch), torch.tensor([out.epoch, out.mean], dtype=torch.float64)

    def ccc(self, targets, predicts):
        import torch

        return torch.tensor([ccc_numpy(np.asarray(targets), np.asarray(predicts))], dtype=torch.float64)
