"""Fit the fusion weights: the reference's offline search (data/utils.py:115-209) with its inner loop on the GPU.

The tables of avcer_amd/fusion.py (WEIGHTS_AV_1, WEIGHTS_V_1, ...) are recorded outputs of three functions the reference drives
from get_pred_video.py:346-390 and get_pred_av.py:339-405 under np.random.seed(42):

  get_weights_prob_model   10 000 Dirichlet matrices [M, C], one weight per (model, class)      data/utils.py:138-163
  get_weights_v_model      a grid over a weight list for two models                             data/utils.py:166-185
  get_weights_av_model     the same for three models                                            data/utils.py:188-209

Each candidate is scored by get_metrics_for_fusion (:115-122): sklearn's classification_report on the argmax of the weighted sum,
of which the mean recall of classes 1..6 is the objective.  That report is a function of three integer vectors -- per class, how
often it was predicted (`pred`), how often rightly (`tp`), how often it is the label (`support`) -- so the search splits in two:
the counts of every candidate come from one kernel (Engine.weight_search_counts, csrc/search.hip), the metrics from
`metrics_from_counts` below in sklearn's own float64 expressions.  The result is the reference's bit for bit: the same metric
per candidate, the same first maximum, the same returned weights (tests/golden/weight_search.npz).

Arithmetic.  The kernel works in float64: tables and weights are converted on entry.  That is what numpy does with a float32
table and the float64 weights the reference's drivers pass (np.random.dirichlet, np.arange); a caller who hands the reference's
grid functions plain Python floats together with float32 tables gets float32 arithmetic there and is not mirrored here.

`counts_numpy` states the kernel in numpy for the tests and tools/weight_search_bench.py; like heatmaps.py it is a statement of
the arithmetic, not a CPU path of the product."""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

# candidate-frame pairs per launch: a launch of this size is tens of milliseconds of f64 work, well inside one GPU time slice
MAX_PAIRS_PER_LAUNCH = 1 << 32
MAX_CANDIDATES_PER_LAUNCH = 1 << 24  # include/avcer_hip.h AVCER_SEARCH_MAX_CANDIDATES
FUSION_CLASSES = range(1, 7)  # get_metrics_for_fusion sums classes 1..6: class 0 (and a 7th) sit in the report and in no sum


# --------------------------------------------------------------------------- candidates
def dirichlet_weights(num_weights: int, num_models: int, num_classes: int) -> np.ndarray:
    """[W, M, C] float64: the loop of data/utils.py:141-145, drawing from numpy's GLOBAL state exactly as the reference does --
    under np.random.seed(42) it consumes the same stream and returns the same candidates."""
    weights = np.zeros(shape=(num_weights, num_models, num_classes))
    for i in range(num_weights):
        weights[i] = np.random.dirichlet(alpha=np.ones((num_models,)), size=num_classes).T
    return weights


def grid_weights(values, num_models: int, num_classes: int = 1) -> np.ndarray:
    """[len(values) ** M, M, C] float64: the candidates of the reference's nested loops (data/utils.py:174-175, :197-199) in
    their iteration order -- the first model's weight is the outermost loop -- each scalar repeated over the classes."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if num_models < 1 or v.size < 1:
        raise ValueError(f"grid_weights: {v.size} values, {num_models} models")
    combos = np.array(list(itertools.product(v, repeat=num_models)), dtype=np.float64).reshape(-1, num_models)
    return np.ascontiguousarray(np.broadcast_to(combos[:, :, None], combos.shape + (num_classes,)))


# --------------------------------------------------------------------------- the kernel, stated in numpy
def _tables(ground_truth, predictions):
    preds = np.stack([np.asarray(p) for p in predictions]).astype(np.float64)
    labels = np.asarray(ground_truth).reshape(-1)
    if preds.ndim != 3 or labels.shape[0] != preds.shape[1]:
        raise ValueError(f"weight search: tables {preds.shape} (models, frames, classes) and {labels.shape[0]} labels disagree")
    return preds, labels.astype(np.int64)


def counts_numpy(preds, labels, weights):
    """(tp, pred) int32 [W, C]: data/utils.py:151-154 per candidate, in float64 with every product and every sum rounded on
    its own, np.argmax's first-maximum / first-NaN rule, then the two histograms the kernel accumulates."""
    preds = np.asarray(preds).astype(np.float64)
    weights = np.asarray(weights).astype(np.float64)
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    m, n, c = preds.shape
    if weights.ndim != 3 or weights.shape[1:] != (m, c) or labels.shape[0] != n:
        raise ValueError(f"counts_numpy: preds {preds.shape}, labels {labels.shape}, weights {weights.shape} disagree")
    tp = np.zeros((weights.shape[0], c), dtype=np.int32)
    pred = np.zeros((weights.shape[0], c), dtype=np.int32)
    for k in range(weights.shape[0]):
        f = preds[0] * weights[k, 0]
        for i in range(1, m):
            f += preds[i] * weights[k, i]
        am = np.argmax(f, axis=-1)
        pred[k] = np.bincount(am, minlength=c)
        tp[k] = np.bincount(am[am == labels], minlength=c)
    return tp, pred


# --------------------------------------------------------------------------- metrics
def metrics_from_counts(tp, pred, support):
    """sklearn's per-class report from integer counts, and get_metrics_for_fusion's triple (data/utils.py:115-122).
    tp, pred: [W, C] or [C]; support: the labels' histogram, [>= C] (a label class beyond the tables is allowed).
    Returns (precision, f1, recall, (mean_precision, mean_f1, uar)): the first three per class, float64 [..., K] with
    K = max(C, len(support), 7); the triple is the reference's running sum over classes 1..6 in order, divided by 6.
    sklearn 1.7 precision_recall_fscore_support: precision = tp / pred, recall = tp / support, f1 = 2 tp / (support + pred),
    each 0.0 where its denominator is 0.  A class of 1..6 that is neither a label nor predicted by a candidate is missing from
    that candidate's report: KeyError(str(cl)), as the reference's dict lookup raises (first candidate, first class)."""
    tp = np.asarray(tp, dtype=np.int64)
    pred = np.asarray(pred, dtype=np.int64)
    support = np.asarray(support, dtype=np.int64).reshape(-1)
    k = max(tp.shape[-1], support.shape[0], 7)

    def widen(a):
        out = np.zeros(a.shape[:-1] + (k,), dtype=np.int64)
        out[..., :a.shape[-1]] = a
        return out

    tp, pred, support = widen(tp), widen(pred), widen(support)
    absent = (pred[..., 1:7] == 0) & (support[1:7] == 0)
    if absent.any():
        raise KeyError(str(1 + int(np.argwhere(absent.reshape(-1, 6))[0][1])))

    def divide(num, den):
        den = np.broadcast_to(den, num.shape)
        out = num / np.where(den == 0, 1, den)
        out[den == 0] = 0.0
        return out

    precision = divide(tp, pred)
    recall = divide(tp, support)
    f1 = divide(2 * tp, support + pred)
    triple = []
    for per_class in (precision, f1, recall):
        acc = np.zeros(per_class.shape[:-1])
        for cl in FUSION_CLASSES:
            acc = acc + per_class[..., cl]
        triple.append(acc / 6)
    return precision, f1, recall, tuple(triple)


# --------------------------------------------------------------------------- search
@dataclass
class SearchResult:
    metric: np.ndarray        # float64 [W]: the reference's objective (its `uar`) per candidate, in candidate order
    best_index: int | None    # the first candidate whose metric exceeds every earlier one and 0; None: every metric is 0
    best_metric: float
    best_weights: np.ndarray | None  # weights[best_index], [M, C]
    tp: np.ndarray            # int32 [W, C]
    pred: np.ndarray          # int32 [W, C]


def device_counts(engine, preds, labels, weights, max_pairs: int | None = None):
    """Engine.weight_search_counts over all candidates, split into launches of at most `max_pairs` candidate-frame pairs (default MAX_PAIRS_PER_LAUNCH)
    (candidates are independent: the split changes nothing).  The tables go to the device once.  Returns numpy (tp, pred)."""
    import torch

    p = engine._dev(preds, torch.float64)
    lab = engine._dev(labels, torch.int32)
    weights = np.asarray(weights, dtype=np.float64)
    if p.dim() != 3 or weights.ndim != 3:
        raise ValueError(f"weight search: preds [M, N, C] and weights [W, M, C] expected, got {tuple(p.shape)}, {weights.shape}")
    max_pairs = MAX_PAIRS_PER_LAUNCH if max_pairs is None else int(max_pairs)
    step = max(1, min(MAX_CANDIDATES_PER_LAUNCH, max_pairs // max(1, int(p.shape[1]))))
    tps, preds_ = [], []
    for s in range(0, weights.shape[0], step):
        tp, pr = engine.weight_search_counts(p, lab, weights[s:s + step])
        tps.append(tp)
        preds_.append(pr)
    if not tps:
        raise ValueError("weight search: no candidates")
    return torch.cat(tps).cpu().numpy(), torch.cat(preds_).cpu().numpy()


def select(metric):
    """The reference's selection (data/utils.py:147-158): a strict `>` from 0, so the first maximum wins, a NaN never does,
    and nothing is selected when every metric is 0.  Returns (best_index or None, best_metric)."""
    metric = np.asarray(metric, dtype=np.float64)
    if metric.size == 0 or not (metric > 0).any():
        return None, 0.0
    i = int(np.argmax(np.where(metric > 0, metric, -np.inf)))
    return i, float(metric[i])


def result_from_counts(tp, pred, labels, weights) -> SearchResult:
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if labels.size and labels.min() < 0:
        raise ValueError("weight search: negative label")
    support = np.bincount(labels, minlength=7)
    metric = metrics_from_counts(tp, pred, support)[3][2]
    i, best = select(metric)
    return SearchResult(metric=metric, best_index=i, best_metric=best, best_weights=None if i is None else np.array(weights[i]),
                        tp=np.asarray(tp), pred=np.asarray(pred))


def search(engine, ground_truth, predictions, weights) -> SearchResult:
    """Score every candidate of `weights` [W, M, C] on the GPU and select as the reference does."""
    preds, labels = _tables(ground_truth, predictions)
    weights = np.asarray(weights, dtype=np.float64)
    tp, pred = device_counts(engine, preds, labels, weights)
    return result_from_counts(tp, pred, labels, weights)


# --------------------------------------------------------------------------- the reference's three functions
def get_weights_prob_model(engine, ground_truth, predictions, num_weights, num_classes):
    """data/utils.py:138-163: the best of `num_weights` Dirichlet matrices [M, C], or None when no candidate scores above 0."""
    weights = dirichlet_weights(num_weights, len(predictions), num_classes)
    return search(engine, ground_truth, predictions, weights).best_weights


def _grid_model(engine, weights, ground_truth, predictions, num_models):
    preds, _ = _tables(ground_truth, [np.array(p) for p in predictions[:num_models]])
    values = list(weights)
    r = search(engine, ground_truth, preds, grid_weights(values, num_models, preds.shape[2]))
    if r.best_index is None:
        return [0] * num_models
    idx = np.unravel_index(r.best_index, (len(values),) * num_models)
    return [values[i] for i in idx]


def get_weights_v_model(engine, weights, ground_truth, predictions):
    """data/utils.py:166-185: [w_static, w_dynamic] from the grid weights x weights, or [0, 0]."""
    return _grid_model(engine, weights, ground_truth, predictions, 2)


def get_weights_av_model(engine, weights, ground_truth, predictions):
    """data/utils.py:188-209: [w_static, w_dynamic, w_audio] from the grid weights^3, or [0, 0, 0]."""
    return _grid_model(engine, weights, ground_truth, predictions, 3)


# --------------------------------------------------------------------------- the figures of the fitted weights
WEIGHT_FIGURE_LABELS = (("VS", "VD", "A"), ("Ne", "An", "Di", "Fe", "Ha", "Sa", "Su", "Mo"))  # get_weights_matrices.py:20,43,66
# models, audio classes -> file stem, title, figsize in inches (100 pixels each), x_labels    (get_weights_matrices.py:18-72)
WEIGHT_FIGURES = {(2, None): ("weights1_video", "Weights for video modality fusion", (6, 4), False),
                  (3, 7): ("weights1_av_7", "Weights for audio (7cl) and video modality fusion", (6, 6), False),
                  (3, 8): ("weights1_av_8", "Weights for audio (8cl) and video modality fusion", (6, 6), True)}


def weight_figure_matrix(weights_1, weights_2) -> np.ndarray:
    """What get_weights_matrices.py plots: weights_1 [M, 7] (a row per model, as the searches return it) with weights_2 [M] as an
    eighth column "Mo" -- the script's 8 x M table, transposed as it transposes it."""
    w1, w2 = np.asarray(weights_1, dtype=np.float64), np.asarray(weights_2, dtype=np.float64).reshape(-1)
    if w1.ndim != 2 or w1.shape[1] != 7 or w2.shape[0] != w1.shape[0] or w1.shape[0] not in (2, 3):
        raise ValueError(f"weight figures: weights_1 [M, 7] and weights_2 [M] of M = 2 or 3 models, got {w1.shape} and {w2.shape}")
    return np.concatenate([w1, w2[:, None]], axis=1)


def write_weight_figures(engine, weights_1=None, weights_2=None, save_dir=".", audio_classes: int = 8, quality: int = 95,
                         subsampling: int = 2, entropy: str = "device"):
    """get_weights_matrices.py:18-70 through figures.write_weights_matrices: the figure of fitted weights -- `weights_1` [M, 7] and
    `weights_2` [M] as get_weights_prob_model and get_weights_v_model / get_weights_av_model return them -- under the script's
    labels, title, size and file stem for that model set: M = 2 "weights1_video" (600 x 400, no x labels), M = 3 "weights1_av_7"
    (600 x 600, no x labels) or, with audio_classes=8, "weights1_av_8" (600 x 600, x labels).  With both weights None: the
    script itself, its three figures from the tables on record in fusion.py (WEIGHTS_V_*, WEIGHTS_AV7_*, WEIGHTS_AV_*); the two
    600 x 600 figures share one draw call, the 600 x 400 one has its own.  The reference names its files `.pdf`; this project
    writes no PDF, so the stems are kept and the files are `.jpg`.  Returns the paths, in the script's order."""
    import os

    from . import figures, fusion

    if (weights_1 is None) != (weights_2 is None):
        raise ValueError("weight figures: weights_1 and weights_2 are given together, or neither")
    if weights_1 is None:
        sets = [(fusion.WEIGHTS_V_1, fusion.WEIGHTS_V_2, None), (fusion.WEIGHTS_AV7_1, fusion.WEIGHTS_AV7_2, 7),
                (fusion.WEIGHTS_AV_1, fusion.WEIGHTS_AV_2, 8)]
    else:
        sets = [(weights_1, weights_2, None if len(weights_2) == 2 else int(audio_classes))]
    jobs = []
    for w1, w2, cls in sets:
        m = weight_figure_matrix(w1, w2)
        if (len(m), cls) not in WEIGHT_FIGURES:
            raise ValueError(f"weight figures: audio_classes is 7 or 8, not {cls!r}")
        stem, title, (fw, fh), x_labels = WEIGHT_FIGURES[len(m), cls]
        jobs.append((m, os.path.join(os.fspath(save_dir), stem + ".jpg"), title, x_labels, (100 * fw, 100 * fh)))
    for size in sorted({j[4] for j in jobs}):
        group = [j for j in jobs if j[4] == size]
        labels = (WEIGHT_FIGURE_LABELS[0][:len(group[0][0])], WEIGHT_FIGURE_LABELS[1])
        if any(len(j[0]) != len(group[0][0]) for j in group):
            raise ValueError("weight figures: figures of one size share their row labels")
        figures.write_weights_matrices(engine, [j[0] for j in group], labels, [j[1] for j in group], [j[2] for j in group], size[0], size[1],
                                       True, [j[3] for j in group], None, quality, subsampling, entropy)
    return [j[1] for j in jobs]
