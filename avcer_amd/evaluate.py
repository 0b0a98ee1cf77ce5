"""Score a dataset: the evaluation half of the reference's get_pred_av.py / get_pred_video.py / get_pred_audio.py.

    abaw_tables / afew_tables    get_abaw_pred / get_afew_pred of the three scripts (get_pred_av.py:77-195, get_pred_video.py:116-200,
                                 get_pred_audio.py:64-141): a folder of per-video CSV tables (io_formats.write_visual_csvs /
                                 write_audio_csv, what flag_save_prob leaves behind) becomes the `trues` / `preds_*` tables that
                                 weight_search.get_weights_* take
    score                        get_metrics (get_pred_av.py:19-45, get_pred_audio.py:17-34) with data/utils.py:130-135: UAR, accuracy,
                                 F1, precision, their mean and the confusion matrix of a model or a fusion

The host reads the CSV files, drops what the reference drops (`dropna`, the labels -1 and 7) and builds the index lists; everything
per row -- the per-frame group mean, the softmax, the selection, the tail repeat, the per-video mean, the weighted sum, the argmax
and the counting -- runs in libavcer_hip.so (csrc/evaluate.hip): one Engine.eval_tables call per model for the whole file list,
one Engine.eval_confusion call per score.  Nothing synchronises with the host before `score` fetches its 49 counts.

Where the reference is odd, so is this:
  * a kept position indexes the GROUP NUMBER of the audio table after `reset_index`, not the frame value (get_pred_av.py:105,116);
  * the static table is extended by the DYNAMIC table's deficit (get_pred_av.py:124-125): where the two CSV files of a video have
    different lengths, `preds_stat` comes out longer or shorter than `trues`, as it does there;
  * get_abaw_pred does not `dropna` the audio table, get_afew_pred does: in the first a NaN is skipped by the group mean
    (pandas' skipna), and a frame whose rows are all NaN stays a group, of NaN;
  * `groupby("frames")` orders the "%06d.jpg" strings; they are read as numbers here, the same order below 10^6 frames;
  * where the reference dies on `[-1]` of an empty selection this raises IndexError too when the host can see it (tables
    without keys); behind a group mean only the device knows the group count, and the rows come out NaN.

`evaluate_numpy` states both kernels in plain numpy float64 for the tests and tools/evaluate_bench.py; like
weight_search.counts_numpy it is a statement of the arithmetic, not a CPU path of the product."""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

EMO = ("Neutral", "Anger", "Disgust", "Fear", "Happiness", "Sadness", "Surprise")  # name_emo[:-1], the audio model's order
AFEW_AUDIO_ORDER = {"Angry": 1, "Disgust": 2, "Fear": 3, "Happy": 4, "Neutral": 0, "Sad": 5, "Surprise": 6}  # get_pred_av.py:145-153
AFEW_VIDEO_ORDER = {"Angry": 6, "Disgust": 5, "Fear": 4, "Happy": 1, "Neutral": 0, "Sad": 2, "Surprise": 3}  # get_pred_video.py:169-177
DROPPED_LABELS = (-1, 7)  # get_pred_av.py:107
MODALITIES = ("av", "video", "audio")
EVAL_COMPOUND, EVAL_CE_WEIGHTS, EVAL_CE_MASK = 1, 2, 4  # include/avcer_hip.h AVCER_EVAL_*
COMPOUND_PAIRS = ((3, 6), (4, 6), (5, 6), (2, 6), (1, 6), (3, 5), (1, 5))  # com_emo, get_pred_audio.py:202-210
COMPOUND_CLASS_WEIGHTS = {1: 5, 2: 6, 3: 5, 4: 6, 5: 4, 6: 2}  # dict_weights, :212-219


# --------------------------------------------------------------------------- what the host prepares
@dataclass
class Table:
    """One model's raw rows for a whole file list, and what becomes of them."""
    name: str                        # "stat", "dyn", "audio"
    rows: np.ndarray                 # float64 [R, c]
    row_counts: np.ndarray           # int64 [V]
    out_counts: np.ndarray           # int64 [V]: output rows per video
    softmax: bool
    keys: np.ndarray | None = None   # int32 [R]: the `frames` number of each row
    key_lo: np.ndarray | None = None     # int64 [V]
    key_spans: np.ndarray | None = None  # int64 [V]


@dataclass
class Job:
    tables: list
    trues: np.ndarray                # int32
    video_level: bool
    need: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))        # kept positions, all videos
    need_counts: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))


def _visual_rows(path: str, by_name: bool) -> np.ndarray:
    import pandas as pd

    df = pd.read_csv(path)
    return np.asarray((df[list(EMO)] if by_name else df).values, dtype=np.float64)


def _audio_rows(path: str, dropna: bool):
    """(rows [n, c], frame numbers [n]).  Rows without a frame name belong to no group (groupby drops a NaN key)."""
    import pandas as pd

    df = pd.read_csv(path)
    df = df.dropna() if dropna else df[df["frames"].notna()]
    cols = [c for c in EMO + ("Other",) if c in df.columns]
    keys = np.array([int(str(f).split(".")[0]) for f in df["frames"]], dtype=np.int64)
    return np.asarray(df[cols].values, dtype=np.float64).reshape(len(df), len(cols)), keys


def _stack(parts, width=None):
    if parts and any(p.shape[1] != parts[0].shape[1] for p in parts):
        raise ValueError("evaluate: tables of one model differ in their column count")
    return np.concatenate(parts) if parts else np.zeros((0, width or 7))


def _keyed_table(name, parts, keys, out_counts, softmax=True) -> Table:
    lo = np.array([int(k.min()) if len(k) else 0 for k in keys], dtype=np.int64)
    spans = np.array([int(k.max()) - int(k.min()) + 1 if len(k) else 0 for k in keys], dtype=np.int64)
    allk = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    if len(allk) and (allk.min() < 0 or allk.max() >= 2 ** 31):
        raise ValueError("evaluate: frame numbers must lie in 0 .. 2^31-1")
    return Table(name, _stack(parts), np.array([len(p) for p in parts], dtype=np.int64), np.asarray(out_counts, dtype=np.int64), softmax,
                 allk.astype(np.int32), lo, spans)


def _plain_table(name, parts, out_counts, softmax) -> Table:
    return Table(name, _stack(parts), np.array([len(p) for p in parts], dtype=np.int64), np.asarray(out_counts, dtype=np.int64), softmax)


def _paths(root, path_preds, modality):
    if modality not in MODALITIES:
        raise ValueError(f"evaluate: modality {modality!r}, expected one of {MODALITIES}")
    if isinstance(path_preds, (str, os.PathLike)):
        path_preds = [path_preds, path_preds, ""]
    root = root or ""
    return os.path.join(root, path_preds[0]), os.path.join(root, path_preds[1], path_preds[2])


def abaw_job(path_ann, root, path_preds, ann_files, modality="av") -> Job:
    """The host half of get_abaw_pred: parse, filter, index.  path_preds: [video folder, audio folder, audio model folder] under
    `root` as get_pred_av.py takes them, or one folder for a single modality."""
    import pandas as pd

    vdir, adir = _paths(root, path_preds, modality)
    stat, dyn, aud, akeys, needs, trues = [], [], [], [], [], []
    out = {"stat": [], "dyn": [], "audio": []}
    for ann in ann_files:
        labels = pd.read_csv(os.path.join(path_ann, ann))["Neutral"].values
        need = np.nonzero(~np.isin(labels, DROPPED_LABELS))[0]
        true = labels[need]
        needs.append(need)
        trues.append(true)
        if modality != "audio":
            s = _visual_rows(os.path.join(vdir, "static__" + ann[:-4]) + ".csv", True)
            d = _visual_rows(os.path.join(vdir, "dynamic__" + ann[:-4]) + ".csv", True)
            kept_s, kept_d = int(np.searchsorted(need, len(s))), int(np.searchsorted(need, len(d)))
            deficit = max(0, len(true) - kept_d)
            if deficit and (kept_s == 0 or kept_d == 0):
                raise IndexError("list index out of range")  # curr_pred_stat_df[-1], get_pred_av.py:122-123
            stat.append(s)
            dyn.append(d)
            out["stat"].append(kept_s + deficit)  # :124: the static table grows by the dynamic table's deficit
            out["dyn"].append(kept_d + deficit)
        if modality != "video":
            rows, keys = _audio_rows(os.path.join(adir, ann[:-4]) + ".csv", dropna=False)
            aud.append(rows)
            akeys.append(keys)
            out["audio"].append(len(true))
    tables = []
    if modality != "audio":
        tables += [_plain_table("stat", stat, out["stat"], False), _plain_table("dyn", dyn, out["dyn"], True)]
    if modality != "video":
        tables.append(_keyed_table("audio", aud, akeys, out["audio"]))
    return Job(tables, np.concatenate(trues).astype(np.int32) if trues else np.zeros(0, dtype=np.int32), False,
               np.concatenate(needs).astype(np.int64) if needs else np.zeros(0, dtype=np.int64),
               np.array([len(n) for n in needs], dtype=np.int64))


def afew_job(table, root, path_preds, modality="av") -> Job:
    """The host half of get_afew_pred.  table: (name_video, emotion) pairs, the file the reference reads from a fixed path
    (`name_video` with its extension, which is cut off as there)."""
    vdir, adir = _paths(root, path_preds, modality)
    order = AFEW_VIDEO_ORDER if modality == "video" else AFEW_AUDIO_ORDER
    stat, dyn, aud, akeys, trues = [], [], [], [], []
    for name, emotion in table:
        video = name[:-4]
        if modality != "audio":
            # get_pred_video.py:184-189 takes the columns as the file has them (the video models' order), get_pred_av.py:171-176 by name
            stat.append(_visual_rows(os.path.join(vdir, "static__" + video) + ".csv", modality == "av"))
            dyn.append(_visual_rows(os.path.join(vdir, "dynamic__" + video) + ".csv", modality == "av"))
        if modality != "video":
            rows, keys = _audio_rows(os.path.join(adir, video) + ".csv", dropna=True)
            aud.append(rows)
            akeys.append(keys)
        trues.append(order[emotion])
    ones = np.ones(len(trues), dtype=np.int64)
    tables = []
    if modality != "audio":
        tables += [_plain_table("stat", stat, ones, False), _plain_table("dyn", dyn, ones, True)]
    if modality != "video":
        tables.append(_keyed_table("audio", aud, akeys, ones))
    return Job(tables, np.array(trues, dtype=np.int32), True)


# --------------------------------------------------------------------------- device
def run_job(engine, job: Job):
    """One Engine.eval_tables launch sequence per model.  Returns (preds_stat, preds_dyn, preds_audio, trues), those the job has,
    float64 [N, 7] and int32 [N] tensors on the device."""
    import torch

    outs = [engine.eval_tables(t.rows, t.row_counts, job.need, job.need_counts, t.out_counts, t.softmax, job.video_level, t.keys,
                               t.key_lo, t.key_spans) for t in job.tables]
    return tuple(outs) + (torch.from_numpy(np.ascontiguousarray(job.trues)).to(engine.device, non_blocking=True),)


def abaw_tables(engine, path_ann, root, path_preds, ann_files, modality="av"):
    """get_abaw_pred: (preds_stat, preds_dyn, preds_audio, trues) for "av", (preds_stat, preds_dyn, trues) for "video",
    (preds_audio, trues) for "audio", one row per kept annotation frame of every file, as device tensors."""
    return run_job(engine, abaw_job(path_ann, root, path_preds, ann_files, modality))


def afew_tables(engine, table, root, path_preds, modality="av"):
    """get_afew_pred: the same tuple with one row per video, the mean of its frames' probabilities."""
    return run_job(engine, afew_job(table, root, path_preds, modality))


def metrics_from_cm(cm) -> dict:
    """data/utils.py:130-135 from a confusion matrix whose every label lies in 0..6: sklearn's recall_score / f1_score /
    precision_score(average="macro") and recall_score(average="micro").  Per class, as weight_search.metrics_from_counts states
    sklearn 1.7's precision_recall_fscore_support: recall = tp / support, precision = tp / pred, f1 = 2 tp / (support + pred),
    each 0.0 where its denominator is 0; the macro average runs over the classes that occur as a label or as a prediction."""
    cm = np.asarray(cm, dtype=np.int64)
    tp, support, pred = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    present = (support + pred) > 0

    def divide(num, den):
        out = num / np.where(den == 0, 1, den)
        out[den == 0] = 0.0
        return out[present]

    if not present.any():
        raise ValueError("evaluate: an empty confusion matrix has no metrics")
    uar = float(np.average(divide(tp, support)))
    precision = float(np.average(divide(tp, pred)))
    f1 = float(np.average(divide(2 * tp, support + pred)))
    acc = float(tp.sum() / support.sum())
    return {"uar": uar, "acc": acc, "f1": f1, "precision": precision, "mean": float(np.mean((uar, acc, f1, precision))), "cm": cm}


def _stacked(engine, predictions):
    import torch

    if isinstance(predictions, torch.Tensor) and predictions.dim() == 3:
        return predictions
    if isinstance(predictions, torch.Tensor) or (isinstance(predictions, np.ndarray) and predictions.ndim == 2):
        predictions = [predictions]  # get_pred_audio.get_metrics takes one table
    return torch.stack([engine._dev(p, torch.float64) for p in predictions])


def score(engine, trues, predictions, weights_1=None, weights_2=None, save_path=None, labels=None, title="") -> dict:
    """get_metrics: {"uar", "acc", "f1", "precision", "mean", "cm"} of the argmax of sum_i predictions[i] * weights_1[i] *
    weights_2[i] (one table without weights: get_pred_audio.get_metrics).  One Engine.eval_confusion launch; the 49 counts are
    the only thing fetched.  Labels outside 0..6 are in no cell of the matrix, and sklearn would average over their classes
    too: ValueError.
    save_path (a .jpg / .jpeg file; anything else is refused before any launch): the matrix is also drawn as the reference's
    plot_conf_matrix draws it (figures.write_conf_matrices; `labels`: the tick labels, None: EMO; `title`) and the path is
    out["plot_conf"].  None, the default: the figures module is not imported and the dict is the one above."""
    if save_path is not None:
        from . import figures

        save_path = figures.check_paths([save_path])[0]
    t = _stacked(engine, predictions)
    _, cm = engine.eval_confusion(t, trues, weights_1, weights_2, want_pred=False)
    cm = cm.cpu().numpy()
    if int(cm.sum()) != int(t.shape[1]):
        raise ValueError(f"score: {int(t.shape[1]) - int(cm.sum())} labels outside 0..6")
    out = metrics_from_cm(cm)
    if save_path is not None:
        out["plot_conf"] = figures.write_conf_matrices(engine, [out["cm"]], EMO if labels is None else labels, [save_path], [title])[0]
    return out


MODEL_STEMS = {"stat": "static", "dyn": "dynamic", "audio": "audio"}  # get_pred_video.py:66,81; "audio": see score_models
MODEL_TITLES = {"stat": "Static video model", "dyn": "Dynamic video model", "audio": "Audio model ()"}  # :64,79; get_pred_audio.py:40


def score_models(engine, trues, models: dict, weights_1=None, weights_2=None, save_dir=None, corpus: str = "ABAW", modality=None,
                 weight_type: str = "single", name_model: str = "", labels=None, **figure_options) -> dict:
    """The loop the get_metrics of get_pred_av.py / get_pred_video.py / get_pred_audio.py run: `models` is {"stat" / "dyn" /
    "audio": table [N, 7]} in the order of `weights_1` [M, 7] / `weights_2` [M].  Scored (`score`) are the fusion of all models --
    "fusion", left out when there is one model -- and every single model on its own, unweighted, as get_pred_video.py:55-83 does.
    Returns {"fusion": metrics, "stat": metrics, ...}.
    save_dir: every confusion matrix is drawn, ALL in one figures.write_conf_matrices call, and each metrics dict gets its
    "plot_conf".  The file names are the reference's with `.jpg` for its `.pdf` (this project writes no PDF), `modality`
    defaulting to "AV" / "V" / "A" by the models given:
      fusion       <corpus>_<modality>_sd_<weight_type>.jpg         "Audio-Video fusion. <corpus>. UAR = xx.xx%" (get_pred_av.py:52-53),
                                                                    without an audio model "Video fusion. ..." (get_pred_video.py:51-52)
      stat, dyn    <corpus>_<modality>_static_<weight_type>.jpg, ..._dynamic_...   "Static video model. ...", "Dynamic video model. ..."
      audio alone  <corpus>_<modality>_<name_model>.jpg             "Audio model (). ..." (get_pred_audio.py:40-42)
      audio beside visual models: <corpus>_<modality>_audio_<weight_type>.jpg -- get_pred_av.py draws the fusion only; the
                   single models are scored and drawn here in the video script's manner.
    `figure_options` (width, height, colorbar, font, quality, subsampling, entropy) go to write_conf_matrices.  A bad option is
    refused before anything is scored."""
    unknown = [k for k in models if k not in MODEL_STEMS]
    if unknown or not models:
        raise ValueError(f"score_models: models are keyed by {tuple(MODEL_STEMS)}, not {unknown[0]!r}" if unknown else "score_models: no model")
    names = list(models)
    if save_dir is not None:
        from . import figures

        bad = [k for k in figure_options if k not in ("width", "height", "colorbar", "font", "quality", "subsampling", "entropy")]
        if bad:
            raise ValueError(f"score_models: unknown figure option {bad[0]!r}")
    elif figure_options:
        raise ValueError("score_models: figure options without save_dir")
    if modality is None:
        modality = "A" if names == ["audio"] else "AV" if "audio" in names else "V"
    out, stems, titles = {}, {}, {}
    if len(names) > 1:
        out["fusion"] = score(engine, trues, [models[k] for k in names], weights_1, weights_2)
        stems["fusion"] = f"{corpus}_{modality}_sd_{weight_type}"
        titles["fusion"] = "Audio-Video fusion" if "audio" in names else "Video fusion"
    for k in names:
        out[k] = score(engine, trues, [models[k]])
        stems[k] = f"{corpus}_{modality}_{name_model}" if len(names) == 1 and k == "audio" else f"{corpus}_{modality}_{MODEL_STEMS[k]}_{weight_type}"
        titles[k] = MODEL_TITLES[k]
    if save_dir is not None:
        paths = [os.path.join(os.fspath(save_dir), stems[k] + ".jpg") for k in out]
        heads = ["{0}. {1}. UAR = {2:.2f}%".format(titles[k], corpus, out[k]["uar"] * 100) for k in out]
        figures.write_conf_matrices(engine, [out[k]["cm"] for k in out], EMO if labels is None else labels, paths, heads, **figure_options)
        for k, path in zip(out, paths):
            out[k]["plot_conf"] = path
    return out


# --------------------------------------------------------------------------- the kernels, stated in numpy
def _softmax(matrix):
    exp_matrix = np.exp(matrix - np.max(matrix, axis=1, keepdims=True))  # data/utils.py:125-127
    return exp_matrix / np.sum(exp_matrix, axis=1, keepdims=True)


def _group_means(rows, keys):
    """groupby(key).mean(): ascending distinct keys, NaN skipped per column, each group's rows added in file order."""
    if not len(keys):
        return np.full((0, 7), np.nan)
    order = np.argsort(keys, kind="stable")
    k, x = np.asarray(keys)[order], rows[order]
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    ok = ~np.isnan(x)
    n = np.add.reduceat(ok.astype(np.int64), starts, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, np.add.reduceat(np.where(ok, x, 0.0), starts, axis=0) / np.where(n > 0, n, 1), np.nan)


def tables_numpy(rows, row_counts, need, need_counts, out_counts, softmax, video_level=False, keys=None, key_lo=None, key_spans=None):
    """avcer_eval_tables (include/avcer_hip.h), video by video as the reference's loop goes."""
    rows = np.asarray(rows, dtype=np.float64)[:, :7]
    r_off = np.concatenate([[0], np.cumsum(row_counts)]).astype(np.int64)
    n_off = np.concatenate([[0], np.cumsum(need_counts)]).astype(np.int64) if not video_level else None
    out = []
    for v in range(len(row_counts)):
        x = rows[r_off[v]:r_off[v + 1]]
        if keys is not None:
            k = np.asarray(keys)[r_off[v]:r_off[v + 1]].astype(np.int64)
            inside = (k >= key_lo[v]) & (k < key_lo[v] + key_spans[v])
            x = _group_means(x[inside], k[inside])
        if softmax and len(x):
            with np.errstate(invalid="ignore"):
                x = _softmax(x)
        if video_level:
            out.append(np.mean(x, axis=0, keepdims=True) if len(x) else np.full((1, 7), np.nan))
            continue
        nd = np.asarray(need)[n_off[v]:n_off[v + 1]]
        nd = nd[nd < len(x)]
        target = int(out_counts[v])
        if not len(nd):
            out.append(np.full((target, 7), np.nan))
            continue
        out.append(x[nd[np.minimum(np.arange(target), len(nd) - 1)]])
    return np.concatenate(out) if out else np.zeros((0, 7))


def compound_numpy(pred, ce_weights_type, ce_mask):
    """get_compound_expression (data/utils.py:222-241) with the audio order's pairs and class weights."""
    prob = np.zeros((len(pred), 7))
    for idx, (i1, i2) in enumerate(COMPOUND_PAIRS):
        w_1 = w_2 = 1
        if ce_weights_type:
            s_w = COMPOUND_CLASS_WEIGHTS[i1] + COMPOUND_CLASS_WEIGHTS[i2]
            w_1, w_2 = COMPOUND_CLASS_WEIGHTS[i1] / s_w, COMPOUND_CLASS_WEIGHTS[i2] / s_w
        if ce_mask:
            pred = np.where(pred > 1 / 7, pred, 0)
        prob[:, idx] = pred[:, i1] * w_1 + pred[:, i2] * w_2
    return prob


def confusion_numpy(tables, labels=None, weights_1=None, weights_2=None, compound=0):
    """avcer_eval_confusion: (pred int32 [N], cm int64 [7, 7] or None)."""
    t = np.asarray(tables, dtype=np.float64)
    m = t.shape[0]
    w1 = np.ones((m, 7)) if weights_1 is None else np.asarray(weights_1, dtype=np.float64)
    w2 = np.ones(m) if weights_2 is None else np.asarray(weights_2, dtype=np.float64)
    f = t[0] * w1[0] * w2[0]  # get_pred_av.py:35-38
    for i in range(1, m):
        f += t[i] * w1[i] * w2[i]
    if compound & EVAL_COMPOUND:
        f = compound_numpy(f, bool(compound & EVAL_CE_WEIGHTS), bool(compound & EVAL_CE_MASK))
    pred = np.argmax(f, axis=-1).astype(np.int32)
    cm = None
    if labels is not None:
        lab = np.asarray(labels).reshape(-1).astype(np.int64)
        ok = (lab >= 0) & (lab < 7)
        cm = np.zeros((7, 7), dtype=np.int64)
        np.add.at(cm, (lab[ok], pred[ok]), 1)
    return pred, cm


def job_numpy(job: Job):
    """run_job on the CPU: the same tuple as numpy arrays."""
    return tuple(tables_numpy(t.rows, t.row_counts, job.need, job.need_counts, t.out_counts, t.softmax, job.video_level, t.keys,
                              t.key_lo, t.key_spans) for t in job.tables) + (job.trues,)


def score_numpy(trues, predictions, weights_1=None, weights_2=None) -> dict:
    return metrics_from_cm(confusion_numpy(np.stack([np.asarray(p, dtype=np.float64) for p in predictions]), trues, weights_1, weights_2)[1])


class NumpyEngine:
    """The two Engine entries answered by the numpy statements above, on CPU tensors: what the CPU tests hand to run_job, score and
    io_formats.dataset_fusion_audio in an Engine's place.  Never chosen by the product."""
    device = "cpu"

    @staticmethod
    def _dev(t, dtype):
        import torch

        return (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))).to(dtype=dtype).contiguous()

    def eval_tables(self, rows, row_counts, need, need_counts, out_counts, softmax, video_level=False, keys=None, key_lo=None,
                    key_spans=None, out=None):
        import torch

        return torch.from_numpy(tables_numpy(np.asarray(rows), row_counts, need, need_counts, out_counts, softmax, video_level, keys, key_lo,
                                             key_spans))

    def eval_confusion(self, tables, labels=None, weights_1=None, weights_2=None, compound=0, want_pred=True, want_cm=True, pred=None,
                       cm=None):
        import torch

        pred, cm = confusion_numpy(np.asarray(tables), None if labels is None else np.asarray(labels), weights_1, weights_2, compound)
        return torch.from_numpy(pred), None if cm is None else torch.from_numpy(cm)


evaluate_numpy = SimpleNamespace(engine=NumpyEngine, tables=tables_numpy, confusion=confusion_numpy, compound=compound_numpy, job=job_numpy, score=score_numpy)
