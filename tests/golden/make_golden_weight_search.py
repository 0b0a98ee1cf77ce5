#!/usr/bin/env python3
"""Generate tests/golden/weight_search.npz by running the REFERENCE's unmodified get_weights_prob_model, get_weights_v_model and
get_weights_av_model (data/utils.py:138-209) under np.random.seed(42), on CPU, with sklearn's classification_report.

Run in the build container only (`python tests/golden/make_golden_weight_search.py`), like make_golden.py, whose stubs it
reuses (that file is unchanged).  Inputs come from avcer_amd/synth.py fusion_tables, so only results are stored.  The
reference's get_metrics_for_fusion is wrapped by a recorder that calls the original and notes, per call and in call order, the
objective it returned and the histogram of the argmax it was given; the arithmetic is untouched.  Stored per case: `metric`
float64 [W], `hist` (the argmax histogram of every candidate) [W, C], the returned weights, and the case's parameters.  The
archive is written with fixed member timestamps, so a second run gives the same bytes.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository root and the reference on sys.path)

from avcer_amd import synth  # noqa: E402

C = 7
GRID = np.arange(0.01, 0.5, 0.05)  # get_pred_av.py:354
# name -> (function, seed of the tables, frames, models, classes the labels are drawn from, Dirichlet candidates)
CASES = {
    "prob_m2": ("prob", 101, 600, 2, 7, 300),
    "prob_m3": ("prob", 102, 3000, 3, 7, 2000),
    "prob_m3_label7": ("prob", 103, 400, 3, 8, 500),   # labels include class 7: in the report, in no sum
    "prob_m2_tie": ("prob", 132, 200, 2, 7, 300),      # the best metric is shared by two candidates: the first wins
    "grid_v": ("v", 104, 300, 2, 7, 0),                # 10^2 candidates, three share the best metric
    "grid_av": ("av", 105, 250, 3, 7, 0),              # 10^3 candidates, two share the best metric
}


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy's own writer stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    mg.install_stubs()
    import data.utils as du

    calls = []
    original = du.get_metrics_for_fusion

    def recorder(true, pred):
        out = original(true, pred)
        calls.append((out[2], np.bincount(np.asarray(pred), minlength=C)))
        return out

    du.get_metrics_for_fusion = recorder
    out = {"grid": GRID}
    for name, (kind, seed, n, m, label_classes, w) in CASES.items():
        labels, tables = synth.fusion_tables(seed, n, m, C, label_classes)
        calls.clear()
        np.random.seed(42)
        if kind == "prob":
            best = du.get_weights_prob_model(labels, list(tables), w, C)
        elif kind == "v":
            best = du.get_weights_v_model(GRID, labels, list(tables))
        else:
            best = du.get_weights_av_model(GRID, labels, list(tables))
        metric = np.array([c[0] for c in calls], dtype=np.float64)
        hist = np.stack([c[1] for c in calls])
        assert hist.max() < 32768 and hist.shape[1] == C
        out[f"{name}_params"] = np.array([seed, n, m, label_classes, len(calls)], dtype=np.int64)
        out[f"{name}_metric"] = metric
        out[f"{name}_hist"] = hist.astype(np.int16)
        out[f"{name}_best"] = np.asarray(best, dtype=np.float64)
        first = int(np.argmax(metric))
        print(name, "candidates", len(calls), "best", metric.max(), "at", first, "candidates sharing it", int((metric == metric.max()).sum()),
              "distinct metrics", len(np.unique(metric)))
    path = os.path.join(HERE, "weight_search.npz")
    save_npz(path, out)
    print("size", os.path.getsize(path))


if __name__ == "__main__":
    main()
