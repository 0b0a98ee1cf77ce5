"""Records tests/golden/validate.npz: what the reference's own loss/loss.py and utils/accuracy_utils.py (with torch, sklearn and
pandas) give on seeded inputs.  Run once, where the reference project is at hand:

    python tests/golden/make_validate_golden.py <reference>/src/audio

The two modules are imported from there and called; nothing of them is copied.  Recorded, per class count C in (7, 8):
  logits f32 [130, C], targets, weights (train_c_audio.py's max(counts) / counts as float32), batch size 64
  ce_batch / ce_row        torch.nn.CrossEntropyLoss(weight, label_smoothing) on float64 copies, per DataLoader batch
                           (reduction="mean") and per row (reduction="none"), for label_smoothing 0.2 and 0
  focal_batch / focal_row  SoftFocalLossWrapper(SoftFocalLoss(alpha=weight, gamma), C) the same way (a row: a batch of one),
                           for gamma 0 and 2
  probs, m_targets         softmax rows and targets in which the last class is never a target and class 1 neither a target nor
                           a prediction; recall / precision / f1 / accuracy (average="macro") and conf_matrix of accuracy_utils
and once: ccc_score on two series, v_score / a_score / va_score on two [n, t, 2] tables, and the bytes of
pd.DataFrame(rows).to_csv(sep=";", index=False) for a three-epoch table (net_trainer.py:319-334) with a NaN in it."""
import importlib.util
import io
import os
import sys

import numpy as np


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root):
    import pandas as pd
    import torch

    loss = _load(os.path.join(root, "loss", "loss.py"), "ref_loss")
    acc = _load(os.path.join(root, "utils", "accuracy_utils.py"), "ref_accuracy_utils")
    out = {}
    for c in (7, 8):
        rng = np.random.default_rng(c)
        n, bsz = 130, 64
        logits = (rng.standard_normal((n, c)) * 2).astype(np.float32)
        targets = rng.integers(0, c, n)
        counts = rng.integers(40, 900, c)
        weights = torch.Tensor(max(counts) / counts)                      # train_c_audio.py:240: float32
        x, y, w = torch.from_numpy(logits).double(), torch.from_numpy(targets), weights.double()
        out[f"logits{c}"], out[f"targets{c}"], out[f"weights{c}"], out[f"counts{c}"] = logits, targets, weights.numpy(), counts
        for eps in (0.2, 0.0):
            ce = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps)
            out[f"ce_batch{c}_{eps}"] = np.array([ce(x[i:i + bsz], y[i:i + bsz]).item() for i in range(0, n, bsz)])
            out[f"ce_row{c}_{eps}"] = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps, reduction="none")(x, y).numpy()
        for gamma in (0.0, 2.0):
            fl = loss.SoftFocalLossWrapper(loss.SoftFocalLoss(alpha=w, gamma=gamma), num_classes=c)
            out[f"focal_batch{c}_{gamma}"] = np.array([fl(x[i:i + bsz], y[i:i + bsz]).item() for i in range(0, n, bsz)])
            out[f"focal_row{c}_{gamma}"] = np.array([fl(x[i:i + 1], y[i:i + 1]).item() for i in range(n)])
        m_logits = (rng.standard_normal((200, c)) * 2).astype(np.float32)
        m_logits[:, 1] = -30.0                                            # class 1 is never predicted
        probs = torch.softmax(torch.from_numpy(m_logits), dim=-1).numpy()
        m_targets = rng.integers(2, c - 1, 200)                           # classes 0, 1 and the last are never targets
        out[f"probs{c}"], out[f"m_targets{c}"] = probs, m_targets
        for fn in (acc.recall, acc.precision, acc.f1, acc.accuracy):
            out[f"{fn.__name__}{c}"] = np.float64(fn(m_targets, probs, average="macro"))
        out[f"conf_matrix{c}"] = acc.conf_matrix(m_targets, probs, [str(k) for k in range(c)])
    rng = np.random.default_rng(99)
    t, p = rng.uniform(-1, 1, 300), rng.uniform(-1, 1, 300)
    p = 0.6 * t + 0.4 * p + 0.1
    out["ccc_t"], out["ccc_p"], out["ccc"] = t, p, np.float64(acc.ccc_score(t, p))
    vt, vp = rng.uniform(-1, 1, (20, 5, 2)), rng.uniform(-1, 1, (20, 5, 2))
    vp = 0.5 * vt + 0.5 * vp
    out["va_t"], out["va_p"] = vt, vp
    out["v_score"], out["a_score"], out["va_score"] = (np.float64(f(vt, vp)) for f in (acc.v_score, acc.a_score, acc.va_score))
    rows = [{"epoch": 1, "devel_loss": 2.3908523559570312, "devel_recall": 0.125, "devel_precision": float("nan"), "devel_f1": 1e-05},
            {"epoch": 2, "devel_loss": 0.1 + 0.2, "devel_recall": 1.0 / 3.0, "devel_precision": 0.5, "devel_f1": 0.4},
            {"epoch": 10, "devel_loss": 12345.678, "devel_recall": 1.0 / 3.0, "devel_precision": 1.0, "devel_f1": 0.0}]
    buf = io.StringIO()
    pd.DataFrame(rows).to_csv(buf, sep=";", index=False)
    out["stats_csv"] = np.frombuffer(buf.getvalue().encode(), dtype=np.uint8)
    out["stats_cols"] = np.array(list(rows[0]))
    out["stats_values"] = np.array([[float(r[k]) for k in rows[0]] for r in rows])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "validate.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
