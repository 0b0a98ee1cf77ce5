"""Shared by tests/test_evaluate_cpu.py and tests/test_gpu_evaluate.py: the synthetic dataset folder of tests/golden/eval_golden.npz
(tests/golden/make_eval_golden.py) written back to disk, and the jobs the host builds from it."""
from __future__ import annotations

import os

import numpy as np

from avcer_amd import evaluate as ev

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAIN = ("va", "vb", "vc")
AFEW = (("va.mp4", "Happy"), ("vb.avi", "Sad"), ("vc.mp4", "Angry"))
PATH_PREDS = ["video", "audio", "model"]
NAMES = {"av": ("stat", "dyn", "audio", "trues"), "video": ("stat", "dyn", "trues"), "audio": ("audio", "trues")}
TABLE_TOL = 1e-12   # the issue's bound: a plain against a compensated sum of <= ~10 values <= ~20 (2e-14), a few ulp in exp
METRIC_TOL = 1e-15


def load():
    return np.load(os.path.join(GOLDEN, "eval_golden.npz"))


def write_folder(g, root):
    for i, rel in enumerate(g["paths"]):
        path = os.path.join(root, str(rel))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(g[f"file_{i:03d}"].tobytes())
    return root


def jobs(root, videos=MAIN):
    """{golden prefix: (Job, output names)} for every modality and both corpora, plus the quirk video on its own."""
    ann = os.path.join(root, "ann")
    out = {}
    for modality in ev.MODALITIES:
        out[f"{modality}_abaw"] = (ev.abaw_job(ann, root, PATH_PREDS, [v + ".txt" for v in videos], modality), NAMES[modality])
        out[f"{modality}_afew"] = (ev.afew_job([a for a in AFEW if a[0][:-4] in videos], root, PATH_PREDS, modality), NAMES[modality])
    out["av_quirk"] = (ev.abaw_job(ann, root, PATH_PREDS, ["vq.txt"], "av"), NAMES["av"])
    return out


def check_tables(g, prefix, names, got):
    for name, t in zip(names, got):
        want = g[f"{prefix}_{name}"]
        t = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
        assert t.shape == want.shape, (prefix, name, t.shape, want.shape)
        if name == "trues":
            assert np.array_equal(t, want), (prefix, name)
        else:
            err = float(np.abs(t - want).max())
            print(f"{prefix}_{name}: max abs error {err:.3e}")
            assert err <= TABLE_TOL, (prefix, name, err)


def check_score(g, prefix, index, got):
    want_cm, want_m = g[f"{prefix}_cm"][index], g[f"{prefix}_metrics"][index]
    assert np.array_equal(got["cm"], want_cm), (prefix, index)
    have = np.array([got[k] for k in ("uar", "acc", "f1", "precision", "mean")])
    print(f"{prefix}[{index}] metrics: max abs error {float(np.abs(have - want_m).max()):.3e}")
    assert np.abs(have - want_m).max() <= METRIC_TOL, (prefix, index, have, want_m)
