"""The cases of tests/test_figures_cpu.py: the matrices at which a matrix figure can go wrong, and their CPU statement computed
once."""
import functools

import numpy as np

from avcer_amd import evaluate, figures as fg

WEIGHT_LABELS = (["VS", "VD", "A"], ["Ne", "An", "Di", "Fe", "Ha", "Sa", "Su"])


def conf_edge():
    """7 x 7 counts: a row of one entry (the largest pct), a row that halves it exactly (a cell AT thresh, the minimum being 0), a
    row all zero, 2^31 - 1 beside a 1, 1999 of 2000 (99.95 before the 1e-10), and two ordinary rows."""
    cm = np.zeros((7, 7), dtype=np.int64)
    cm[0, 0] = 4
    cm[1, :2] = 2
    cm[3, 2], cm[3, 3] = 2 ** 31 - 1, 1
    cm[4, 4], cm[4, 5] = 1999, 1
    cm[5:] = np.random.default_rng(5).integers(0, 3000, (2, 7))
    shown = fg.shown_values(cm, "conf")
    assert shown[1, 0] == (shown.max() + shown.min()) / 2.0 and shown.min() == 0.0
    return cm


def conf_8():
    cm = np.random.default_rng(8).integers(0, 10 ** 9, (8, 8)).astype(np.int64)
    cm[0, 0], cm[7, 7], cm[3, 4] = fg.COUNT_MAX, 0, 7
    return cm


def weights(rows, cols, seed):
    w = np.random.default_rng(seed).random((rows, cols))
    w.reshape(-1)[:4] = (0.0, 1.0, 0.005, 0.995)
    return w


@functools.lru_cache(maxsize=None)
def mixed():
    """Five figures of mixed sizes and kinds, all 800 x 600: [(values, plan, statement)]."""
    out = []
    for values, kw in ((np.array([[5]], dtype=np.int64), dict(kind="conf", title="one cell")),
                       (conf_edge(), dict(kind="conf", labels=evaluate.EMO, title="Static video model. ABAW. UAR = 41.23%")),
                       (conf_8(), dict(kind="conf")),
                       (weights(3, 7, 3), dict(kind="weights", labels=WEIGHT_LABELS, title="Weights for audio and video fusion")),
                       (weights(16, 16, 16), dict(kind="weights", x_labels=False))):
        plan = fg.matrix_plan(values.shape[0], values.shape[1], **kw)
        pic = fg.matrix_numpy(values, plan)
        pic.setflags(write=False)
        out.append((values, plan, pic))
    return out


def text_of(glyphs):
    return "".join(fg.GLYPHS[g] for g, _, _ in glyphs)
