"""The shared cases of tests/test_chart_cpu.py and tests/test_gpu_chart.py: one statement of the lengths and the class tables at
which the chart's traces can go wrong, on a small picture, and the CPU reference of each, computed once and never written to."""
import numpy as np

from avcer_amd import chart

WIDTH, HEIGHT = 96, 64
TABLES = ("constant", "ramp", "alternating", "random")
_REF = {}


def plan(T, width=WIDTH, height=HEIGHT):
    return chart.chart_plan(T, width, height)


def lengths():
    """1 and 2 (a point, one segment), 7, the threshold between the two envelope paths and its neighbours, several frames per
    column with a remainder, and 1000."""
    pw = plan(1).pw
    return (1, 2, 7, pw - 1, pw, pw + 1, 3 * pw + 5, 1000)


def table(kind, T):
    """int32 [4, T], classes 0..6."""
    i = np.arange(T, dtype=np.int64)
    if kind == "constant":      # two series coincide: the thinning keeps both visible
        rows = [np.full(T, 3), np.full(T, 3), np.full(T, 0), np.full(T, 6)]
    elif kind == "ramp":        # over all seven classes: up, down, up with a 6 -> 0 drop, three times up
        up = (i * 7) // T if T >= 7 else i % 7
        rows = [up, 6 - up, (up + 3) % 7, ((i * 21) // T) % 7 if T >= 21 else (2 * i) % 7]
    elif kind == "alternating":  # 0 / 6 every frame: the longest segments there are, up and down
        rows = [(i % 2) * 6, (1 - i % 2) * 6, ((i // 2) % 2) * 6, (i % 2) * 6]
    elif kind == "random":
        rows = list(np.random.default_rng(T * 31 + 5).integers(0, 7, (4, T)))
    else:
        raise KeyError(kind)
    return np.stack(rows).astype(np.int32)


def reference(kind, T, width=WIDTH, height=HEIGHT):
    """(table, plan, what the four series paint: bool [4, height, width]) -- chart.series_numpy."""
    key = (kind, T, width, height)
    if key not in _REF:
        p, t = plan(T, width, height), table(kind, T)
        want = chart.series_numpy(t, p)
        for a in (t, want):
            a.setflags(write=False)
        _REF[key] = (t, p, want)
    return _REF[key]


def painted(series_mask):
    """bool [S, h, w] -> the picture before the decoration: uint8 [h, w, 3], white with the series in their colours."""
    pic = np.full(series_mask.shape[1:] + (3,), 255, dtype=np.uint8)
    for s, m in enumerate(series_mask):
        pic[m] = chart.COLOURS[s]
    return pic
