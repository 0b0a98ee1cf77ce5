"""The cases of tests/test_figures_items_cpu.py and tests/test_gpu_figures.py: the matrices and plans at which a figure drawn as an
annotate item list can differ from its statement, the smallest pictures a plan accepts, and the statements computed once."""
import functools

import numpy as np

from avcer_amd import evaluate, figures as fg

WIDEST_WEIGHT = -9999.99  # "-9999.99": the most characters cell_records writes for a weight


def accepts(rows, cols, kind, width, height, **kw):
    try:
        return fg.matrix_plan(rows, cols, kind, width, height, **kw)
    except ValueError:
        return None


def least(ok, hi):
    """The least v in 1..hi with ok(v), given ok(hi), by bisection: ok(v) holds and ok(v - 1) does not."""
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


@functools.lru_cache(maxsize=None)
def smallest_sizes(rows, cols, kind):
    """(width, height) pairs at the edge of what matrix_plan accepts for this grid: the least width at height 600, the least height
    at width 800 (where 800 x 600 is accepted at all) and the least height at width 16384 with the least width at that height.
    "Least" is a boundary the bisection finds: that size is accepted and one pixel less is refused (the font grows with the height,
    so acceptance is not monotone in it)."""
    out = []
    big = fg.chart.MAX_SIDE
    if accepts(rows, cols, kind, big, 600):
        out.append((least(lambda w: accepts(rows, cols, kind, w, 600) is not None, big), 600))
    if accepts(rows, cols, kind, 800, 600):
        out.append((800, least(lambda h: accepts(rows, cols, kind, 800, h) is not None, 600)))
    h = least(lambda h: accepts(rows, cols, kind, big, h) is not None, 600) if accepts(rows, cols, kind, big, 600) else None
    if h is not None:
        out.append((least(lambda w: accepts(rows, cols, kind, w, h) is not None, big), h))
    return tuple(dict.fromkeys(out))


def glyphs_outside(values, plan):
    """[(i, j)] of the cells whose text, placed where cell_records places it, leaves the cell: judged from the records and the
    glyph table alone, not through matrix_items."""
    _, table, _ = fg.glyph_atlas(plan.font)
    bad = []
    for c, (_, _, glyphs) in enumerate(fg.cell_records(values, plan)):
        i, j = divmod(c, plan.cols)
        x0, y0, x1, y1 = plan.cell(i, j)
        if any(x < x0 or y < y0 or x + int(table[g, 1]) - 1 > x1 or y + int(table[g, 2]) - 1 > y1 for g, x, y in glyphs):
            bad.append((i, j))
    return bad


def conf_extremes(rows, cols):
    """Count matrices that between them put every extreme text into every cell: ten digits everywhere; and per shift s a matrix
    whose row i holds its one count, of ten digits, in column (i + s) % cols, which reads "100.0%" there and "0" / "0.0%" elsewhere."""
    out = [np.full((rows, cols), fg.COUNT_MAX, dtype=np.int64)]
    for s in range(cols):
        m = np.zeros((rows, cols), dtype=np.int64)
        m[np.arange(rows), (np.arange(rows) + s) % cols] = fg.COUNT_MAX
        out.append(m)
    return out


def conf_7():
    """7 x 7 counts with a row of zeros (the + 1e-10 division), a count of ten digits, a row of one entry (100.0%) and ordinary
    rows."""
    cm = np.random.default_rng(7).integers(0, 5000, (7, 7)).astype(np.int64)
    cm[2] = 0
    cm[4, 4] = fg.COUNT_MAX
    cm[0] = 0
    cm[0, 0] = 4
    return cm


def weights_neg(rows, cols, seed):
    w = np.random.default_rng(seed).random((rows, cols))
    w.reshape(-1)[0] = -0.25
    w.reshape(-1)[-1] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> (values, plan, statement): a 7 x 7 "conf" and a 3 x 7 "weights" figure at 800 x 600, a 16 x 16 "weights" figure at
    800 x 600, and the same 16 x 16 grid at the smallest picture its plan accepts."""
    w16 = np.random.default_rng(16).random((16, 16))
    small = smallest_sizes(16, 16, "weights")[-1]
    cases = {"conf7": (conf_7(), fg.matrix_plan(7, 7, "conf", labels=evaluate.EMO, title="Audio-Video fusion. ABAW. UAR = 41.23%")),
             "w3x7": (weights_neg(3, 7, 3), fg.matrix_plan(3, 7, "weights", labels=(["VS", "VD", "A"], list("abcdefg")), title="Weights")),
             "w16": (w16, fg.matrix_plan(16, 16, "weights", x_labels=False)),
             "w16_small": (w16, fg.matrix_plan(16, 16, "weights", small[0], small[1]))}
    out = {}
    for name, (values, plan) in cases.items():
        pic = fg.matrix_numpy(values, plan)
        pic.setflags(write=False)
        out[name] = (values, plan, pic)
    return out


def pil_file(pic, quality=95, subsampling=2) -> bytes:
    import io

    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.asarray(pic)).save(b, "JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()
