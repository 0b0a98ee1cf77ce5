"""The matrix figures of the evaluation scripts (visualization/visualize.py:10-172): `plot_conf_matrix`, which every get_metrics of
get_pred_video.py / get_pred_av.py / get_pred_audio.py ends in, and `plot_weights_matrix` of get_weights_matrices.py -- a grid of
coloured cells with their numbers written into them, a colour bar, tick labels, captions and a title.

The CPU STATEMENT of those figures: the plan (`matrix_plan`), the numbers as text (`round_scaled`, `fixed`), the colours
(`lut_index`, `BLUES`), the per-cell records (`cell_records`) and the picture (`paint_numpy`, `matrix_numpy`).  It is what the
device path is held to, bit for bit, as chart.chart_numpy is for the timeline chart.

The DEVICE PATH has no kernel of its own ("Matrix figures").  Everything a figure consists of is an item
kind of annotate.draw -- a cell and a colour band are FILL items, a glyph is a MASK item -- so a figure is an item list built on
the host (`matrix_items`: the text is formatted on the host, from counts `evaluate.score` has there anyway) in front of the
existing avcer_annotate_frames, followed by the existing JPEG encoder: `render` draws a batch, `write_conf_matrices` /
`write_weights_matrices` write the files, and only file bytes cross to the host.

The reference plots with matplotlib and saves `.pdf`.  Two identities are claimed, both at tolerance zero: with PIL for
everything drawn (`ImageDraw.rectangle` per cell and colour band, `ImageDraw.bitmap` of the font's masks per glyph and label),
and with matplotlib for the CELL COLOURS only -- `imshow(cmap=Blues)` under `set_clim(0, 100)` / `set_clim(0, 1)`
(tests/test_figures_cpu.py).  Agg's text, matplotlib's layout, `tight_layout` and the PDF output are not reproduced.  The
reference writes every cell's text twice (visualize.py:42-51 and :59-68) at the same place; without anti-aliasing the second
covers the first entirely, so only the second is drawn.

Values.  "conf": int64 counts cm [rows, cols]; a cell shows `pct = cm.astype(float64) / (cm.sum(axis=1)[:, None] + 1e-10) * 100`
in exactly that order (visualize.py:32) and the text "{count}\\n{pct:.1f}%".  "weights": float64 values, the cell shows the value
itself and the text "{v:.2f}".  Text is white where the shown value > thresh = (max + min) / 2 over the figure, else black.

Colour (matplotlib 3.10 Normalize + Colormap.__call__ on floats): t = (v - 0) / (vmax - 0), xa = t * 256; xa == 256 -> 255,
xa < 0 -> 0, xa >= 256 -> 255, else the truncation of xa; the colour is row xa of `BLUES`
(matplotlib.cm.Blues(np.arange(256), bytes=True)[:, :3], also tests/golden/blues_lut.npy).

Decimals (`round_scaled`).  "{x:.kf}" is the correctly rounded decimal of the binary double, ties to even on the EXACT value.  With
p = 10^k (exact in binary64), hi = x * p and lo = fma(x, p, -hi), x * p = hi + lo exactly.  n = floor(hi), t = (hi - n) - 0.5 (exact
where it can be zero); the result is n + 1 when t > 0, or t == 0 and lo > 0, or t == 0 and lo == 0 and n is odd; else n.  |lo| is at
most half an ulp of hi and t a multiple of that ulp, so lo decides only at t == 0.  The digits are those of the integer.

Geometry (`matrix_plan`), integers only.  The plot rectangle (x0, y0, pw, ph) lies inside margins sized by the text; cell (i, j) is
columns x0 + (j * pw) // cols .. x0 + ((j + 1) * pw) // cols - 1 and rows y0 + (i * ph) // rows .. likewise, so the cells tile the
rectangle.  A text line is the glyphs "0123456789.%-" of the font, each its own mask, side by side at their advances
(`glyph_atlas`); the line box is `line_h` rows high; a line is centred in its cell: x = cx0 + ((cw - line width) >> 1); the block
of one line ("weights") or of two lines `gap` rows apart ("conf") at y = cy0 + ((ch - block height) >> 1).  A glyph pixel outside
its own cell is not drawn.  The colour bar is 256 bands, bottom to top: band k holds the rows r = e(k) .. e(k + 1) - 1 counted
from the bar's lowest row, e(k) = (k * bh) // 256.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from . import annotate as an
from . import chart

KINDS = {"conf": 0, "weights": 1}
MAX_DIM = 16               # rows and columns of a figure
MAX_GLYPHS = 17            # the longest cell text: 10 digits over "100.0%", or a sign and "9999.99"
COUNT_MAX = 9_999_999_999  # 10 digits
WEIGHT_MAX = 999_999       # |v| rounded to hundredths: "-9999.99"
GLYPHS = "0123456789.%-"
G_POINT, G_PERCENT, G_MINUS = 10, 11, 12
CAPTIONS = {"conf": ("True label", "Predicted label"), "weights": ("Model", "Weights of emotions and models")}
CLIM = {"conf": 100.0, "weights": 1.0}
BLUES = np.frombuffer(bytes.fromhex(
    "f7fbfff6fafef5f9fef4f9fef3f8fdf3f8fdf2f7fdf1f7fdf0f6fceff6fceff5fceef5fcedf4fbecf4fbecf3fbebf3fbeaf2fae9f2fae8f1fae8f1fae7f0f9e6"
    "f0f9e5eff9e4eff9e4eef8e3eef8e2edf8e1edf8e1ecf7e0ecf7dfebf7deebf7ddeaf6ddeaf6dce9f6dbe9f6dae8f5dae8f5d9e7f5d8e7f5d7e6f4d7e6f4d6e5"
    "f4d5e5f4d4e4f3d4e4f3d3e3f3d2e3f3d1e2f2d1e2f2d0e1f2cfe1f2cee0f1cee0f1cddff1ccdff1cbdef0cbdef0caddf0c9ddf0c8dcefc8dcefc7dbefc6dbef"
    "c5daeec4daeec3d9eec1d9edc0d8edbfd8ecbed7ecbcd7ebbbd6ebbad6eab9d5eab7d4eab6d4e9b5d3e9b4d3e8b2d2e8b1d2e7b0d1e7afd1e6add0e6acd0e6ab"
    "cfe5aacfe5a8cee4a7cee4a6cde3a5cde3a3cce3a2cbe2a1cbe2a0cae19ecae19dc9e09bc8e09ac7e098c7df97c6df95c5df93c4de92c3de90c2de8fc1dd8dc0"
    "dd8bc0dd8abfdc88bedc87bddc85bcdb83bbdb82badb80b9da7fb8da7db8d97bb7d97ab6d978b5d877b4d875b3d873b2d772b1d770b1d76fb0d66dafd66baed6"
    "6aadd569acd567abd466aad465aad363a9d362a8d261a7d260a6d15ea5d15da4d05ca3d05aa3cf59a2cf58a1ce57a0ce559fcd549ecd539dcc519ccc509bcb4f"
    "9bcb4e9aca4c99ca4b98c94a97c94896c84795c84694c74594c74393c64292c64191c54090c53f8fc43e8ec43d8dc33c8cc33b8bc23a8ac13989c13888c03787"
    "c03585bf3484bf3383be3282be3181bd3080bd2f7fbc2e7ebc2d7dbb2c7cbb2b7bba2a7ab92979b92878b82777b82676b72575b72474b62373b62272b52171b5"
    "2070b41f6fb31e6eb21e6db21d6cb11c6bb01b6aaf1a69ae1a68ae1967ad1866ac1765ab1764ab1663aa1562a91461a81360a7135fa7125ea6115da5105ca40f"
    "5ba30f5aa30e59a20d58a10c57a00c56a00b559f0a549e09539d08529c08519c08509a084f99084e97084c96084b94084a9208499108488f08478e08468c0845"
    "8b084489084388084286084185084083083f82083e80083d7e083c7d083b7b083a7a08397808387708377508367408357208347108336f08326e08316c08306b"),
    dtype=np.uint8).reshape(256, 3)


# ---------------------------------------------------------------------------------------------------- decimals
def _fma(a: float, b: float, c: float) -> float:
    """fma(a, b, c): a * b + c rounded once (Fraction's conversion to float is correctly rounded)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def round_scaled(x: float, k: int) -> int:
    """x * 10^k rounded to an integer, ties to even on the exact value, for a finite x >= 0 with x * 10^k < 2^52: the module
    docstring's integer / fma formulation, written so that a kernel can restate it (multiply, fma, floor, compares)."""
    p = float(10 ** k)
    hi = x * p
    lo = _fma(x, p, -hi)
    n = math.floor(hi)
    t = (hi - n) - 0.5
    up = t > 0 or (t == 0 and (lo > 0 or (lo == 0 and n % 2 == 1)))
    return n + int(up)


def fixed(x: float, k: int) -> str:
    """format(x, f".{k}f") for k >= 1, through `round_scaled`."""
    n = round_scaled(abs(x), k)
    return ("-" if math.copysign(1.0, x) < 0 else "") + f"{n // 10 ** k}.{n % 10 ** k:0{k}d}"


def lut_index(v: float, vmax: float) -> int:
    """matplotlib's row of the 256-entry table for value v under set_clim(0, vmax)."""
    xa = (v - 0.0) / (vmax - 0.0) * 256.0
    if xa == 256.0:
        return 255
    return 0 if xa < 0 else 255 if xa >= 256 else int(xa)


def shown_values(values, kind: str) -> np.ndarray:
    """What the cells show, float64 [rows, cols]: `pct` of a count matrix, or the weights themselves."""
    if kind == "conf":
        cm = np.asarray(values).astype(np.int64)
        return cm.astype(np.float64) / (cm.sum(axis=1)[:, np.newaxis] + 1e-10) * 100
    return np.asarray(values, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- fonts
def default_font(height: int):
    """The default font at height // 50 pixels (at least 3): 12 for the default picture, through chart.default_font's cache."""
    return chart.default_font(20 * max(int(height) // 50, 3))


_ATLASES = {}  # id(font) -> (font, flat, table, line_h)


def glyph_atlas(font):
    """(flat u8 [bytes], table int32 [13, 5], line_h): the masks of GLYPHS of `font` (annotate.label_masks: `font.getmask(ch, "L")`)
    back to back, per glyph its offset, width, height, its first row below the top of the line box and its advance (at least its
    width); line_h: the rows of the line box, from the highest first row to the lowest last row of the 13."""
    hit = _ATLASES.get(id(font))
    if hit is not None and hit[0] is font:
        return hit[1:]
    cache = an.label_masks(font)
    got = [cache.get(ch) for ch in GLYPHS]
    top0 = min(top for _, top, _ in got)
    table = np.zeros((len(GLYPHS), 5), dtype=np.int32)
    at = 0
    for g, (a, top, adv) in enumerate(got):
        table[g] = (at, a.shape[1], a.shape[0], top - top0, max(adv, a.shape[1]))
        at += a.size
    flat = np.concatenate([np.ascontiguousarray(a).reshape(-1) for a, _, _ in got])
    line_h = int(max(t[3] + t[2] for t in table))
    _ATLASES[id(font)] = (font, flat, table, line_h)
    return flat, table, line_h


# ---------------------------------------------------------------------------------------------------- the plan
@dataclass
class MatrixPlan:
    """The geometry of one figure and its decoration: `items` (annotate ITEM records of frame 0) over `masks`."""
    kind: str
    rows: int
    cols: int
    width: int
    height: int
    x0: int
    y0: int
    pw: int
    ph: int
    bar: tuple              # (bx, by, bw, bh); bw = 0: no colour bar
    line_h: int
    gap: int
    font: object = field(repr=False)
    items: np.ndarray = field(repr=False)
    masks: list = field(repr=False)

    def xe(self, j: int) -> int:
        return self.x0 + (j * self.pw) // self.cols

    def ye(self, i: int) -> int:
        return self.y0 + (i * self.ph) // self.rows

    def cell(self, i: int, j: int):
        """(x0, y0, x1, y1) of cell (i, j), inclusive."""
        return self.xe(j), self.ye(i), self.xe(j + 1) - 1, self.ye(i + 1) - 1

    def band(self, k: int):
        """(x0, y0, x1, y1) of colour band k, inclusive, or None for an empty band."""
        bx, by, bw, bh = self.bar
        lo, hi = (k * bh) // 256, ((k + 1) * bh) // 256 - 1
        return None if hi < lo or bw < 1 else (bx, by + bh - 1 - hi, bx + bw - 1, by + bh - 1 - lo)


def _check_dim(name, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_DIM:
        raise ValueError(f"a matrix figure has 1..{MAX_DIM} {name}, not {v!r}")
    return int(v)


def matrix_plan(rows, cols, kind, width: int = 800, height: int = 600, labels=None, title: str = "", font=None, colorbar: bool = True,
                x_labels: bool = True) -> MatrixPlan:
    """The geometry and the decoration of a `kind` ("conf" / "weights") figure of rows x cols cells, `width` x `height` pixels
    (800 x 600: figsize=(8, 6) at 100 dpi).  labels: the tick labels -- one list for both axes of a square "conf" figure, or the
    pair (row labels, column labels) of visualize.py:145-146; None: the indices.  x_labels=False drops the x ticks, their labels and
    the x caption (visualize.py:150-158).  With pad = max(size // 3, 1) of the font's pixel size:
      top margin     pad + title + pad (no title: pad), the title centred over the plot;
      left margin    pad + the y caption turned a quarter + pad + the widest row label + pad + a tick of pad pixels + 1 for the frame;
      bottom margin  1 + a tick of pad pixels + pad + the column labels + pad + the x caption + pad (x_labels=False: 1 + pad);
      right margin   1 + 2 * pad + a bar of 2 * size columns + 1 + a tick of pad pixels + pad + the widest bar label + pad
                     (colorbar=False: 1 + pad).  The bar is as high as the plot for "conf" and a quarter of it, centred, for
                     "weights" (shrink=0.25, visualize.py:128); its labels are 0, 20, .. 100 / 0.0, 0.2, .. 1.0.
    All text is BLACK.  rows / cols outside 1..16, a picture whose margins leave no plot rectangle, and a cell smaller than its
    widest text (10 digits over "100.0%" for "conf", "0.00" for "weights") raise ValueError."""
    if kind not in KINDS:
        raise ValueError(f"kind {kind!r}: 'conf' or 'weights'")
    rows, cols = _check_dim("rows", rows), _check_dim("cols", cols)
    width, height = int(width), int(height)
    if not (1 <= width <= chart.MAX_SIDE and 1 <= height <= chart.MAX_SIDE):
        raise ValueError(f"a figure of {width} x {height} pixels: sides must be in 1..{chart.MAX_SIDE}")
    if labels is None:
        labels = ([str(i) for i in range(rows)], [str(j) for j in range(cols)])
    elif len(labels) == 2 and not isinstance(labels[0], str):
        labels = ([str(s) for s in labels[0]], [str(s) for s in labels[1]])
    else:
        labels = ([str(s) for s in labels], [str(s) for s in labels])
    if len(labels[0]) != rows or (x_labels and len(labels[1]) != cols):
        raise ValueError(f"{len(labels[0])} row and {len(labels[1])} column labels for {rows} x {cols} cells")
    font = default_font(height) if font is None else font
    cache = an.label_masks(font)
    _, table, line_h = glyph_atlas(font)
    masks, index = [], {}

    def use(text, turn=False):
        a, top, adv = cache.get(text)
        key = (text, turn)
        if key not in index:
            index[key] = len(masks)
            masks.append(np.ascontiguousarray(np.rot90(a)) if turn else a)
        return index[key], masks[index[key]], top

    size = int(getattr(font, "size", 10))
    pad, gap = max(size // 3, 1), max(size // 4, 1)
    y_cap, x_cap = CAPTIONS[kind]
    yt = [use(s) for s in labels[0]]
    xt = [use(s) for s in labels[1]] if x_labels else []
    jy, ay, _ = use(y_cap, turn=True)
    bar_text = [str(v) for v in range(0, 101, 20)] if kind == "conf" else [f"{v / 10:.1f}" for v in range(0, 11, 2)]
    bt = [use(s) for s in bar_text] if colorbar else []
    top_m = pad
    if title:
        jt, at, tt = use(title)
        top_m = pad + tt + at.shape[0] + pad
    left_m = pad + ay.shape[1] + pad + max(a.shape[1] for _, a, _ in yt) + pad + pad + 1
    bottom_m = 1 + pad
    if x_labels:
        jx, ax, tx = use(x_cap)
        xl_h = max(top + a.shape[0] for _, a, top in xt)
        bottom_m = 1 + pad + pad + xl_h + pad + tx + ax.shape[0] + pad
    bar_w = 2 * size if colorbar else 0
    right_m = 1 + 2 * pad + bar_w + 1 + pad + pad + max(a.shape[1] for _, a, _ in bt) + pad if colorbar else 1 + pad
    x0, y0 = left_m, top_m + 1
    pw, ph = width - left_m - right_m, height - y0 - bottom_m
    if pw < 1 or ph < 1:
        raise ValueError(f"a figure of {width} x {height} pixels leaves an empty plot rectangle ({pw} x {ph}) inside its margins "
                         f"(left {left_m}, right {right_m}, top {y0}, bottom {bottom_m})")
    digit = int(table[:10, 4].max())
    if kind == "conf":
        need_w = max(10 * digit, 4 * digit + int(table[G_POINT, 4]) + int(table[G_PERCENT, 4]))
        need_h = 2 * line_h + gap
    else:
        need_w, need_h = 3 * digit + int(table[G_POINT, 4]), line_h
    if pw // cols < need_w or ph // rows < need_h:
        raise ValueError(f"cells of {pw // cols} x {ph // rows} pixels are too small for their text ({need_w} x {need_h} at font size "
                         f"{size}): {rows} x {cols} cells in a plot rectangle of {pw} x {ph}")
    bh = ph if kind == "conf" else max(ph // 4, 1)
    bar = (x0 + pw + 1 + 2 * pad, y0 + (ph - bh) // 2, bar_w, bh) if colorbar else (0, 0, 0, 0)
    plan = MatrixPlan(kind, rows, cols, width, height, x0, y0, pw, ph, bar, line_h, gap, font, None, masks)
    out = [an.outline(0, (x0 - 1, y0 - 1, x0 + pw, y0 + ph), an.BLACK, 1)]
    for i, (j, a, top) in enumerate(yt):
        yc = (plan.ye(i) + plan.ye(i + 1) - 1) // 2
        out.append(an.fill(0, (x0 - 1 - pad, yc, x0 - 2, yc), an.BLACK))
        out.append(an.mask(0, (x0 - 1 - 2 * pad - a.shape[1], yc - a.shape[0] // 2), an.BLACK, j))
    for c, (j, a, top) in enumerate(xt):
        xc = (plan.xe(c) + plan.xe(c + 1) - 1) // 2
        out.append(an.fill(0, (xc, y0 + ph + 1, xc, y0 + ph + pad), an.BLACK))
        out.append(an.mask(0, (xc - a.shape[1] // 2, y0 + ph + 1 + 2 * pad + top), an.BLACK, j))
    if x_labels:
        out.append(an.mask(0, (x0 + pw // 2 - ax.shape[1] // 2, y0 + ph + 1 + 2 * pad + xl_h + pad + tx), an.BLACK, jx))
    out.append(an.mask(0, (pad, y0 + ph // 2 - ay.shape[0] // 2), an.BLACK, jy))
    if title:
        out.append(an.mask(0, (x0 + pw // 2 - at.shape[1] // 2, pad + tt), an.BLACK, jt))
    if colorbar:
        bx, by, bw, _ = bar
        out.append(an.outline(0, (bx - 1, by - 1, bx + bw, by + bh), an.BLACK, 1))
        for t, (j, a, top) in enumerate(bt):
            yc = by + bh - 1 - (t * (bh - 1)) // 5
            out.append(an.fill(0, (bx + bw + 1, yc, bx + bw + pad, yc), an.BLACK))
            out.append(an.mask(0, (bx + bw + 1 + 2 * pad, yc - a.shape[0] // 2), an.BLACK, j))
    plan.items = an.as_items(out)
    return plan


# ---------------------------------------------------------------------------------------------------- the statement
def _check_values(values, plan: MatrixPlan) -> np.ndarray:
    v = np.asarray(values)
    if v.shape != (plan.rows, plan.cols):
        raise ValueError(f"values of shape {v.shape} for a plan of {plan.rows} x {plan.cols} cells")
    if plan.kind == "conf":
        if not np.issubdtype(v.dtype, np.integer):
            raise ValueError("a 'conf' figure takes integer counts")
        v = v.astype(np.int64)
        if v.min() < 0 or v.max() > COUNT_MAX:
            i, j = np.argwhere((v < 0) | (v > COUNT_MAX))[0]
            raise ValueError(f"cell ({i}, {j}): the count {int(v[i, j])} is outside 0..{COUNT_MAX} (10 digits)")
        return v
    v = v.astype(np.float64)
    if not np.isfinite(v).all():
        i, j = np.argwhere(~np.isfinite(v))[0]
        raise ValueError(f"cell ({i}, {j}): the weight {v[i, j]} is not finite")
    return v


def cell_records(values, plan: MatrixPlan):
    """What a kernel would prepare per cell, stated: per cell, row-major, (row of BLUES, text colour 255 / 0, [(glyph, x, y), ...]) -- the cell's
    colour, whether its text is white, and every glyph of its text with the picture position of its mask's top left pixel."""
    v = _check_values(values, plan)
    shown = shown_values(v, plan.kind)
    thresh = (shown.max() + shown.min()) / 2.0
    _, table, line_h = glyph_atlas(plan.font)
    out = []
    for i in range(plan.rows):
        for j in range(plan.cols):
            x = float(shown[i, j])
            if plan.kind == "conf":
                lines = [str(int(v[i, j])), fixed(x, 1) + "%"]
            else:
                if round_scaled(abs(x), 2) > WEIGHT_MAX:
                    raise ValueError(f"cell ({i}, {j}): the weight {x} needs more than {MAX_GLYPHS // 2} characters")
                lines = [fixed(x, 2)]
            cx0, cy0, cx1, cy1 = plan.cell(i, j)
            block = len(lines) * line_h + (len(lines) - 1) * plan.gap
            ty = cy0 + ((cy1 - cy0 + 1 - block) >> 1)
            glyphs = []
            for ln, text in enumerate(lines):
                idx = [GLYPHS.index(ch) for ch in text]
                pen = cx0 + ((cx1 - cx0 + 1 - int(sum(table[g, 4] for g in idx))) >> 1)
                for g in idx:
                    glyphs.append((g, pen, ty + ln * (line_h + plan.gap) + int(table[g, 3])))
                    pen += int(table[g, 4])
            out.append((lut_index(x, CLIM[plan.kind]), 255 if x > thresh else 0, glyphs))
    return out


def paint_numpy(values, plan: MatrixPlan, pic: np.ndarray) -> np.ndarray:
    """Cells, cell text and colour bar painted into `pic` u8 [height, width, 3], IN PLACE: every cell in its colour with its text,
    clipped to the cell, and the colour bar.  Nothing outside the plot rectangle and the bar is touched."""
    flat, table, _ = glyph_atlas(plan.font)
    recs = cell_records(values, plan)
    for c, (lut, ink, glyphs) in enumerate(recs):
        cx0, cy0, cx1, cy1 = plan.cell(c // plan.cols, c % plan.cols)
        pic[cy0:cy1 + 1, cx0:cx1 + 1] = BLUES[lut]
        for g, gx, gy in glyphs:
            off, w, h = (int(t) for t in table[g, :3])
            ax, bx, ay, by = max(gx, cx0), min(gx + w - 1, cx1), max(gy, cy0), min(gy + h - 1, cy1)
            if ax > bx or ay > by:
                continue
            cov = flat[off:off + w * h].reshape(h, w)[ay - gy:by - gy + 1, ax - gx:bx - gx + 1].astype(np.int64)[:, :, None]
            view = pic[ay:by + 1, ax:bx + 1]
            view[...] = np.where(cov > 0, an._blend(view.astype(np.int64), cov, ink), view).astype(np.uint8)
    for k in range(256):
        b = plan.band(k)
        if b is not None:
            pic[b[1]:b[3] + 1, b[0]:b[2] + 1] = BLUES[k]
    return pic


def matrix_numpy(values, plan: MatrixPlan) -> np.ndarray:
    """The CPU statement of a figure: values [rows, cols] (integer counts for "conf", floats for "weights") -> uint8 [height, width,
    3] RGB: a white picture, cells, text and colour bar (`paint_numpy`), then `plan.items` through annotate.draw_numpy."""
    pic = np.full((1, plan.height, plan.width, 3), 255, dtype=np.uint8)
    paint_numpy(values, plan, pic[0])
    return an.draw_numpy(pic, plan.items, plan.masks)[0]


# ---------------------------------------------------------------------------------------------------- the device path
_GLYPH_MASKS = {}  # id(font) -> (font, [u8 [h, w]] * 13)


def glyph_masks(font) -> list:
    """The 13 masks of `glyph_atlas` as u8 [h, w] arrays, the same objects at every call, so that a batch stores them once."""
    hit = _GLYPH_MASKS.get(id(font))
    if hit is None or hit[0] is not font:
        flat, table, _ = glyph_atlas(font)
        hit = _GLYPH_MASKS[id(font)] = (font, [flat[o:o + w * h].reshape(h, w) for o, w, h in table[:, :3].tolist()])
    return hit[1]


def matrix_items(values, plan: MatrixPlan, frame: int = 0):
    """The whole figure as (items ITEM [m] of frame `frame`, masks): drawn in list order onto a WHITE picture (annotate.draw_numpy,
    annotate.draw) they give `matrix_numpy(values, plan)`.  In this order: an opaque FILL per cell in its colour; a MASK per glyph
    of every cell at the position `cell_records` gives, in ink 255 or 0; a FILL per non-empty colour band; `plan.items`.  masks: the
    13 glyph masks (`glyph_masks`), then `plan.masks`.
    `paint_numpy` clips a glyph to its cell, a MASK item is not clipped: a glyph that leaves its cell -- only a weight wider than
    the "0.00" `matrix_plan` sized the cells for can -- raises ValueError naming the cell; nothing else is drawn in its place."""
    recs = cell_records(values, plan)
    glyphs = glyph_masks(plan.font)
    cells, text = [], []
    for c, (lut, ink, line) in enumerate(recs):
        i, j = divmod(c, plan.cols)
        cx0, cy0, cx1, cy1 = plan.cell(i, j)
        cells.append(an.fill(frame, (cx0, cy0, cx1, cy1), BLUES[lut].tolist()))
        for g, gx, gy in line:
            h, w = glyphs[g].shape
            if gx < cx0 or gy < cy0 or gx + w - 1 > cx1 or gy + h - 1 > cy1:
                raise ValueError(f"cell ({i}, {j}): its text {''.join(GLYPHS[q] for q, _, _ in line)!r} leaves the cell of "
                                 f"{cx1 - cx0 + 1} x {cy1 - cy0 + 1} pixels: a larger picture or fewer cells are needed")
            text.append(an.mask(frame, (gx, gy), (ink, ink, ink), g))
    bands = [(k, plan.band(k)) for k in range(256)]
    bands = [an.fill(frame, b, BLUES[k].tolist()) for k, b in bands if b is not None]
    own = plan.items.copy()
    own["frame"] = frame
    own["mask"] = np.where(own["kind"] == an.MASK, own["mask"] + len(glyphs), own["mask"])
    return np.concatenate([an.as_items(cells + text + bands), own]), glyphs + list(plan.masks)


def batch_items(values_list, plans):
    """The item lists of a batch, figure k as frame k, over ONE mask list in which identical masks (the same array, or the same
    shape and bytes) stand once -> (items, masks).  Checks everything `render` refuses."""
    values_list, plans = list(values_list), list(plans)
    if not plans:
        raise ValueError("render: no figure")
    if len(values_list) != len(plans):
        raise ValueError(f"render: {len(values_list)} matrices for {len(plans)} plans")
    if any((p.height, p.width) != (plans[0].height, plans[0].width) for p in plans):
        raise ValueError("render: the figures of one call share one picture size; " +
                         ", ".join(sorted({f"{p.width} x {p.height}" for p in plans})) + " were given")
    masks, by_id, by_bytes, parts = [], {}, {}, []
    for k, (values, plan) in enumerate(zip(values_list, plans)):
        items, own = matrix_items(values, plan, frame=k)
        slot = np.zeros(len(own), dtype=np.int32)
        for q, m in enumerate(own):
            if id(m) not in by_id:
                key = (m.shape, m.tobytes())
                if key not in by_bytes:
                    by_bytes[key] = len(masks)
                    masks.append(m)
                by_id[id(m)] = (by_bytes[key], m)  # the array is kept: its id stays its own
            slot[q] = by_id[id(m)][0]
        items["mask"] = np.where(items["kind"] == an.MASK, slot[items["mask"]], items["mask"])
        parts.append(items)
    return np.concatenate(parts), masks


def render(engine, values_list, plans, max_figures_per_call=None):
    """`matrix_numpy` on the device for a batch: values_list[k] drawn after plans[k]; kinds and shapes may be mixed, the picture
    size is one.  Returns uint8 [n, height, width, 3] RGB on the device: one white canvas, the item lists of all figures with
    frame = k over one shared mask buffer (`batch_items`), drawn by ONE annotate.draw call.  Where annotate.work_table would refuse
    the tiles of one call (2^31 tiles of 64 x 4 pixels) the batch is split by WHOLE figures into several calls; the pictures are
    the same (`max_figures_per_call` forces such a split, for the tests).  An empty list, mixed picture sizes and whatever
    `_check_values` / `matrix_items` refuse of a matrix raise ValueError before any launch."""
    import torch

    items, masks = batch_items(values_list, plans)
    n, height, width = len(plans), plans[0].height, plans[0].width
    flat, table = an.pack_masks(masks)
    an.check_items(items, n, table, len(flat))
    per = ((width - 1) // an.TILE_W + 1) * ((height - 1) // an.TILE_H + 1)  # the most tiles work_table counts for one figure
    step = max(((1 << 31) - 1) // per, 1)
    if max_figures_per_call is not None:
        if int(max_figures_per_call) < 1:
            raise ValueError("render: max_figures_per_call must be at least 1")
        step = min(step, int(max_figures_per_call))
    out = torch.full((n, height, width, 3), 255, dtype=torch.uint8, device=engine.device)
    flat_d = torch.from_numpy(flat).to(engine.device)
    for lo in range(0, n, step):
        sel = items if step >= n else items[(items["frame"] >= lo) & (items["frame"] < lo + step)].copy()
        sel["frame"] -= lo
        an.draw(engine, out[lo:lo + step], sel, (flat_d, table))
    return out


FILE_TYPES = (".jpg", ".jpeg")
NOT_WRITTEN = {".png": "PNG", ".pdf": "PDF", ".svg": "SVG"}  # what the reference's savefig would take from the extension


def check_paths(paths, n=None) -> list:
    """The paths of n figures as strings.  The reference takes the format from the extension (visualize.py:85); this project writes
    JPEG files only: `.jpg` / `.jpeg` pass, `.png`, `.pdf`, `.svg` are refused by name, anything else too (ValueError)."""
    paths = [os.fspath(p) for p in paths]
    for p in paths:
        ext = os.path.splitext(p)[1].lower()
        if ext in NOT_WRITTEN:
            raise ValueError(f"{p}: {NOT_WRITTEN[ext]} files are not written by this project: name the figure .jpg or .jpeg")
        if ext not in FILE_TYPES:
            raise ValueError(f"{p}: a figure is a JPEG file, named .jpg or .jpeg, not {ext!r}")
    if n is not None and len(paths) != n:
        raise ValueError(f"{len(paths)} paths for {n} figures")
    return paths


def _titles(titles, n):
    if titles is None:
        return ["Confusion Matrix"] * n  # the default of both functions of the reference (visualize.py:13,91)
    if isinstance(titles, str):
        return [titles] * n
    if len(titles) != n:
        raise ValueError(f"{len(titles)} titles for {n} figures")
    return [str(t) for t in titles]


def write_figures(engine, values_list, plans, paths, quality: int = 95, subsampling: int = 2, entropy: str = "device"):
    """`render`, then one file per figure: paths[k] is PIL's Image.save(quality=quality, subsampling=subsampling) of
    `matrix_numpy(values_list[k], plans[k])`, byte for byte (ONE jpeg.encode_images call over the batch; `entropy` as there).
    Directories are made.  Every refusal comes before the first launch.  Returns the paths."""
    from . import jpeg

    jpeg._check_entropy(entropy)
    plans = list(plans)
    paths = check_paths(paths, len(plans))
    pics = render(engine, values_list, plans)
    n, h, w = (int(v) for v in pics.shape[:3])
    rects = np.zeros((n, 5), dtype=np.int32)
    rects[:, 0], rects[:, 3], rects[:, 4] = np.arange(n), w, h
    files = jpeg.encode_images(engine, pics, rects, bgr=False, quality=quality, subsampling=subsampling, entropy=entropy)
    for path, data in zip(paths, files):
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)
    return paths


def write_conf_matrices(engine, cms, labels, paths, titles=None, width: int = 800, height: int = 600, colorbar: bool = True,
                        font=None, quality: int = 95, subsampling: int = 2, entropy: str = "device"):
    """plot_conf_matrix (visualize.py:10-85) for a batch: cms[k] (integer counts [rows, cols]) with the tick labels `labels` (one
    list for all; None: the indices) and titles[k] (None: the reference's "Confusion Matrix"; a string: that for all) is written
    to paths[k], all in one `write_figures` call.  Returns the paths."""
    cms = [np.asarray(cm) for cm in cms]
    paths = check_paths(paths, len(cms))
    titles = _titles(titles, len(cms))
    plans = [matrix_plan(cm.shape[0], cm.shape[1], "conf", width, height, labels, t, font, colorbar) if cm.ndim == 2 else None
             for cm, t in zip(cms, titles)]
    if any(p is None for p in plans):
        raise ValueError("a confusion matrix is a [rows, cols] array")
    return write_figures(engine, cms, plans, paths, quality, subsampling, entropy)


def write_weights_matrices(engine, weights, labels, paths, titles=None, width: int = 800, height: int = 600, colorbar: bool = True,
                           x_labels=True, font=None, quality: int = 95, subsampling: int = 2, entropy: str = "device"):
    """plot_weights_matrix (visualize.py:88-172) for a batch: weights[k] (floats [models, classes]) with `labels` = (row labels,
    column labels) for all (None: the indices), titles[k] as in `write_conf_matrices` and x_labels (a bool for all, or one per
    figure) is written to paths[k], all in one `write_figures` call.  Returns the paths."""
    weights = [np.asarray(w) for w in weights]
    paths = check_paths(paths, len(weights))
    titles = _titles(titles, len(weights))
    xl = [x_labels] * len(weights) if isinstance(x_labels, (bool, np.bool_)) else list(x_labels)
    if len(xl) != len(weights):
        raise ValueError(f"{len(xl)} x_labels for {len(weights)} figures")
    if any(w.ndim != 2 for w in weights):
        raise ValueError("a weight matrix is a [models, classes] array")
    plans = [matrix_plan(w.shape[0], w.shape[1], "weights", width, height, labels, t, font, colorbar, bool(x))
             for w, t, x in zip(weights, titles, xl)]
    return write_figures(engine, weights, plans, paths, quality, subsampling, entropy)
