"""The prediction timeline chart (run.py:272-296 `flag_save_plot_pred`, visualization/visualize.py:175-215
plot_compound_expression_prediction): the compound-expression class of the four models against the frame number, in one picture,
`pedicted_CEs_Rule N.jpg` -- drawn on the device from the class tables where they lie and written as a JPEG file.

tables -> traces -> text -> file: `Engine.chart_series` (avcer_chart_series, csrc/chart.hip) rasterises the four traces of every
chart of a batch, `annotate.draw` lays frame, ticks, titles and legend over them, `jpeg.encode_images` writes the files; only file
bytes cross to the host.

The reference plots with matplotlib, which is not among this project's dependencies.  As with the result video the claim is
identity with PIL at tolerance zero -- `ImageDraw.line(width=1)` for the traces, `ImageDraw.bitmap` for the text, `Image.save` for
the file -- and `chart_numpy` is the statement the kernel and PIL are both held to (tests/test_chart_cpu.py,
tests/test_gpu_chart.py).  Agg's anti-aliasing, matplotlib's fonts and its `bbox_inches="tight"` crop are not reproduced.

Geometry (`chart_plan`), integers only: the plot rectangle (x0, y0, pw, ph) inside margins sized by the text; seven row centres
yc[c] = y0 + ph - 1 - ((2c + 1) * ph) // 14, class 0 lowest; the column of frame i: col(i) = x0 + ((2i + 1) * pw) // (2T).

The line rule (`line_runs`): PIL 12's ImagingDrawLine from (xa, ya) to (xb, yb), dx = |xb - xa|, dy = |yb - ya|, both ends drawn:
  dx > dy   one pixel per column: at the column m steps from xa the row (2 * dy * m + dx) // (2 * dx) steps from ya;
  else      one pixel per row: at the row j steps from ya the column (2 * dx * j + dy) // (2 * dy) steps from xa (dx = 0: xa),
            so column m holds the rows j = ceil(dy * (2m - 1) / (2dx)) (0 for m = 0) .. min(dy, ceil(dy * (2m + 1) / (2dx)) - 1).
A tie steps away from the START, so the rule depends on the direction; the chart always draws from frame i to frame i + 1.
The trace of a series is the union over its T - 1 segments (T = 1: the one point); then it is widened by one row up and down,
clipped to the plot rectangle and THINNED: pixel (x, y) of series s is painted iff (x + y) % 4 == s.  The thinning stands in for
linestyle="dotted"; no two series contend for a pixel, so coinciding traces all stay visible and the order plays no part.

One interval per column: every segment covers, in one column, one contiguous run of rows, and it covers both its end points.  In a
column that holds frames f .. l the runs of the segments f-1 -> f, ..., l -> l+1 each contain one of the points (col, yc[v[i]]),
f <= i <= l, and consecutive ones share a point, so their union is one interval min .. max; a column that holds no frame is
crossed by one segment.  The envelope is therefore ONE row interval per (series, column), for every T.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np

from . import annotate as an
from .fusion import COMPOUND_NAMES, MODEL_ORDER

COLOUR_NAMES = ("green", "orange", "red", "purple")  # visualize.py:178, in series order
COLOURS = ((0, 128, 0), (255, 165, 0), (255, 0, 0), (128, 0, 128))  # PIL.ImageColor.getrgb of those names
N_CLASSES = len(COMPOUND_NAMES)
MAX_SERIES = 4        # the thinning rule has four residues
MAX_SIDE = 16384      # AVCER_CHART_MAX_SIDE: a row fits the 16 bits the envelope gives it
TITLE = "Compound expressions predicted by models"  # run.py:291 (its first letter there is U+0421, which the default font lacks)
X_TITLE, Y_TITLE = "Number of frames", "Compound expression"  # visualize.py:192-193
PATH_REDUCE, PATH_SEGMENT = 1, 2  # AVCER_CHART_REDUCE / _SEGMENT: T >= pw, a column reduces its frames / T < pw, one segment crosses it
PATH_NAMES = {PATH_REDUCE: "T >= pw: column reduction", PATH_SEGMENT: "T < pw: crossing segment"}
PLAN = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("pw", "<i4"), ("ph", "<i4"), ("yc", "<i4", N_CLASSES), ("pad", "<i4"),
                 ("offset", "<i8"), ("length", "<i8")])  # struct avcer_chart_plan


@dataclass
class ChartPlan:
    """The geometry of one chart of T frames and its decoration: `items` (annotate ITEM records of frame 0) over `masks`."""
    T: int
    width: int
    height: int
    x0: int
    y0: int
    pw: int
    ph: int
    yc: tuple
    items: np.ndarray = field(repr=False)
    masks: list = field(repr=False)

    def col(self, i):
        """The column of frame i (an int, or an int64 array), in 64 bits."""
        return self.x0 + ((2 * np.asarray(i, dtype=np.int64) + 1) * self.pw) // (2 * self.T)

    @property
    def path(self) -> int:
        return PATH_REDUCE if self.T >= self.pw else PATH_SEGMENT

    def with_T(self, T: int) -> "ChartPlan":
        """The same picture layout for another number of frames (the decoration does not depend on T)."""
        T = _check_T(T)
        return ChartPlan(T, self.width, self.height, self.x0, self.y0, self.pw, self.ph, self.yc, self.items, self.masks)

    def record(self, offset: int = 0) -> np.ndarray:
        return np.array([(self.x0, self.y0, self.pw, self.ph, self.yc, 0, offset, self.T)], dtype=PLAN)


def _check_T(T) -> int:
    if isinstance(T, (bool, np.bool_)) or not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError(f"a chart needs T >= 1 frames, not {T!r}")
    return int(T)


def default_font(height: int):
    """The default font at height // 20 pixels (at least 3): 10 for the default picture, through annotate's font cache."""
    from PIL import ImageFont

    key = ("default", max(int(height) // 20, 3))
    if key not in an._LABEL_CACHES:
        font = ImageFont.load_default(size=key[1])
        an._LABEL_CACHES[key] = (font, an.LabelMasks(font))
    return an._LABEL_CACHES[key][0]


def chart_plan(T, width: int = 1200, height: int = 200, font=None) -> ChartPlan:
    """The geometry and the decoration of a chart of T frames, `width` x `height` pixels.  With pad = max(size // 3, 1) of the font's
    pixel size and the text masks of annotate's cache (mask, top, advance):
      top margin     pad + title + pad, the title centred over the picture;
      left margin    pad + the y title turned a quarter (np.rot90 of its mask) + pad + the widest tick label + pad + a tick of pad
                     pixels + 1 for the frame;
      right margin   1 + pad + a swatch of `size` pixels + pad + the widest legend label + pad;
      bottom margin  1 + pad + x title + pad.
    Items, in this order: the frame, an OUTLINE of width 1 around the plot rectangle (outside it); per class its tick and its label
    (visualize.py:196-207), right-aligned and centred on yc[c]; the x title centred under the plot, the y title centred beside it,
    the title; per series a swatch in its colour and its MODEL_ORDER name, from the top of the right margin down.  All text is BLACK.
    T < 1, and a picture whose margins leave no plot rectangle, raise ValueError."""
    T = _check_T(T)
    width, height = int(width), int(height)
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"a chart of {width} x {height} pixels: sides must be in 1..{MAX_SIDE}")
    font = default_font(height) if font is None else font
    cache = an.label_masks(font)
    masks, index = [], {}

    def use(text, turn=False):
        a, top, adv = cache.get(text)
        key = (text, turn)
        if key not in index:
            index[key] = len(masks)
            masks.append(np.ascontiguousarray(np.rot90(a)) if turn else a)
        return index[key], masks[index[key]], top

    size = int(getattr(font, "size", 10))
    pad = max(size // 3, 1)
    ticks = [use(n) for n in COMPOUND_NAMES]
    legend = [use(n) for n in MODEL_ORDER[:MAX_SERIES]]
    jt, at, tt = use(TITLE)
    jx, ax, tx = use(X_TITLE)
    jy, ay, _ = use(Y_TITLE, turn=True)
    top_m = pad + tt + at.shape[0] + pad
    left_m = pad + ay.shape[1] + pad + max(a.shape[1] for _, a, _ in ticks) + pad + pad + 1
    right_m = 1 + pad + size + pad + max(a.shape[1] for _, a, _ in legend) + pad
    bottom_m = 1 + pad + tx + ax.shape[0] + pad
    x0, y0 = left_m, top_m + 1
    pw, ph = width - left_m - right_m, height - y0 - bottom_m
    if pw < 1 or ph < 1:
        raise ValueError(f"a chart of {width} x {height} pixels leaves an empty plot rectangle ({pw} x {ph}) inside its margins "
                         f"(left {left_m}, right {right_m}, top {y0}, bottom {bottom_m})")
    yc = tuple(y0 + ph - 1 - ((2 * c + 1) * ph) // (2 * N_CLASSES) for c in range(N_CLASSES))
    out = [an.outline(0, (x0 - 1, y0 - 1, x0 + pw, y0 + ph), an.BLACK, 1)]
    for c, (j, a, top) in enumerate(ticks):
        out.append(an.fill(0, (x0 - 1 - pad, yc[c], x0 - 2, yc[c]), an.BLACK))
        out.append(an.mask(0, (x0 - 1 - 2 * pad - a.shape[1], yc[c] - a.shape[0] // 2), an.BLACK, j))
    out.append(an.mask(0, (x0 + pw // 2 - ax.shape[1] // 2, y0 + ph + 1 + pad + tx), an.BLACK, jx))
    out.append(an.mask(0, (pad, y0 + ph // 2 - ay.shape[0] // 2), an.BLACK, jy))
    out.append(an.mask(0, (width // 2 - at.shape[1] // 2, pad + tt), an.BLACK, jt))
    for s, (j, a, top) in enumerate(legend):
        ly = y0 + s * (size + pad)
        out.append(an.fill(0, (x0 + pw + 1 + pad, ly, x0 + pw + pad + size, ly + size - 1), COLOURS[s]))
        out.append(an.mask(0, (x0 + pw + 1 + 2 * pad + size, ly + (size - a.shape[0]) // 2), an.BLACK, j))
    return ChartPlan(T, width, height, x0, y0, pw, ph, yc, an.as_items(out), masks)


def line_runs(xa, ya, xb, yb):
    """The pixels of ImageDraw.line([(xa, ya), (xb, yb)], width=1), for n segments at once (int arrays [n]), as one run of rows per
    column a segment touches: (x, lo, hi) int64 arrays, rows lo .. hi inclusive.  The module docstring states the rule."""
    xa, ya, xb, yb = (np.atleast_1d(np.asarray(v, dtype=np.int64)) for v in (xa, ya, xb, yb))
    dx, dy = np.abs(xb - xa), np.abs(yb - ya)
    xs, ys = np.sign(xb - xa), np.sign(yb - ya)
    cols = dx + 1
    seg = np.repeat(np.arange(len(xa)), cols)
    m = np.arange(int(cols.sum()), dtype=np.int64) - np.repeat(np.cumsum(cols) - cols, cols)
    sdx, sdy = dx[seg], dy[seg]
    den = np.maximum(2 * sdx, 1)
    k = (2 * sdy * m + sdx) // den                                                   # dx > dy: the one row of column m
    j_lo = np.where(m == 0, 0, -((-(sdy * (2 * m - 1))) // den))                     # else: the rows j_lo .. j_hi of column m
    j_hi = np.where(sdx == 0, sdy, np.minimum(sdy, -((-(sdy * (2 * m + 1))) // den) - 1))
    shallow = sdx > sdy
    a = ya[seg] + ys[seg] * np.where(shallow, k, j_lo)
    b = ya[seg] + ys[seg] * np.where(shallow, k, j_hi)
    return xa[seg] + xs[seg] * m, np.minimum(a, b), np.maximum(a, b)


def runs_to_mask(x, lo, hi, height: int, width: int) -> np.ndarray:
    """The union of runs (column x, rows lo .. hi) as a bool [height, width]; what lies outside the canvas is dropped."""
    keep = (x >= 0) & (x < width) & (hi >= 0) & (lo < height)
    x, lo, hi = x[keep], np.maximum(lo[keep], 0), np.minimum(hi[keep], height - 1)
    d = np.zeros((height + 1, width), dtype=np.int64)
    np.add.at(d, (lo, x), 1)
    np.add.at(d, (hi + 1, x), -1)
    return np.cumsum(d, axis=0)[:height] > 0


def check_classes(lo: int, hi: int):
    if lo < 0 or hi >= N_CLASSES:
        raise ValueError(f"a class value {lo if lo < 0 else hi} outside 0..{N_CLASSES - 1}")


def _check_preds(preds, plan: ChartPlan) -> np.ndarray:
    p = np.asarray(preds)
    if p.ndim != 2 or not (1 <= p.shape[0] <= MAX_SERIES) or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"preds must be an integer [S, T] table of 1..{MAX_SERIES} series")
    if p.shape[1] != plan.T:
        raise ValueError(f"preds hold {p.shape[1]} frames, the plan {plan.T}")
    check_classes(int(p.min()), int(p.max()))
    return p.astype(np.int64)


def trace_numpy(v, plan: ChartPlan) -> np.ndarray:
    """The trace of one series v int [T] before widening, clipping and thinning: bool [height, width], the union of
    ImageDraw.line(width=1) between (col(i), yc[v[i]]) of consecutive frames; a lone frame is one point."""
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    x = plan.col(np.arange(plan.T))
    y = np.asarray(plan.yc, dtype=np.int64)[v]
    if plan.T == 1:
        return runs_to_mask(x, y, y, plan.height, plan.width)
    return runs_to_mask(*line_runs(x[:-1], y[:-1], x[1:], y[1:]), plan.height, plan.width)


def series_numpy(preds, plan: ChartPlan) -> np.ndarray:
    """What series s paints: bool [S, height, width] -- its trace widened by one row up and down, clipped to the plot rectangle
    and thinned to (x + y) % 4 == s."""
    p = _check_preds(preds, plan)
    yy, xx = np.mgrid[0:plan.height, 0:plan.width]
    inside = (xx >= plan.x0) & (xx < plan.x0 + plan.pw) & (yy >= plan.y0) & (yy < plan.y0 + plan.ph)
    out = np.zeros((len(p), plan.height, plan.width), dtype=bool)
    for s, v in enumerate(p):
        t = trace_numpy(v, plan)
        wide = t.copy()
        wide[1:] |= t[:-1]
        wide[:-1] |= t[1:]
        out[s] = wide & inside & ((xx + yy) % 4 == s)
    return out


def chart_numpy(preds, plan: ChartPlan) -> np.ndarray:
    """The CPU statement of the chart: preds int [S, T] (S <= 4, classes 0..6, series in MODEL_ORDER) -> uint8 [height, width, 3]
    RGB: a white picture, the four series in their colours (`series_numpy`), then `plan.items` through annotate.draw_numpy."""
    pic = np.full((1, plan.height, plan.width, 3), 255, dtype=np.uint8)
    for s, m in enumerate(series_numpy(preds, plan)):
        pic[0][m] = COLOURS[s]
    return an.draw_numpy(pic, plan.items, plan.masks)[0]


def batch_items(plans):
    """The decoration of a batch: every plan's items with frame = its place in the batch, over one shared mask list."""
    masks, at, parts = [], {}, []
    for v, plan in enumerate(plans):
        key = id(plan.masks)
        if key not in at:
            at[key] = len(masks)
            masks.extend(plan.masks)
        it = plan.items.copy()
        it["frame"] = v
        it["mask"] = np.where(it["kind"] == an.MASK, it["mask"] + at[key], it["mask"])
        parts.append(it)
    return np.concatenate(parts), masks


def _plans(preds, T, plan):
    """(lengths, plans) of a call: T None -> one chart of all columns; an int or a list -> charts back to back."""
    total = int(preds.shape[1])
    lengths = [total] if T is None else ([T] if isinstance(T, (int, np.integer)) else list(T))
    lengths = [_check_T(t) for t in lengths]
    if sum(lengths) != total:
        raise ValueError(f"charts of {lengths} frames over a table of {total} columns")
    if plan is None:
        base = chart_plan(lengths[0])
        plans = [base if t == base.T else base.with_T(t) for t in lengths]
    elif isinstance(plan, ChartPlan):
        plans = [plan if t == plan.T else plan.with_T(t) for t in lengths]
    else:
        plans = list(plan)
        if len(plans) != len(lengths) or any(p.T != t for p, t in zip(plans, lengths)):
            raise ValueError("one plan per chart, each of its chart's length")
    if any((p.height, p.width) != (plans[0].height, plans[0].width) for p in plans):
        raise ValueError("the charts of one call share one picture size")
    return lengths, plans


def render(engine, preds, T=None, plan=None):
    """`chart_numpy` on the device: preds int32 / int64 [S, sum T] on the device (as the fusion leaves `am`), the tables of V charts
    back to back; T: their lengths (None: one chart); plan: a ChartPlan for all (its T is replaced) or one per chart; None:
    chart_plan's default picture.  Returns uint8 [V, height, width, 3] RGB on the device: white, the traces by ONE
    Engine.chart_series call, the decoration by ONE annotate.draw call.  The tables stay on the device: two numbers, their smallest
    and largest value, are read back to refuse a class outside 0..6 (ValueError) before any launch of this module."""
    import torch

    if not (torch.is_tensor(preds) and preds.dim() == 2 and preds.dtype in (torch.int32, torch.int64)):
        raise ValueError("render: preds must be an int32 or int64 [S, sum T] tensor")
    if not 1 <= int(preds.shape[0]) <= MAX_SERIES:
        raise ValueError(f"render: 1..{MAX_SERIES} series")
    lengths, plans = _plans(preds, T, plan)
    preds = preds.to(engine.device).contiguous()
    check_classes(*(int(v) for v in torch.stack(torch.aminmax(preds)).tolist()))
    out = torch.full((len(plans), plans[0].height, plans[0].width, 3), 255, dtype=torch.uint8, device=engine.device)
    engine.chart_series(preds, plans, out)
    items, masks = batch_items(plans)
    return an.draw(engine, out, items, masks)


def write_charts(engine, preds, paths, quality: int = 95, entropy: str = "device", T=None, plan=None):
    """`render`, then one file per chart: paths[v] is PIL's Image.save(quality=quality, subsampling=2) of chart v, byte for byte
    (jpeg.encode_images; `entropy` as there).  Directories are made.  Returns `paths`."""
    from . import jpeg

    jpeg._check_entropy(entropy)
    paths = [os.fspath(p) for p in paths]
    pics = render(engine, preds, T, plan)
    if len(paths) != int(pics.shape[0]):
        raise ValueError(f"{len(paths)} paths for {int(pics.shape[0])} charts")
    n, h, w = (int(v) for v in pics.shape[:3])
    rects = np.zeros((n, 5), dtype=np.int32)
    rects[:, 0], rects[:, 3], rects[:, 4] = np.arange(n), w, h
    files = jpeg.encode_images(engine, pics, rects, bgr=False, quality=quality, subsampling=2, entropy=entropy)
    for path, data in zip(paths, files):
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)
    return paths


# ---------------------------------------------------------------------------------------------------- run_inference's option
def rule_name(ce_weights_type, ce_mask) -> str:
    """run.py:281-284: "Rule 1" with ce_mask, overwritten by "Rule 2" with ce_weights_type; with neither the reference dies on an
    unbound name, here ValueError."""
    if ce_weights_type:
        return "Rule 2"
    if ce_mask:
        return "Rule 1"
    raise ValueError("flag_save_plot_pred needs ce_mask (Rule 1) or ce_weights_type (Rule 2): the file is named after the rule")


def check_plot_pred(flag_save_plot_pred, path_save_results, ce_weights_type, ce_mask, plot_size):
    """What the option refuses before any work -> (rule, (height, width)), or None when it is off."""
    if isinstance(flag_save_plot_pred, (bool, np.bool_)) and not flag_save_plot_pred:
        return None
    if not isinstance(flag_save_plot_pred, (bool, np.bool_)):
        raise ValueError(f"flag_save_plot_pred must be a bool, not {flag_save_plot_pred!r}")
    if not path_save_results:
        raise ValueError("flag_save_plot_pred needs path_save_results: the chart is a file there")
    rule = rule_name(ce_weights_type, ce_mask)
    try:
        height, width = (int(v) for v in plot_size)
    except (TypeError, ValueError):
        raise ValueError(f"plot_size must be (height, width), not {plot_size!r}") from None
    chart_plan(1, width, height)  # an empty plot rectangle is refused here
    return rule, (height, width)


def plot_paths(path_save_results, rule: str, tracks=None):
    """`<path_save_results>/pedicted_CEs_<rule>.jpg` (the reference's spelling, run.py:286); with `tracks` (the selected track
    directories) the first under that name and every other track k as `pedicted_CEs_<rule>__t<kk>.jpg`."""
    first = os.path.join(path_save_results, f"pedicted_CEs_{rule}.jpg")
    if tracks is None:
        return [first]
    return [first] + [os.path.join(path_save_results, f"pedicted_CEs_{rule}__t{k:02d}.jpg") for k in list(tracks)[1:]]
