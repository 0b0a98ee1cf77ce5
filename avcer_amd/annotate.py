"""The result video (video/visualization.py, video/functions/get_visualization.py:40-118): every face box and a
"<label>: <p>%" line drawn on every frame, on the device, and the frames written as a Motion-JPEG AVI file.

decode -> draw -> encode: `jpeg.decode_frames` left the frames on the device, `draw` (avcer_annotate_frames, csrc/annotate.hip) draws
into a copy of them there, the JPEG encoder turns the copy into files, and only file bytes cross to the host (`avi.AviWriter`).

The reference draws with cv2 (LINE_AA rectangles, the Hershey font).  cv2 is not among this project's dependencies; as everywhere
else the claim is identity with PIL, here `ImageDraw`, with tolerance zero -- `draw_numpy` is the statement the kernel and PIL are
both held to (tests/test_annotate_cpu.py, tests/test_gpu_annotate.py).  Anti-aliased box edges and cv2's glyphs are not reproduced.

A drawing is a list of ITEM records sorted by frame (struct avcer_draw_item, include/avcer_hip.h), three kinds:
  OUTLINE  ImageDraw.rectangle((x0, y0, x1, y1), outline=colour, width=t): inclusive corners, the border grows inward;
  FILL     ImageDraw.bitmap((x0, y0), Image.new("L", (x1 - x0 + 1, y1 - y0 + 1), c), fill=colour): constant coverage c in 1..255;
  MASK     ImageDraw.bitmap((x, y), mask.resize((k * w, k * h), NEAREST), fill=colour): a u8 coverage mask at integer scale k.
Within a frame the result is that of drawing the items one after another in list order.  Coverage blends as PIL's BLEND8 does
in this PIL (12.x): dst = MULDIV255-rounding of the SUM dst * (255 - c) + colour * c, rounded once -- not each product on its own;
the two agree for colours 0 and 255 only, and the exhaustive test settles it.  Colours are in the frame's channel order.
"""
from __future__ import annotations

import numpy as np

from .fusion import COMPOUND_NAMES

OUTLINE, FILL, MASK = 0, 1, 2  # AVCER_DRAW_*
KIND_NAMES = ("OUTLINE", "FILL", "MASK")
ITEM = np.dtype([("frame", "<i4"), ("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("arg", "<i4"),
                 ("mask", "<i4"), ("colour", "<i4", 3), ("pad", "<i4")])  # struct avcer_draw_item
COORD_MAX = 1 << 24   # corners beyond +-2^24 are refused: every sum of the kernel then fits 32 bits many times over
SCALE_MAX = 64        # the largest integer scale of a MASK
TILE_W, TILE_H = 64, 4  # csrc/annotate.hip: pixels of one block
MAGENTA = (255, 0, 255)  # get_visualization.py:48; the same in BGR and RGB
WHITE, BLACK = (255, 255, 255), (0, 0, 0)
BACKDROP = 160        # coverage of the black rectangle behind a label and behind the panel


def outline(frame, box, colour, width=1):
    """The record of ImageDraw.rectangle(box, outline=colour, width=width) on frame `frame`; box = (x0, y0, x1, y1) inclusive."""
    return (frame, OUTLINE, box[0], box[1], box[2], box[3], width, 0, tuple(colour), 0)


def fill(frame, box, colour, coverage=255):
    """The record of a rectangle of constant coverage (255: opaque); box = (x0, y0, x1, y1) inclusive."""
    return (frame, FILL, box[0], box[1], box[2], box[3], coverage, 0, tuple(colour), 0)


def mask(frame, xy, colour, index, scale=1):
    """The record of mask `index` drawn with its top left pixel at xy, every mask pixel `scale` x `scale` frame pixels."""
    return (frame, MASK, xy[0], xy[1], 0, 0, scale, index, tuple(colour), 0)


def as_items(items) -> np.ndarray:
    """A list of records (`outline`, `fill`, `mask`) or an ITEM array -> a contiguous ITEM array."""
    if isinstance(items, np.ndarray) and items.dtype == ITEM:
        return np.ascontiguousarray(items.reshape(-1))
    return np.array([tuple(it) for it in items], dtype=ITEM).reshape(-1)


def pack_masks(masks):
    """A list of u8 [h, w] coverage masks -> (the masks back to back u8 [bytes], table int32 [k, 3] = offset, width, height).  A pair
    that is already packed passes through."""
    if isinstance(masks, tuple) and len(masks) == 2 and getattr(masks[0], "ndim", 0) == 1 and np.ndim(masks[1]) == 2:
        return masks[0], np.ascontiguousarray(masks[1], dtype=np.int32).reshape(-1, 3)
    table = np.zeros((len(masks), 3), dtype=np.int32)
    parts, at = [], 0
    for j, m in enumerate(masks):
        m = np.asarray(m)
        if m.dtype != np.uint8 or m.ndim != 2 or m.size == 0:
            raise ValueError(f"mask {j}: a non-empty uint8 [h, w] array is needed")
        table[j] = (at, m.shape[1], m.shape[0])
        parts.append(np.ascontiguousarray(m).reshape(-1))
        at += m.size
    flat = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return flat, table


def check_items(items: np.ndarray, n_frames: int, table: np.ndarray, masks_bytes: int):
    """What is refused before any launch, with a ValueError that names the item (or the mask)."""
    table = np.asarray(table).reshape(-1, 3)
    t64 = table.astype(np.int64)
    bad = np.flatnonzero((t64[:, 0] < 0) | (t64[:, 1] <= 0) | (t64[:, 2] <= 0) | (t64[:, 0] + t64[:, 1] * t64[:, 2] > masks_bytes))
    if len(bad):
        j = int(bad[0])
        raise ValueError(f"mask {j}: offset {t64[j, 0]}, {t64[j, 1]} x {t64[j, 2]} leaves the mask buffer of {masks_bytes} bytes")
    if not len(items):
        return
    it = items
    k, a = it["kind"], it["arg"].astype(np.int64)
    box = (k == OUTLINE) | (k == FILL)
    width = np.zeros(len(it), dtype=np.int64)
    height = np.zeros(len(it), dtype=np.int64)
    ok_mask = (k == MASK) & (it["mask"] >= 0) & (it["mask"] < len(table))
    width[ok_mask] = table[it["mask"][ok_mask], 1]
    height[ok_mask] = table[it["mask"][ok_mask], 2]
    corners = np.stack([it["x0"], it["y0"], np.where(box, it["x1"], 0), np.where(box, it["y1"], 0)], axis=1).astype(np.int64)
    rules = (
        ((k < 0) | (k > MASK), lambda i: f"kind {int(k[i])} (0 OUTLINE, 1 FILL, 2 MASK)"),
        ((it["frame"] < 0) | (it["frame"] >= n_frames), lambda i: f"frame {int(it['frame'][i])} outside [0, {n_frames})"),
        (np.concatenate([[False], np.diff(it["frame"]) < 0]),
         lambda i: f"frame {int(it['frame'][i])} behind frame {int(it['frame'][i - 1])}: the items must be sorted by frame"),
        ((np.abs(corners) > COORD_MAX).any(axis=1), lambda i: f"a corner beyond +-{COORD_MAX}"),
        (box & ((it["x1"] < it["x0"]) | (it["y1"] < it["y0"])),
         lambda i: f"box ({int(it['x0'][i])}, {int(it['y0'][i])}, {int(it['x1'][i])}, {int(it['y1'][i])}) has x1 < x0 or y1 < y0"),
        ((k == OUTLINE) & ((a < 1) | (a > COORD_MAX)), lambda i: f"width {int(a[i])} (at least 1)"),
        ((k == FILL) & ((a < 1) | (a > 255)), lambda i: f"coverage {int(a[i])} outside 1..255"),
        ((k == MASK) & ~ok_mask, lambda i: f"mask index {int(it['mask'][i])} outside [0, {len(table)})"),
        ((k == MASK) & ((a < 1) | (a > SCALE_MAX)), lambda i: f"scale {int(a[i])} outside 1..{SCALE_MAX}"),
        (((it["colour"] < 0) | (it["colour"] > 255)).any(axis=1), lambda i: f"colour {tuple(int(c) for c in it['colour'][i])} outside 0..255"),
    )
    first = None
    for bad, say in rules:
        hit = np.flatnonzero(bad)
        if len(hit) and (first is None or hit[0] < first[0]):
            first = (int(hit[0]), say)
    if first is not None:
        i, say = first
        raise ValueError(f"item {i} ({KIND_NAMES[int(k[i])] if 0 <= k[i] <= MASK else '?'}): {say(i)}")


def extents(items: np.ndarray, table: np.ndarray):
    """(x0, y0, x1, y1) int64 [m] each: an inclusive rectangle that holds every pixel the item can touch, before clipping.  For an
    OUTLINE that is more than its box when the width exceeds a side: PIL's border rows y0 .. y0+t-1 and y1-t+1 .. y1 and its columns
    then run past the box, and so do this module's."""
    it = items
    k, a = it["kind"], it["arg"].astype(np.int64)
    x0, y0, x1, y1 = (it[f].astype(np.int64) for f in ("x0", "y0", "x1", "y1"))
    o = k == OUTLINE
    ex0 = np.where(o, np.minimum(x0, x1 - a + 1), x0)
    ey0 = np.where(o, np.minimum(y0, y1 - a + 1), y0)
    ex1 = np.where(o, np.maximum(x1, x0 + a - 1), x1)
    ey1 = np.where(o, np.maximum(y1, y0 + a), y1)
    m = k == MASK
    if m.any():
        tw = np.zeros(len(it), dtype=np.int64)
        th = np.zeros(len(it), dtype=np.int64)
        tw[m] = np.asarray(table).reshape(-1, 3)[it["mask"][m], 1]
        th[m] = np.asarray(table).reshape(-1, 3)[it["mask"][m], 2]
        ex1 = np.where(m, x0 + a * tw - 1, ex1)
        ey1 = np.where(m, y0 + a * th - 1, ey1)
    return ex0, ey0, ex1, ey1


def work_table(items: np.ndarray, table: np.ndarray, n_frames: int, height: int, width: int):
    """The launch plan of avcer_annotate_frames (include/avcer_hip.h): int32 [rows, 8], one row per frame whose items touch it --
    frame, first item, one past the last, x and y of the top left pixel of the area the frame's items cover (the union of their
    clipped extents), 64-pixel tiles per row of that area, the 64 x 4 tiles of all rows before, 0 -- and the number of tiles in all.
    `items` are checked (`check_items`) and sorted by frame."""
    if not len(items):
        return np.zeros((0, 8), dtype=np.int32), 0
    ex0, ey0, ex1, ey1 = extents(items, table)
    cx0, cy0 = np.maximum(ex0, 0), np.maximum(ey0, 0)
    cx1, cy1 = np.minimum(ex1, width - 1), np.minimum(ey1, height - 1)
    dead = (cx0 > cx1) | (cy0 > cy1)
    cx0, cy0 = np.where(dead, width, cx0), np.where(dead, height, cy0)
    cx1, cy1 = np.where(dead, -1, cx1), np.where(dead, -1, cy1)
    f = items["frame"]
    starts = np.flatnonzero(np.concatenate([[True], f[1:] != f[:-1]]))
    ends = np.concatenate([starts[1:], [len(f)]])
    ux0, uy0 = np.minimum.reduceat(cx0, starts), np.minimum.reduceat(cy0, starts)
    ux1, uy1 = np.maximum.reduceat(cx1, starts), np.maximum.reduceat(cy1, starts)
    live = (ux0 <= ux1) & (uy0 <= uy1)
    starts, ends, ux0, uy0, ux1, uy1 = (v[live] for v in (starts, ends, ux0, uy0, ux1, uy1))
    tiles_x = (ux1 - ux0) // TILE_W + 1
    tiles = tiles_x * ((uy1 - uy0) // TILE_H + 1)
    total = int(tiles.sum())
    if total >= 1 << 31:
        raise ValueError(f"{total} tiles of {TILE_W} x {TILE_H} pixels in one call: draw fewer frames per call")
    work = np.zeros((len(starts), 8), dtype=np.int32)
    work[:, 0], work[:, 1], work[:, 2] = f[starts], starts, ends
    work[:, 3], work[:, 4], work[:, 5] = ux0, uy0, tiles_x
    work[:, 6] = np.cumsum(tiles) - tiles
    return work, total


def _blend(dst, cov, ink):
    """PIL's BLEND8 on int arrays: the sum rounded once, the shift form of / 255."""
    t = dst * (255 - cov) + ink * cov + 128
    return ((t >> 8) + t) >> 8


def _coverage(it, x, y, flat, table):
    """Coverage 0..255 of the pixels (x [1, w], y [h, 1], int64) by one item: csrc/annotate.hip item_coverage, line for line."""
    x0, y0, x1, y1, a = (int(it[f]) for f in ("x0", "y0", "x1", "y1", "arg"))
    kind = int(it["kind"])
    if kind == OUTLINE:
        rows = (x >= x0) & (x <= x1) & (((y >= y0) & (y <= y0 + a - 1)) | ((y >= y1 - a + 1) & (y <= y1)))
        p, q = y0 + a, y1 - a + 1
        lo, hi = (p, q - 1) if p < q else (q + 1, p)
        cols = (((x >= x0) & (x <= x0 + a - 1)) | ((x >= x1 - a + 1) & (x <= x1))) & (y >= lo) & (y <= hi)
        return np.where(rows | cols, 255, 0)
    if kind == FILL:
        return np.where((x >= x0) & (x <= x1) & (y >= y0) & (y <= y1), a, 0)
    off, w, h = (int(v) for v in table[int(it["mask"])])
    dx, dy = x - x0, y - y0
    inside = (dx >= 0) & (dy >= 0) & (dx < a * w) & (dy < a * h)
    src = off + np.clip(dy // a, 0, h - 1) * w + np.clip(dx // a, 0, w - 1)
    return np.where(inside, flat[src].astype(np.int64), 0)


def draw_numpy(frames: np.ndarray, items, masks=()):
    """The CPU statement of avcer_annotate_frames: draws `items` into `frames` (uint8 [n, H, W, 3], IN PLACE) one after another and
    returns `frames`.  Pure numpy, the kernel's integer arithmetic; `masks`: a list of u8 [h, w] arrays, or `pack_masks`' pair."""
    if not (isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3):
        raise ValueError("frames must be a uint8 [n, H, W, 3] array")
    items = as_items(items)
    flat, table = pack_masks(masks)
    n, height, width = frames.shape[:3]
    check_items(items, n, table, len(flat))
    ex0, ey0, ex1, ey1 = extents(items, table)
    for i, it in enumerate(items):
        ax, bx = max(int(ex0[i]), 0), min(int(ex1[i]), width - 1)
        ay, by = max(int(ey0[i]), 0), min(int(ey1[i]), height - 1)
        if ax > bx or ay > by:
            continue
        x = np.arange(ax, bx + 1, dtype=np.int64)[None, :]
        y = np.arange(ay, by + 1, dtype=np.int64)[:, None]
        cov = _coverage(it, x, y, flat, table)[:, :, None]
        view = frames[int(it["frame"]), ay:by + 1, ax:bx + 1]
        ink = it["colour"].astype(np.int64)[None, None, :]
        view[...] = np.where(cov > 0, _blend(view.astype(np.int64), cov, ink), view).astype(np.uint8)
    return frames


def draw(engine, frames, items, masks=()):
    """`draw_numpy` on the device: frames uint8 [n, H, W, 3] on the device, drawn IN PLACE by avcer_annotate_frames and returned.
    `masks` as draw_numpy takes them, or (u8 tensor already on the device, table)."""
    flat, table = masks if _is_device_pair(masks) else pack_masks(masks)
    return engine.annotate(frames, items, flat, table)


def _is_device_pair(masks):
    return isinstance(masks, tuple) and len(masks) == 2 and hasattr(masks[0], "is_cuda")


# ---------------------------------------------------------------------------------------------------- labels
class LabelMasks:
    """Text masks of one PIL font, rendered once: get(text) -> (u8 [h, w] coverage of `font.getmask(text, "L")`, the row of its
    first line below the text's origin (`font.getbbox(text)[1]`), the text's advance in pixels (`round(font.getlength(text))`))."""

    def __init__(self, font):
        self.font = font
        self._cache = {}

    def get(self, text: str):
        hit = self._cache.get(text)
        if hit is None:
            m = self.font.getmask(text, "L")
            w, h = m.size
            if w <= 0 or h <= 0:
                raise ValueError(f"the font renders {text!r} as an empty mask")
            a = np.array(m, dtype=np.uint8).reshape(h, w)
            hit = self._cache[text] = (a, int(self.font.getbbox(text)[1]), int(round(self.font.getlength(text))))
        return hit

    def __len__(self):
        return len(self._cache)


_LABEL_CACHES = {}  # id(font) -> (font, LabelMasks); default fonts by size


def line_width(height: int, width: int) -> int:
    """get_visualization.py:46: lw = max(round(sum(frame.shape) / 2 * 0.003), 2) with frame.shape = (H, W, 3)."""
    return max(round((height + width + 3) / 2 * 0.003), 2)


def default_font(lw: int):
    from PIL import ImageFont

    key = ("default", 11 * max(lw - 1, 1))
    if key not in _LABEL_CACHES:
        font = ImageFont.load_default(size=key[1])
        _LABEL_CACHES[key] = (font, LabelMasks(font))
    return _LABEL_CACHES[key][0]


def label_masks(font) -> LabelMasks:
    """The cache of `font`'s text masks, kept across calls: a label is its name part (COMPOUND_NAMES[c] + ": ", seven strings) and
    its number part ("%.2f%%", at most 10 001 strings) rendered separately, so after warm-up no frame costs any font work."""
    for f, cache in _LABEL_CACHES.values():
        if f is font:
            return cache
    _LABEL_CACHES[id(font)] = (font, LabelMasks(font))
    return _LABEL_CACHES[id(font)][1]


def layout(records, pred, prob, height: int, width: int, font=None, panel: bool = False):
    """The drawing of a whole video -> (items ITEM [m] sorted by frame, masks: list of u8 arrays).

    records int64 [r, 6] = frame, track, x0, y0, x1, y1 (face_tiles.VideoTiler); pred int [T] and prob [T, 7]: the chosen model's
    compound class and probabilities per frame.  With lw = line_width(H, W), per frame t in this order:

    1. panel=True, first: a FILL of BLACK, coverage 160, over (0, 0, pw-1, ph-1); then per class c = 0..6 the mask of
       COMPOUND_NAMES[c] + ": " in WHITE at (lw, lw + c*rh + top_c) and, when L = round(prob[t, c] * bar_w) >= 1, an opaque FILL
       (lw + nw, lw + c*rh + 1, lw + nw + L - 1, lw + c*rh + rh - 2) in MAGENTA for c = pred[t], else WHITE.  nw = the largest advance
       of the seven names, rh = the largest (top + mask height) of the seven + 2, bar_w = max(W // 8, 8), pw = nw + bar_w + 3*lw,
       ph = 7*rh + 2*lw.  Frames at or past len(pred) get no panel.
    2. every record of frame t, in record order: OUTLINE (x0, y0, x1, y1) inclusive, MAGENTA, width lw.
    3. for the record of track 0, when t < len(pred): the label "<name>: " + "%.2f%%" % (prob[t, pred[t]] * 100).  Name and number are
       two masks side by side: tw = advance(name) + width(number mask), th = max(top + mask height) of the two.  The backdrop is
       bw = tw + 2*lw by bh = th + 2*lw; bx = x0 + (x1 - x0 + 1)//2 - bw//2, moved into [0, W - bw] when the frame is wide enough
       (else 0); by = y0 - bh, above the box, or y0 + lw, inside under the top border, when y0 - bh < 0.  Items: FILL (bx, by,
       bx+bw-1, by+bh-1) BLACK coverage 160; MASK name at (bx + lw, by + lw + top_name); MASK number at (bx + lw + advance(name),
       by + lw + top_number); both MAGENTA, scale 1.
    In this positional form (pred, prob arrays) tracks other than 0 get their box and no label.  Each distinct mask appears once in
    `masks`.

    Per-track form: `pred` and `prob` are dicts {track directory: pred int [T]} / {track directory: prob [T, 7]} with the same
    keys.  Every record of a track in the dict gets, behind its own box, the label of step 3 from that track's arrays; the other
    tracks keep a bare box; the panel of step 1 shows the dict's FIRST track.  The positional form is the dict {0: ...}."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, 6)
    if isinstance(pred, dict) != isinstance(prob, dict):
        raise ValueError("layout: pred and prob are both arrays (track 00) or both dicts keyed by track")
    if not isinstance(pred, dict):
        pred, prob = {0: pred}, {0: prob}
    if not pred or list(pred) != list(prob):
        raise ValueError("layout: pred and prob need the same tracks in the same order, at least one")
    by_track = {}
    for k in pred:
        p = np.asarray(pred[k]).reshape(-1)
        by_track[int(k)] = (p, np.asarray(prob[k], dtype=np.float64).reshape(len(p), -1))
    pred, prob = next(iter(by_track.values()))  # the panel's
    lw = line_width(height, width)
    cache = label_masks(default_font(lw) if font is None else font)
    masks, index = [], {}

    def use(text):
        a, top, adv = cache.get(text)
        if text not in index:
            index[text] = len(masks)
            masks.append(a)
        return index[text], a, top, adv

    names = [use(n + ": ") for n in COMPOUND_NAMES]
    nw = max(n[3] for n in names)
    rh = max(n[2] + n[1].shape[0] for n in names) + 2
    bar_w = max(width // 8, 8)
    out = []
    order = np.argsort(records[:, 0], kind="stable")
    by_frame = {}
    for r in records[order]:
        by_frame.setdefault(int(r[0]), []).append(r)
    frames = sorted(set(by_frame) | (set(range(len(pred))) if panel else set()))
    for t in frames:
        if panel and t < len(pred):
            out.append(fill(t, (0, 0, nw + bar_w + 3 * lw - 1, 7 * rh + 2 * lw - 1), BLACK, BACKDROP))
            for c, (j, a, top, adv) in enumerate(names):
                out.append(mask(t, (lw, lw + c * rh + top), WHITE, j))
                length = int(round(float(prob[t, c]) * bar_w))
                if length >= 1:
                    out.append(fill(t, (lw + nw, lw + c * rh + 1, lw + nw + length - 1, lw + c * rh + rh - 2),
                                    MAGENTA if c == int(pred[t]) else WHITE))
        for r in by_frame.get(t, ()):
            x0, y0, x1, y1 = (int(v) for v in r[2:6])
            out.append(outline(t, (x0, y0, x1, y1), MAGENTA, lw))
            tpred, tprob = by_track.get(int(r[1]), ((), None))
            if t >= len(tpred):
                continue
            c = int(tpred[t])
            jn, an, topn, advn = names[c]
            jp, ap, topp, _ = use("%.2f%%" % (float(tprob[t, c]) * 100))
            tw, th = advn + ap.shape[1], max(topn + an.shape[0], topp + ap.shape[0])
            bw, bh = tw + 2 * lw, th + 2 * lw
            bx = x0 + (x1 - x0 + 1) // 2 - bw // 2
            bx = min(max(bx, 0), width - bw) if bw <= width else 0
            by = y0 - bh if y0 - bh >= 0 else y0 + lw
            out.append(fill(t, (bx, by, bx + bw - 1, by + bh - 1), BLACK, BACKDROP))
            out.append(mask(t, (bx + lw, by + lw + topn), MAGENTA, jn))
            out.append(mask(t, (bx + lw + advn, by + lw + topp), MAGENTA, jp))
    return as_items(out) if out else np.zeros(0, dtype=ITEM), masks


def write_result_video(engine, frames, records, pred, prob, path, rate, scale=1, pcm=None, audio_rate=44100, quality=90, subsampling=2,
                       entropy="device", frames_per_pass=64, bgr=True, font=None, panel=False, tracks=None, opendml=False,
                       segment_bytes=1 << 30):
    """The result video of `frames` (uint8 [T, H, W, 3], on the device or moved there; BGR unless bgr=False) as the Motion-JPEG AVI
    file `path` at `rate` / `scale` frames per second, with `pcm` (int16 [L] / [L, C] at `audio_rate`) as its sound: `layout(records,
    pred, prob, H, W, font, panel)` drawn on every frame.  `frames` may also be a frame SOURCE -- a callable returning an iterator, or
    an iterator, of device passes uint8 [k, H, W, 3] in frame order (run_inference_file's streamed call decodes the file a second
    time this way) -- so that the video never has to exist as one tensor; the file is the same.  In passes of `frames_per_pass`:
    the pass is copied into a scratch buffer of the engine (the caller's frames are never modified), drawn there (`draw`), encoded
    as whole-frame rectangles (jpeg._plan_to_device / Engine.jpeg_forward / jpeg.files_from_coeffs: the files are PIL's
    `save(quality=quality, subsampling=subsampling)` of the drawn frames, byte for byte, under both `entropy` values) and appended
    to the file (avi.AviWriter; the header is patched at the end).  The device holds one pass of copies and coefficients at a time;
    only file bytes cross to the host, and the host keeps the index alone.  What AviWriter refuses (a file past 4 GiB: OSError)
    propagates, and no partial file is left, whatever the failure.  `opendml=True`: the OpenDML layout in segments of
    `segment_bytes` (avi.AviWriter), which may pass 4 GiB; False (the default): the plain file, byte for byte as ever.
    `tracks`: None -- `pred` / `prob` are arrays and label track 00 (or dicts, taken as they are: `layout`) --, "all" or a list of
    track directories (face_tiles.check_tracks): `pred` and `prob` are then dicts keyed by track, and the tracks named ("all": every
    key, ascending) are labelled, each from its own arrays; the panel shows the first.  A named track the dicts do not hold raises
    ValueError before any work.  Returns `path`."""
    import torch

    from . import jpeg
    from .avi import AviWriter
    from .face_tiles import check_tracks

    tracks = check_tracks(tracks)
    if tracks is not None:
        if not (isinstance(pred, dict) and isinstance(prob, dict)):
            raise ValueError("write_result_video: with tracks=, pred and prob are dicts keyed by track")
        keys = tuple(sorted(pred)) if tracks == "all" else tracks
        missing = [k for k in keys if k not in pred or k not in prob]
        if missing or not keys:
            raise ValueError(f"write_result_video: no prediction for track {missing[0]:02d}" if missing else "write_result_video: no track")
        pred, prob = {k: pred[k] for k in keys}, {k: prob[k] for k in keys}
    jpeg._check_entropy(entropy)
    if int(frames_per_pass) < 1:
        raise ValueError("frames_per_pass must be at least 1")
    if callable(frames) or (hasattr(frames, "__next__") and not torch.is_tensor(frames)):
        source, whole = iter(frames() if callable(frames) else frames), False
    else:
        src = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        if src.dim() != 4 or src.shape[-1] != 3 or src.dtype != torch.uint8:
            raise ValueError("frames must be uint8 [T, H, W, 3]")
        source, whole = iter((src,)), True
    writer, state, lo = None, None, 0
    try:
        for part in source:
            if part.dim() != 4 or part.shape[-1] != 3 or part.dtype != torch.uint8:
                raise ValueError("frames must be uint8 [T, H, W, 3]")
            if state is None:
                height, width = int(part.shape[1]), int(part.shape[2])
                items, masks = layout(records, pred, prob, height, width, font, panel)
                flat, table = pack_masks(masks)
                # a source's length is not known in front: its items are held to the last frame they name
                check_items(items, max(int(part.shape[0]), 1) if whole else int(items["frame"].max()) + 1 if len(items) else 1, table, len(flat))
                state = (items, torch.from_numpy(flat).to(engine.device), table)
                writer = AviWriter(path, width, height, rate, scale, audio_rate, pcm=pcm,
                                   **(dict(opendml=True, segment_bytes=segment_bytes) if opendml else {}))
            elif (int(part.shape[1]), int(part.shape[2])) != (height, width):
                raise ValueError(f"a pass of {int(part.shape[2])} x {int(part.shape[1])} frames behind {width} x {height}")
            items, flat_d, table = state
            per = height * width * 3
            fpp = min(int(frames_per_pass), max(int(part.shape[0]), 1))
            scratch = engine.__dict__.get("_annotate_scratch")
            if scratch is None or scratch.numel() < fpp * per:
                scratch = engine.__dict__["_annotate_scratch"] = torch.empty(fpp * per, dtype=torch.uint8, device=engine.device)
            for at in range(0, int(part.shape[0]), fpp):
                k = min(fpp, int(part.shape[0]) - at)
                buf = scratch[:k * per].view(k, height, width, 3)
                buf.copy_(part[at:at + k], non_blocking=True)
                sel = items[(items["frame"] >= lo) & (items["frame"] < lo + k)].copy()
                sel["frame"] -= lo
                engine.annotate(buf, sel, flat_d, table)
                rects = np.zeros((k, 5), dtype=np.int32)
                rects[:, 0], rects[:, 3], rects[:, 4] = np.arange(k), width, height
                src_d, r_dev, d_dev, host, n, blocks, _ = jpeg._plan_to_device(engine, buf, rects, quality, subsampling)
                coeffs = engine.jpeg_forward(src_d, r_dev, d_dev, n, blocks, bgr=bgr)
                writer.add_frames(jpeg.files_from_coeffs(engine, coeffs, d_dev, host, 0, entropy))
                del coeffs
                lo += k
            del part
        if writer is None:
            raise ValueError("write_avi: no frame")
        return writer.close()
    except BaseException:
        if writer is not None:
            writer.__exit__(Exception)
        raise
