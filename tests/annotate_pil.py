"""The PIL side of the drawing tests: an item list redrawn with ImageDraw, and the shared cases of tests/test_annotate_cpu.py and
tests/test_gpu_annotate.py (one statement of the shapes at which the drawing can go wrong)."""
import numpy as np
from PIL import Image, ImageDraw

from avcer_amd import annotate as an


def draw_pil(frames, items, masks=()):
    """A copy of `frames` (uint8 [n, H, W, 3]) with `items` drawn by ImageDraw, one call per item, in list order."""
    items = an.as_items(items)
    out = []
    per_frame = {}
    for it in items:
        per_frame.setdefault(int(it["frame"]), []).append(it)
    for f in range(len(frames)):
        im = Image.fromarray(frames[f].copy())
        d = ImageDraw.Draw(im)
        for it in per_frame.get(f, ()):
            colour = tuple(int(c) for c in it["colour"])
            x0, y0, x1, y1, a = (int(it[k]) for k in ("x0", "y0", "x1", "y1", "arg"))
            if it["kind"] == an.OUTLINE:
                d.rectangle((x0, y0, x1, y1), outline=colour, width=a)
            elif it["kind"] == an.FILL:
                d.bitmap((x0, y0), Image.new("L", (x1 - x0 + 1, y1 - y0 + 1), a), fill=colour)
            else:
                m = Image.fromarray(np.ascontiguousarray(masks[int(it["mask"])]))
                d.bitmap((x0, y0), m.resize((a * m.width, a * m.height), Image.NEAREST), fill=colour)
        out.append(np.array(im))
    return np.stack(out) if out else frames.copy()


def small_case(seed=0):
    """Random frames [3, 37, 53, 3] (a frame is 5883 bytes: frames 1 and 2 start at odd addresses), two masks, and every kind of
    item in every position the issue lists; frame 1 has no item.  Returns (frames, items, masks)."""
    rng = np.random.default_rng(seed)
    h, w = 37, 53
    frames = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    masks = [rng.integers(0, 256, (5, 7), dtype=np.uint8), rng.integers(0, 256, (9, 4), dtype=np.uint8)]
    masks[0][0, 0], masks[0][4, 6], masks[1][0, 0] = 255, 0, 1
    c = lambda: tuple(int(v) for v in rng.integers(0, 256, 3))
    items = []
    for f in (0, 2):
        items += [
            an.outline(f, (-4, 5, 6, 12), c(), 2),           # crosses the left edge
            an.outline(f, (45, 3, 60, 9), c(), 1),           # right
            an.outline(f, (10, -3, 20, 4), c(), 3),          # top
            an.outline(f, (30, 30, 40, 44), c(), 2),         # bottom
            an.outline(f, (-20, -20, -5, -5), c(), 2),       # wholly outside
            an.outline(f, (60, 10, 70, 20), c(), 2),
            an.outline(f, (25, 12, 25, 12), c(), 1),         # 1 x 1
            an.outline(f, (14, 14, 19, 17), c(), 2),         # 2t = the height
            an.outline(f, (22, 20, 24, 30), c(), 2),         # 2t > the width
            an.outline(f, (34, 12, 40, 14), c(), 5),         # t > the height: PIL's rows leave the box
            an.outline(f, (0, 0, w - 1, h - 1), c(), 1),     # the frame's own border
            an.fill(f, (-3, 20, 8, 28), c(), 160),
            an.fill(f, (48, 30, 70, 50), c(), 255),
            an.fill(f, (5, 5, 5, 5), c(), 1),
            an.fill(f, (100, 100, 120, 120), c(), 77),       # wholly outside
        ]
        for k in (1, 2, 3):
            items += [an.mask(f, (-3 * k, 8 + k), c(), 0, k), an.mask(f, (w - 4 * k, 2), c(), 0, k), an.mask(f, (20, -2 * k), c(), 1, k),
                      an.mask(f, (12 * k, h - 3 * k), c(), 1, k), an.mask(f, (-100, -100), c(), 0, k)]
    return frames, an.as_items(sorted(items, key=lambda r: r[0])), masks


def overlap_orders():
    """Three items deep on the same pixels, in two orders that must give different pictures: (frames, masks, order a, order b)."""
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (1, 37, 53, 3), dtype=np.uint8)
    masks = [rng.integers(1, 256, (6, 6), dtype=np.uint8)]
    a = [an.fill(0, (10, 8, 30, 25), (200, 10, 90), 160), an.mask(0, (12, 10), (0, 255, 30), 0, 3), an.outline(0, (8, 6, 26, 20), (255, 0, 255), 3)]
    return frames, masks, a, a[::-1]


def random_items(rng, n_frames, h, w, per_frame, n_masks):
    """`per_frame` random items on every frame, heavily overlapping, sorted by frame."""
    items = []
    for f in range(n_frames):
        for _ in range(per_frame):
            kind = int(rng.integers(0, 3))
            colour = tuple(int(v) for v in rng.integers(0, 256, 3))
            x0, y0 = int(rng.integers(-20, w)), int(rng.integers(-20, h))
            if kind == an.MASK:
                items.append(an.mask(f, (x0, y0), colour, int(rng.integers(0, n_masks)), int(rng.integers(1, 5))))
                continue
            box = (x0, y0, x0 + int(rng.integers(0, 90)), y0 + int(rng.integers(0, 70)))
            items.append(an.outline(f, box, colour, int(rng.integers(1, 7))) if kind == an.OUTLINE else
                         an.fill(f, box, colour, int(rng.integers(1, 256))))
    return an.as_items(items)
