"""The result video's drawing on the CPU: annotate.draw_numpy against PIL's ImageDraw with tolerance zero, the blend settled
exhaustively, the layout's pixel rules pinned through PIL, the launch plan, and every refusal."""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image, ImageDraw, ImageFont

from annotate_pil import draw_pil, overlap_orders, random_items, small_case
from avcer_amd import _lib, build
from avcer_amd import annotate as an
from avcer_amd.fusion import COMPOUND_NAMES


def test_draw_numpy_equals_pil_on_every_kind_at_every_edge():
    frames, items, masks = small_case()
    assert {int(k) for k in items["kind"]} == {an.OUTLINE, an.FILL, an.MASK} and 1 not in items["frame"]
    want = draw_pil(frames, items, masks)
    got = an.draw_numpy(frames.copy(), items, masks)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[1], frames[1])                       # the frame without items
    assert (got[0] != frames[0]).any() and (got[2] != frames[2]).any()
    # one item at a time: a wrong kind cannot hide behind a later item
    for i in range(len(items)):
        one = items[i:i + 1]
        np.testing.assert_array_equal(an.draw_numpy(frames.copy(), one, masks), draw_pil(frames, one, masks), err_msg=str(one))


def test_an_empty_list_draws_nothing_and_draw_numpy_works_in_place():
    frames, items, masks = small_case(1)
    work = frames.copy()
    assert an.draw_numpy(work, [], masks) is work
    np.testing.assert_array_equal(work, frames)
    np.testing.assert_array_equal(an.draw_numpy(work, np.zeros(0, dtype=an.ITEM)), frames)
    assert an.draw_numpy(work, items, masks) is work and (work != frames).any()


def test_outline_of_every_small_box_and_width_equals_pil():
    """PIL's outline, exhaustively where its rules meet: sides 1..7, widths 1..6, at a corner of the frame and inside it."""
    base = np.full((1, 16, 18, 3), 9, dtype=np.uint8)
    for x0, y0 in ((-2, -3), (4, 5), (13, 11)):
        items = []
        for w in range(1, 8):
            for h in range(1, 8):
                for t in range(1, 7):
                    items.append(an.outline(0, (x0, y0, x0 + w - 1, y0 + h - 1), (255, 0, 255), t))
        for it in items:
            np.testing.assert_array_equal(an.draw_numpy(base.copy(), [it]), draw_pil(base, [it]), err_msg=str(it))


def test_overlaps_three_deep_depend_on_the_order_as_in_pil():
    frames, masks, a, b = overlap_orders()
    ga, gb_ = an.draw_numpy(frames.copy(), a, masks), an.draw_numpy(frames.copy(), b, masks)
    np.testing.assert_array_equal(ga, draw_pil(frames, a, masks))
    np.testing.assert_array_equal(gb_, draw_pil(frames, b, masks))
    assert (ga != gb_).any()
    rng = np.random.default_rng(3)
    masks = [rng.integers(0, 256, (5, 9), dtype=np.uint8), rng.integers(0, 256, (8, 3), dtype=np.uint8)]
    frames = rng.integers(0, 256, (2, 40, 64, 3), dtype=np.uint8)
    items = random_items(rng, 2, 40, 64, 40, 2)
    np.testing.assert_array_equal(an.draw_numpy(frames.copy(), items, masks), draw_pil(frames, items, masks))


@pytest.mark.parametrize("ink", [0, 1, 127, 128, 254, 255])
def test_blend_equals_pil_for_every_destination_and_coverage(ink):
    """BLEND8, exhaustively: destination 0..255 down the rows, coverage 0..255 along the columns.  The sum is rounded once; rounding
    each product on its own differs for every ink but 0 and 255."""
    dst = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    cov = np.ascontiguousarray(dst.T)
    colour = (ink, 255 - ink, ink ^ 85)
    im = Image.fromarray(np.stack([dst] * 3, axis=-1))
    ImageDraw.Draw(im).bitmap((0, 0), Image.fromarray(cov), fill=colour)
    frames = np.stack([dst] * 3, axis=-1)[None].copy()
    got = an.draw_numpy(frames, [an.mask(0, (0, 0), colour, 0, 1)], [cov])
    np.testing.assert_array_equal(got[0], np.array(im))
    d, c = dst.astype(np.int64), cov.astype(np.int64)
    md = lambda a, b: (((a * b + 128) >> 8) + a * b + 128) >> 8
    each = md(d, 255 - c) + md(np.int64(ink), c)
    assert (each == got[0, :, :, 0]).all() == (ink in (0, 255))


# ---------------------------------------------------------------------------------------------------- layout
H, W = 120, 200


def video():
    """Four frames: track 0 in frames 0, 1, 3 (touching the top in frame 1), a second track in frames 0 and 2."""
    records = np.array([[0, 0, 60, 50, 130, 100], [0, 1, 5, 60, 40, 110], [1, 0, 70, 0, 150, 70], [2, 1, 150, 40, 210, 90],
                        [3, 0, 2, 70, 30, 119]], dtype=np.int64)
    prob = np.random.default_rng(5).dirichlet(np.ones(7), size=4)
    pred = prob.argmax(axis=1).astype(np.int32)
    return records, pred, prob


def test_layout_redrawn_by_pil_equals_draw_numpy():
    records, pred, prob = video()
    frames = np.random.default_rng(6).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    for panel in (False, True):
        items, masks = an.layout(records, pred, prob, H, W, panel=panel)
        assert (np.diff(items["frame"]) >= 0).all()
        np.testing.assert_array_equal(an.draw_numpy(frames.copy(), items, masks), draw_pil(frames, items, masks))


def test_layout_places_boxes_and_labels_by_its_rules():
    records, pred, prob = video()
    lw = an.line_width(H, W)
    assert lw == max(round((H + W + 3) / 2 * 0.003), 2) == 2 and an.line_width(1080, 1920) == 5
    items, masks = an.layout(records, pred, prob, H, W)
    per = lambda f: items[items["frame"] == f]
    # every record has its box, inclusive corners, magenta, width lw
    boxes = items[items["kind"] == an.OUTLINE]
    assert [tuple(int(b[k]) for k in ("frame", "x0", "y0", "x1", "y1")) for b in boxes] == [tuple(int(v) for v in r[[0, 2, 3, 4, 5]]) for r in records]
    assert (boxes["arg"] == lw).all() and (boxes["colour"] == an.MAGENTA).all()
    # frame 0: two boxes, one label (track 0's): backdrop, name, number, above the box and centred on it
    f0 = per(0)
    assert [int(k) for k in f0["kind"]] == [an.OUTLINE, an.FILL, an.MASK, an.MASK, an.OUTLINE]
    back, name, number = f0[1], f0[2], f0[3]
    assert int(back["arg"]) == 160 and tuple(back["colour"]) == an.BLACK and tuple(name["colour"]) == tuple(number["colour"]) == an.MAGENTA
    font = an.default_font(lw)
    assert font.size == 11 * max(lw - 1, 1)
    text_n, text_p = COMPOUND_NAMES[pred[0]] + ": ", "%.2f%%" % (prob[0, pred[0]] * 100)
    np.testing.assert_array_equal(masks[int(name["mask"])], np.array(font.getmask(text_n, "L"), dtype=np.uint8).reshape(masks[int(name["mask"])].shape))
    mp = font.getmask(text_p, "L")
    assert masks[int(number["mask"])].shape == (mp.size[1], mp.size[0])
    adv = round(font.getlength(text_n))
    bw, bh = int(back["x1"] - back["x0"] + 1), int(back["y1"] - back["y0"] + 1)
    assert bw == adv + mp.size[0] + 2 * lw and int(back["y1"]) == 50 - 1 and int(back["y0"]) == 50 - bh
    assert int(back["x0"]) == 60 + (130 - 60 + 1) // 2 - bw // 2
    assert (int(name["x0"]), int(number["x0"])) == (int(back["x0"]) + lw, int(back["x0"]) + lw + adv)
    assert int(name["y0"]) == int(back["y0"]) + lw + font.getbbox(text_n)[1]
    # frame 1: the box touches the top, the label goes inside under the top border
    f1 = per(1)
    assert int(f1[1]["y0"]) == 0 + lw and int(f1[1]["kind"]) == an.FILL
    # frame 2: only another track: a box and no label; frame 3: the label is moved into the frame on the left
    assert [int(k) for k in per(2)["kind"]] == [an.OUTLINE]
    assert int(per(3)[1]["x0"]) == 0
    # a frame past the predictions gets its box and no label
    late, _ = an.layout(np.array([[9, 0, 10, 40, 50, 80]]), pred, prob, H, W)
    assert [int(k) for k in late["kind"]] == [an.OUTLINE]


def test_panel_adds_exactly_its_items():
    records, pred, prob = video()
    plain, _ = an.layout(records, pred, prob, H, W)
    items, masks = an.layout(records, pred, prob, H, W, panel=True)
    lw = an.line_width(H, W)
    bar_w = max(W // 8, 8)
    for f in range(4):
        a, b = plain[plain["frame"] == f], items[items["frame"] == f]
        bars = sum(1 for c in range(7) if round(float(prob[f, c]) * bar_w) >= 1)
        extra = 1 + 7 + bars
        assert len(b) == len(a) + extra
        np.testing.assert_array_equal(b[extra:], a)                     # the plain drawing follows, unchanged
        assert int(b[0]["kind"]) == an.FILL and (int(b[0]["x0"]), int(b[0]["y0"]), int(b[0]["arg"])) == (0, 0, 160)
        names = b[1:extra][b[1:extra]["kind"] == an.MASK]
        assert len(names) == 7 and (names["x0"] == lw).all()
        fills = b[1:extra][b[1:extra]["kind"] == an.FILL]
        lengths = {int(r["y0"]): int(r["x1"] - r["x0"] + 1) for r in fills}
        assert sorted(lengths.values()) == sorted(round(float(p) * bar_w) for p in prob[f] if round(float(p) * bar_w) >= 1)
        assert sum((fills["colour"] == an.MAGENTA).all(axis=1)) == 1
    assert len(masks) <= 7 + 3


def test_label_masks_are_cached_per_font():
    font = ImageFont.load_default(size=13)
    cache = an.label_masks(font)
    assert an.label_masks(font) is cache and an.label_masks(ImageFont.load_default(size=13)) is not cache
    a = cache.get("12.34%")
    assert cache.get("12.34%") is a and len(cache) == 1
    records, pred, prob = video()
    items, masks = an.layout(records, pred, prob, H, W, font=font)
    assert len(cache) == 1 + 7 + 3 and len(masks) == 7 + 3
    an.layout(records, pred, prob, H, W, font=font)
    assert len(cache) == 1 + 7 + 3


# ---------------------------------------------------------------------------------------------------- the launch plan
def test_work_table_covers_every_touched_pixel_and_no_other_frame():
    frames, items, masks = small_case()
    flat, table = an.pack_masks(masks)
    n, h, w = frames.shape[:3]
    work, tiles = an.work_table(items, table, n, h, w)
    assert work.dtype == np.int32 and work.shape == (2, 8) and list(work[:, 0]) == [0, 2]
    drawn = an.draw_numpy(frames.copy(), items, masks)
    at = 0
    for f, lo, hi, x0, y0, tx, first, _ in work:
        assert first == at and (items["frame"][lo:hi] == f).all() and (lo == 0 or items["frame"][lo - 1] != f)
        ys, xs = np.nonzero((drawn[f] != frames[f]).any(axis=2))
        assert x0 <= xs.min() and y0 <= ys.min() and xs.max() < x0 + tx * an.TILE_W and x0 >= 0 and y0 >= 0
        at += tx * ((min(h - 1, ys.max()) - y0) // an.TILE_H + 1)
    assert tiles >= at and tiles <= 2 * ((w + 63) // 64) * ((h + 3) // 4)
    # items that miss their frame altogether plan nothing
    off = [an.outline(0, (-30, -30, -10, -10), (1, 2, 3), 2), an.mask(1, (w, 0), (1, 2, 3), 0, 2)]
    work, tiles = an.work_table(an.as_items(off), table, n, h, w)
    assert len(work) == 0 and tiles == 0


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("item,match", [
    (an.outline(3, (1, 1, 5, 5), (1, 2, 3), 1), r"item 1 \(OUTLINE\): frame 3 outside \[0, 3\)"),
    (an.fill(-1, (1, 1, 5, 5), (1, 2, 3), 9), r"item 1 \(FILL\): frame -1"),
    (an.outline(2, (6, 1, 5, 5), (1, 2, 3), 1), r"item 1 \(OUTLINE\).*x1 < x0"),
    (an.fill(2, (1, 6, 5, 5), (1, 2, 3), 9), r"item 1 \(FILL\).*y1 < y0"),
    (an.outline(2, (1, 1, 5, 5), (1, 2, 3), 0), r"item 1 \(OUTLINE\): width 0"),
    (an.fill(2, (1, 1, 5, 5), (1, 2, 3), 0), r"item 1 \(FILL\): coverage 0 outside 1..255"),
    (an.fill(2, (1, 1, 5, 5), (1, 2, 3), 256), r"item 1 \(FILL\): coverage 256"),
    (an.mask(2, (1, 1), (1, 2, 3), 2, 1), r"item 1 \(MASK\): mask index 2 outside \[0, 2\)"),
    (an.mask(2, (1, 1), (1, 2, 3), -1, 1), r"item 1 \(MASK\): mask index -1"),
    (an.mask(2, (1, 1), (1, 2, 3), 0, 0), r"item 1 \(MASK\): scale 0"),
    (an.mask(2, (1, 1), (1, 2, 3), 0, an.SCALE_MAX + 1), r"item 1 \(MASK\): scale 65"),
    (an.fill(2, (1, 1, 5, 5), (1, 256, 3), 9), r"item 1 \(FILL\): colour"),
    ((2, 7, 1, 1, 5, 5, 1, 0, (1, 2, 3), 0), r"item 1 \(\?\): kind 7"),
    (an.fill(0, (1, 1, 5, 5), (1, 2, 3), 9), r"item 1 \(FILL\): frame 0 behind frame 1.*sorted"),
])
def test_refusals_name_the_item(item, match):
    frames, _, masks = small_case()
    good = an.outline(1, (1, 1, 5, 5), (1, 2, 3), 1)
    before = frames.copy()
    with pytest.raises(ValueError, match=match):
        an.draw_numpy(frames, [good, item], masks)
    np.testing.assert_array_equal(frames, before)                          # refused before anything is drawn
    flat, table = an.pack_masks(masks)
    with pytest.raises(ValueError, match=match):
        an.check_items(an.as_items([good, item]), 3, table, len(flat))


def test_mask_tables_and_frames_are_checked():
    with pytest.raises(ValueError, match="mask 1"):
        an.pack_masks([np.zeros((2, 2), dtype=np.uint8), np.zeros((2, 2), dtype=np.float32)])
    with pytest.raises(ValueError, match="mask 0"):
        an.pack_masks([np.zeros((0, 2), dtype=np.uint8)])
    with pytest.raises(ValueError, match="mask 1: offset 4, 3 x 3 leaves the mask buffer of 12 bytes"):
        an.check_items(np.zeros(0, dtype=an.ITEM), 1, np.array([[0, 2, 2], [4, 3, 3]]), 12)
    with pytest.raises(ValueError, match="frames"):
        an.draw_numpy(np.zeros((2, 4, 4), dtype=np.uint8), [])
    with pytest.raises(ValueError, match="entropy"):
        an.write_result_video(None, np.zeros((1, 8, 8, 3), dtype=np.uint8), np.zeros((0, 6)), [0], np.ones((1, 7)), "x.avi", 25, entropy="bogus")


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_the_symbol_is_declared_bound_and_built():
    header = open(os.path.join(build.CSRC, "..", "..", "include", "avcer_hip.h")).read()
    assert re.search(r"\bavcer_annotate_frames\s*\(", header) and "avcer_annotate_frames" in _lib.SIGNATURES
    assert "annotate.hip" in build.SOURCES and re.search(r"#define AVCER_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    assert hasattr(ctypes.CDLL(build.build()), "avcer_annotate_frames")
    # the record: 12 x int32 in the header's order
    body = re.search(r"typedef struct avcer_draw_item \{(.*?)\} avcer_draw_item;", header, re.S).group(1)
    fields = re.findall(r"int32_t\s+([^;]+);", body)
    names = [n.strip() for f in fields for n in re.sub(r"\[\d+\]", "", f).split(",")]
    assert names == [n for n in an.ITEM.names] and an.ITEM.itemsize == 48
    assert (an.OUTLINE, an.FILL, an.MASK) == tuple(int(re.search(rf"AVCER_DRAW_{k} = (\d)", header).group(1)) for k in ("OUTLINE", "FILL", "MASK"))
