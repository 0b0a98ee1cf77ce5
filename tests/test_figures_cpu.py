"""avcer_amd/figures.py on the CPU: the integer / fma decimal formulation against Python's `format`, the cell colours against
matplotlib's own lookup, the statement `matrix_numpy` against a PIL drawing of the same plan at tolerance zero, and what the plan
refuses."""
import os

import numpy as np
import pytest
from PIL import Image, ImageDraw

import annotate_pil
import figure_cases as fc
from avcer_amd import evaluate, figures as fg

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


# ---------------------------------------------------------------------------------------------------- decimals
def test_percentages_of_every_small_row_print_as_format_prints_them():
    """Every count / rowsum with rowsum in 1..400 and count in 0..rowsum, as the statement computes the percentage."""
    bad = []
    for rowsum in range(1, 401):
        for count in range(0, rowsum + 1):
            x = float(count) / (rowsum + 1e-10) * 100
            if fg.fixed(x, 1) != format(x, ".1f"):
                bad.append((count, rowsum, fg.fixed(x, 1), format(x, ".1f")))
    assert not bad, bad[:5]


def test_two_decimals_and_the_hand_cases_print_as_format_prints_them():
    for k in range(0, 1001):
        assert fg.fixed(k / 1000, 2) == format(k / 1000, ".2f"), k
    below = np.nextafter(99.95, 0.0)
    hand = [0.25, 0.35, 2.5, 99.95, float(below), 0.125, 0.375, 0.005, 0.995, 0.0, -0.0, -0.001, -0.125, 1e-320, 9999.985, 5e-324,
            100 * (1 / (1 + 1e-10)), 100 * ((2 ** 31 - 1) / ((2 ** 31 - 1) + 1e-10)), 0 / 1e-10 * 100]
    for x in hand:
        for k in (1, 2):
            assert fg.fixed(x, k) == format(x, f".{k}f"), (x, k)
    assert format(0.125, ".2f") == "0.12" and format(0.375, ".2f") == "0.38"  # ties go to even on the exact value
    rng = np.random.default_rng(1)
    for x in np.concatenate([rng.random(20000), rng.random(20000) * 100]):
        assert fg.fixed(float(x), 1) == format(float(x), ".1f") and fg.fixed(float(x), 2) == format(float(x), ".2f"), x


def test_cell_text_is_the_references_format():
    cm = fc.conf_edge()
    plan = fg.matrix_plan(7, 7, "conf")
    shown = cm.astype("float") / (cm.sum(axis=1)[:, np.newaxis] + 1e-10) * 100
    thresh = (shown.max() + shown.min()) / 2.0
    recs = fg.cell_records(cm, plan)
    for i in range(7):
        for j in range(7):
            lut, ink, glyphs = recs[i * 7 + j]
            want = "{0}\n{1:.1f}%".format(cm[i, j], shown[i, j])  # visualize.py:64
            assert fc.text_of(glyphs) == want.replace("\n", ""), (i, j)
            assert ink == (255 if shown[i, j] > thresh else 0)
    assert recs[7][1] == 0 and recs[0][1] == 255  # the cell AT thresh is black, the largest white
    w = fc.weights(3, 7, 3)
    w[2, 6] = -0.001
    for rec, v in zip(fg.cell_records(w, fg.matrix_plan(3, 7, "weights")), w.reshape(-1)):
        assert fc.text_of(rec[2]) == "{0:.2f}".format(v)


# ---------------------------------------------------------------------------------------------------- colours
def test_committed_table_is_the_modules():
    np.testing.assert_array_equal(np.load(os.path.join(GOLDEN, "blues_lut.npy")), fg.BLUES)
    assert fg.BLUES.shape == (256, 3) and fg.BLUES.dtype == np.uint8


def test_cell_colours_are_matplotlibs():
    pytest.importorskip("matplotlib")
    import matplotlib.pyplot as plt
    from matplotlib.colors import Normalize

    np.testing.assert_array_equal(plt.cm.Blues(np.arange(256), bytes=True)[:, :3], fg.BLUES)
    pct = np.array([float(c) / (r + 1e-10) * 100 for r in range(1, 401) for c in range(0, r + 1)])
    want = plt.cm.Blues(Normalize(0, 100)(pct), bytes=True)[:, :3]
    got = fg.BLUES[[fg.lut_index(float(v), 100.0) for v in pct]]
    np.testing.assert_array_equal(got, want)
    w = np.concatenate([np.arange(0, 1001) / 1000, np.arange(0, 257) / 256, np.nextafter(np.arange(1, 257) / 256, 0),
                        [-0.5, -1e-9, 1.0, 1.0000001, 7.0], np.random.default_rng(2).random(5000)])
    want = plt.cm.Blues(Normalize(0, 1)(w), bytes=True)[:, :3]
    np.testing.assert_array_equal(fg.BLUES[[fg.lut_index(float(v), 1.0) for v in w]], want)


# ---------------------------------------------------------------------------------------------------- the statement against PIL
def pil_figure(values, plan):
    """The figure drawn by PIL alone: ImageDraw.rectangle per cell and colour band, ImageDraw.bitmap per glyph, then the plan's
    items one ImageDraw call each (annotate_pil.draw_pil)."""
    flat, table, _ = fg.glyph_atlas(plan.font)
    im = Image.new("RGB", (plan.width, plan.height), (255, 255, 255))
    d = ImageDraw.Draw(im)
    for c, (lut, ink, glyphs) in enumerate(fg.cell_records(values, plan)):
        box = plan.cell(c // plan.cols, c % plan.cols)
        d.rectangle(box, fill=tuple(int(v) for v in fg.BLUES[lut]))
        for g, x, y in glyphs:
            off, w, h = (int(v) for v in table[g, :3])
            assert box[0] <= x and x + w - 1 <= box[2] and box[1] <= y and y + h - 1 <= box[3], "the text of these cases fits its cell"
            d.bitmap((x, y), Image.fromarray(flat[off:off + w * h].reshape(h, w)), fill=(ink, ink, ink))
    for k in range(256):
        b = plan.band(k)
        if b is not None:
            d.rectangle(b, fill=tuple(int(v) for v in fg.BLUES[k]))
    return annotate_pil.draw_pil(np.array(im)[None], plan.items, plan.masks)[0]


def test_mixed_figures_equal_pil():
    for values, plan, pic in fc.mixed():
        np.testing.assert_array_equal(pic, pil_figure(values, plan), err_msg=repr(plan))


@pytest.mark.parametrize("shape, kind, kw", [
    ((3, 7), "weights", dict(labels=fc.WEIGHT_LABELS, title="Weights", x_labels=True)),
    ((3, 7), "weights", dict(labels=fc.WEIGHT_LABELS, title="Weights", x_labels=False)),
    ((4, 8), "weights", dict(x_labels=True)),
    ((4, 8), "weights", dict(x_labels=False, colorbar=False)),
    ((7, 7), "conf", dict(labels=evaluate.EMO, colorbar=False, title="no bar")),
    ((7, 7), "conf", dict(labels=evaluate.EMO, width=400, height=300, title="small")),
    ((3, 7), "weights", dict(width=400, height=300)),
])
def test_statement_equals_pil(shape, kind, kw):
    values = fc.conf_edge() if kind == "conf" else fc.weights(*shape, seed=shape[1])
    if kw.get("width") == 400 and kind == "conf":
        values = np.minimum(values, 10 ** 6)  # still a zero row and the tie
    plan = fg.matrix_plan(shape[0], shape[1], kind, **kw)
    pic = fg.matrix_numpy(values, plan)
    np.testing.assert_array_equal(pic, pil_figure(values, plan))
    assert (pic != 255).any()
    if not kw.get("colorbar", True):
        assert plan.bar[2] == 0


def test_cells_tile_the_plot_rectangle_and_nothing_else_is_painted():
    for values, plan, _ in fc.mixed():
        pic = np.full((plan.height, plan.width, 3), 77, dtype=np.uint8)
        fg.paint_numpy(values, plan, pic)
        touched = np.zeros((plan.height, plan.width), dtype=bool)
        touched[plan.y0:plan.y0 + plan.ph, plan.x0:plan.x0 + plan.pw] = True
        bx, by, bw, bh = plan.bar
        touched[by:by + bh, bx:bx + bw] = True
        assert (pic[~touched] == 77).all()
        assert plan.xe(0) == plan.x0 and plan.xe(plan.cols) == plan.x0 + plan.pw and plan.ye(plan.rows) == plan.y0 + plan.ph


# ---------------------------------------------------------------------------------------------------- what is refused
def test_plan_refuses_before_any_work():
    for rows, cols in ((0, 7), (7, 0), (17, 7), (7, 17), (True, 7), (7.0, 7)):
        with pytest.raises(ValueError, match="1..16"):
            fg.matrix_plan(rows, cols, "conf")
    with pytest.raises(ValueError, match="kind"):
        fg.matrix_plan(7, 7, "heat")
    with pytest.raises(ValueError, match="empty plot rectangle"):
        fg.matrix_plan(2, 2, "conf", width=60, height=600)
    with pytest.raises(ValueError, match="too small for their text"):
        fg.matrix_plan(16, 16, "conf")            # 10 digits do not fit a sixteenth of 800 pixels
    with pytest.raises(ValueError, match="too small for their text"):
        fg.matrix_plan(16, 16, "weights", width=400, height=300, font=fg.default_font(600))
    with pytest.raises(ValueError, match="labels"):
        fg.matrix_plan(7, 7, "conf", labels=["a", "b"][:1])
    plan = fg.matrix_plan(2, 2, "conf")
    for bad in (np.zeros((3, 2), dtype=np.int64), np.zeros((2, 2)), np.array([[1, -1], [0, 0]]), np.array([[10 ** 10, 0], [0, 0]])):
        with pytest.raises(ValueError):
            fg.matrix_numpy(bad, plan)
    plan = fg.matrix_plan(2, 2, "weights")
    for bad in (np.array([[np.nan, 0], [0, 0]]), np.array([[np.inf, 0], [0, 0]]), np.array([[0.5, 10000.0], [0, 0]])):
        with pytest.raises(ValueError, match=r"cell \(0, [01]\)"):
            fg.matrix_numpy(bad, plan)
