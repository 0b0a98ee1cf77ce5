"""The matrix figures as annotate item lists (avcer_amd/figures.py matrix_items, batch_items) on the CPU: the list drawn by
annotate.draw_numpy onto a white picture against the statement `matrix_numpy` at tolerance zero; that an unclipped MASK item never
leaves the cell `paint_numpy` would clip it to, for every plan `matrix_plan` accepts on the grid below; what `render`, the file
writers and `score(save_path=)` refuse, before an engine is touched; and that `score` without the new arguments is today's."""
import numpy as np
import pytest

import eval_cases as ec
import figure_cases as fc
import figure_item_cases as fi
from avcer_amd import annotate as an
from avcer_amd import evaluate as ev
from avcer_amd import figures as fg
from avcer_amd import weight_search as ws


def drawn(values, plan, frame=0, n=1):
    items, masks = fg.matrix_items(values, plan, frame)
    white = np.full((n, plan.height, plan.width, 3), 255, dtype=np.uint8)
    return an.draw_numpy(white, items, masks), items, masks


# ---------------------------------------------------------------------------------------------------- the list is the statement
def values_for(kind, rows, cols):
    if kind == "weights":
        return fi.weights_neg(rows, cols, rows * cols)  # a negative weight, 1.0, and values between
    cm = np.random.default_rng(rows * cols).integers(0, 3000, (rows, cols)).astype(np.int64)
    cm[0, 0] = fg.COUNT_MAX  # ten digits
    cm[rows // 2] = 0        # a row of zeros: 0 / (0 + 1e-10)
    return cm


@pytest.mark.parametrize("colorbar", [True, False])
@pytest.mark.parametrize("kind", ["conf", "weights"])
@pytest.mark.parametrize("rows, cols", [(1, 1), (2, 3), (7, 7), (16, 16)])
def test_items_drawn_on_white_are_the_statement(rows, cols, kind, colorbar):
    size = (800, 600) if fi.accepts(rows, cols, kind, 800, 600) else (3200, 1200)  # 16 x 16 counts of ten digits need the room
    plan = fg.matrix_plan(rows, cols, kind, size[0], size[1], title=f"{kind} {rows} x {cols}", colorbar=colorbar)
    values = values_for(kind, rows, cols)
    got, items, masks = drawn(values, plan)
    np.testing.assert_array_equal(got[0], fg.matrix_numpy(values, plan))
    assert (items["frame"] == 0).all() and len(masks) == len(fg.GLYPHS) + len(plan.masks)
    assert (plan.bar[2] == 0) == (not colorbar)


def test_the_order_of_the_list():
    """Cells, then glyphs, then colour bands, then the plan's own items with their masks behind the 13 glyph masks."""
    values, plan = fi.conf_7(), fg.matrix_plan(7, 7, "conf", labels=ev.EMO, title="order")
    items, masks = fg.matrix_items(values, plan, frame=3)
    recs = fg.cell_records(values, plan)
    n_glyphs = sum(len(r[2]) for r in recs)
    n_bands = sum(plan.band(k) is not None for k in range(256))
    assert len(items) == 49 + n_glyphs + n_bands + len(plan.items) and (items["frame"] == 3).all()
    cells, text, bands, own = np.split(items, np.cumsum([49, n_glyphs, n_bands]))
    assert (cells["kind"] == an.FILL).all() and (cells["arg"] == 255).all()
    np.testing.assert_array_equal(cells["colour"], fg.BLUES[[r[0] for r in recs]])
    assert [tuple(int(v) for v in c) for c in cells[["x0", "y0", "x1", "y1"]].tolist()] == [plan.cell(i, j) for i in range(7) for j in range(7)]
    assert (text["kind"] == an.MASK).all() and (text["mask"] < 13).all() and set(np.unique(text["colour"])) <= {0, 255}
    assert [(int(t["mask"]), int(t["x0"]), int(t["y0"])) for t in text] == [g for r in recs for g in r[2]]
    assert (bands["kind"] == an.FILL).all()
    np.testing.assert_array_equal(bands["colour"], fg.BLUES[[k for k in range(256) if plan.band(k) is not None]])
    want = plan.items.copy()
    want["frame"] = 3
    want["mask"] = np.where(want["kind"] == an.MASK, want["mask"] + 13, want["mask"])
    np.testing.assert_array_equal(own, want)
    assert all(a is b for a, b in zip(masks[13:], plan.masks))


def test_a_batch_is_its_figures_over_one_mask_list():
    cases = fc.mixed()
    items, masks = fg.batch_items([c[0] for c in cases], [c[1] for c in cases])
    assert (np.diff(items["frame"]) >= 0).all() and set(items["frame"]) == set(range(len(cases)))
    keys = [(m.shape, m.tobytes()) for m in masks]
    assert len(set(keys)) == len(keys) < sum(13 + len(c[1].masks) for c in cases)  # identical masks stand once
    white = np.full((len(cases), 600, 800, 3), 255, dtype=np.uint8)
    got = an.draw_numpy(white, items, masks)
    for k, (_, plan, pic) in enumerate(cases):
        np.testing.assert_array_equal(got[k], pic, err_msg=repr(plan))


# ---------------------------------------------------------------------------------------------------- no glyph leaves its cell
def sizes_of(rows, cols, kind):
    return ([(800, 600)] if fi.accepts(rows, cols, kind, 800, 600) else []) + list(fi.smallest_sizes(rows, cols, kind))


@pytest.mark.parametrize("rows", range(1, 17))
def test_no_count_text_leaves_its_cell(rows):
    """Every accepted plan of 1..16 columns, at the default size and at the smallest sizes: ten digits over "100.0%" in every cell
    (fi.conf_extremes).  matrix_plan sizes a "conf" cell for exactly these, so matrix_items must accept them all."""
    seen = 0
    for cols in range(1, 17):
        for width, height in sizes_of(rows, cols, "conf"):
            plan = fg.matrix_plan(rows, cols, "conf", width, height)
            for values in fi.conf_extremes(rows, cols):
                assert fi.glyphs_outside(values, plan) == [], (rows, cols, width, height)
                seen += 1
            fg.matrix_items(fi.conf_extremes(rows, cols)[1], plan)  # does not raise
    assert seen >= 16 * 3


@pytest.mark.parametrize("rows", range(1, 17))
def test_no_weight_text_leaves_its_cell_or_the_cell_is_named(rows):
    """Weights in 0..1 ("0.00" .. "1.00", what matrix_plan sizes a "weights" cell for) stay inside at every accepted plan.  The
    widest weight, "-9999.99", stays inside or matrix_items raises ValueError naming the first cell it leaves: never a picture."""
    refused = inside = 0
    for cols in range(1, 17):
        for width, height in sizes_of(rows, cols, "weights"):
            plan = fg.matrix_plan(rows, cols, "weights", width, height)
            usual = np.linspace(0.0, 1.0, rows * cols).reshape(rows, cols)
            assert fi.glyphs_outside(usual, plan) == [] and fi.glyphs_outside(np.ones((rows, cols)), plan) == []
            wide = np.full((rows, cols), fi.WIDEST_WEIGHT)
            bad = fi.glyphs_outside(wide, plan)
            if bad:
                with pytest.raises(ValueError, match=rf"cell \({bad[0][0]}, {bad[0][1]}\)"):
                    fg.matrix_items(wide, plan)
                refused += 1
            else:
                fg.matrix_items(wide, plan)  # does not raise
                if rows * cols <= 4:  # the equality itself, where it is cheap
                    np.testing.assert_array_equal(drawn(wide, plan)[0][0], fg.matrix_numpy(wide, plan))
                inside += 1
    assert refused and inside  # both outcomes occur in every row of the grid


def test_one_wide_weight_names_its_own_cell():
    width, height = fi.smallest_sizes(3, 7, "weights")[0]
    plan = fg.matrix_plan(3, 7, "weights", width, height)
    w = np.full((3, 7), 0.5)
    fg.matrix_items(w, plan)
    w[1, 4] = fi.WIDEST_WEIGHT
    assert fi.glyphs_outside(w, plan) == [(1, 4)]
    with pytest.raises(ValueError, match=r"cell \(1, 4\).*-9999\.99"):
        fg.matrix_items(w, plan)
    fg.matrix_numpy(w, plan)  # the statement still clips, as before


# ---------------------------------------------------------------------------------------------------- refusals
class NoEngine:
    """An engine none of whose attributes may be touched: a refusal has to come before any of them is."""

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was used before the call was refused")


def test_render_refuses_before_anything_is_drawn(monkeypatch):
    monkeypatch.setattr(an, "draw", lambda *a, **k: pytest.fail("annotate.draw was called"))
    eng = NoEngine()
    conf, weights = fg.matrix_plan(2, 2, "conf"), fg.matrix_plan(2, 2, "weights")
    small = fg.matrix_plan(2, 2, "conf", width=400, height=300)
    cm, w = np.array([[1, 2], [3, 4]]), np.array([[0.1, 0.2], [0.3, 0.4]])
    with pytest.raises(ValueError, match="no figure"):
        fg.render(eng, [], [])
    with pytest.raises(ValueError, match="one picture size.*400 x 300.*800 x 600"):
        fg.render(eng, [cm, cm], [conf, small])
    with pytest.raises(ValueError, match="2 matrices for 1 plans"):
        fg.render(eng, [cm, cm], [conf])
    for values, plan in ((np.zeros((3, 2), dtype=np.int64), conf), (w, conf), (np.array([[1, -1], [0, 0]]), conf),
                         (np.array([[fg.COUNT_MAX + 1, 0], [0, 0]]), conf), (np.array([[np.nan, 0.0], [0, 0]]), weights),
                         (np.array([[0.5, 10000.0], [0, 0]]), weights)):
        with pytest.raises(ValueError):
            fg.render(eng, [cm, values], [conf, plan])
    with pytest.raises(ValueError, match="max_figures_per_call"):
        fg.render(eng, [cm], [conf], max_figures_per_call=0)


@pytest.mark.parametrize("name, word", [("cm.png", "PNG"), ("cm.pdf", "PDF"), ("cm.svg", "SVG"), ("cm.PDF", "PDF"), ("cm.txt", "JPEG"),
                                        ("cm", "JPEG")])
def test_writers_refuse_other_formats_by_name(tmp_path, name, word):
    eng = NoEngine()
    cm, w = np.array([[1, 2], [3, 4]]), np.array([[0.1, 0.2], [0.3, 0.4]])
    with pytest.raises(ValueError, match=word):
        fg.write_conf_matrices(eng, [cm, cm], None, [tmp_path / "a.jpg", tmp_path / name])
    with pytest.raises(ValueError, match=word):
        fg.write_weights_matrices(eng, [w], None, [tmp_path / name])
    with pytest.raises(ValueError, match=word):
        ev.score(eng, [0, 1], [np.eye(7)[:2]], save_path=tmp_path / name)
    assert list(tmp_path.iterdir()) == []


def test_writers_refuse_before_anything_is_drawn(tmp_path):
    eng = NoEngine()
    cm, w = np.array([[1, 2], [3, 4]]), np.array([[0.1, 0.2], [0.3, 0.4]])
    good = [tmp_path / "a.jpg", tmp_path / "b.jpeg"]
    assert fg.check_paths(good) == [str(p) for p in good]
    with pytest.raises(ValueError, match="1 paths for 2 figures"):
        fg.write_conf_matrices(eng, [cm, cm], None, good[:1])
    with pytest.raises(ValueError, match="3 titles for 2 figures"):
        fg.write_conf_matrices(eng, [cm, cm], None, good, titles=["a", "b", "c"])
    with pytest.raises(ValueError, match="entropy"):
        fg.write_conf_matrices(eng, [cm, cm], None, good, entropy="gpu")
    with pytest.raises(ValueError, match="labels"):
        fg.write_conf_matrices(eng, [cm], ["a", "b", "c"], good[:1])
    with pytest.raises(ValueError, match="integer counts"):
        fg.write_conf_matrices(eng, [w], None, good[:1])
    with pytest.raises(ValueError, match="too small"):
        fg.write_conf_matrices(eng, [np.zeros((16, 16), dtype=np.int64)], None, good[:1])
    with pytest.raises(ValueError, match=r"\[rows, cols\]"):
        fg.write_conf_matrices(eng, [np.zeros(4, dtype=np.int64)], None, good[:1])
    with pytest.raises(ValueError, match="1 x_labels for 2 figures"):
        fg.write_weights_matrices(eng, [w, w], None, good, x_labels=[True])
    with pytest.raises(ValueError, match="not finite"):
        fg.write_weights_matrices(eng, [w, w * np.inf], None, good)
    with pytest.raises(ValueError, match="unknown figure option"):
        ev.score_models(eng, [0], {"stat": np.eye(7)[:1]}, save_dir=tmp_path, dpi=100)
    with pytest.raises(ValueError, match="keyed by"):
        ev.score_models(eng, [0], {"static": np.eye(7)[:1]})
    with pytest.raises(ValueError, match="M = 2 or 3"):
        ws.write_weight_figures(eng, np.ones((4, 7)), np.ones(4), tmp_path)
    with pytest.raises(ValueError, match="audio_classes"):
        ws.write_weight_figures(eng, np.ones((3, 7)), np.ones(3), tmp_path, audio_classes=9)
    assert list(tmp_path.iterdir()) == []


# ---------------------------------------------------------------------------------------------------- the wiring
def test_score_without_a_path_is_todays_dict():
    g = ec.load()
    trues, tables = g["av_abaw_trues"], [g["av_abaw_stat"], g["av_abaw_dyn"], g["av_abaw_audio"]]
    for w1, w2 in ((g["w1"], g["w2"]), (None, None)):
        want = ev.score_numpy(trues, tables, w1, w2)
        for got in (ev.score(ev.NumpyEngine(), trues, tables, w1, w2), ev.score(ev.NumpyEngine(), trues, tables, w1, w2, save_path=None)):
            assert list(got) == list(want) == ["uar", "acc", "f1", "precision", "mean", "cm"]
            assert all(np.array_equal(got[k], want[k]) and type(got[k]) is type(want[k]) for k in want)
    ec.check_score(g, "av_abaw", 0, ev.score(ev.NumpyEngine(), trues, tables, g["w1"], g["w2"], save_path=None))


def test_score_models_without_a_dir_scores_the_fusion_and_every_model():
    g = ec.load()
    trues = g["video_abaw_trues"]
    models = {"stat": g["video_abaw_stat"], "dyn": g["video_abaw_dyn"]}
    got = ev.score_models(ev.NumpyEngine(), trues, models, g["w1"][:2], g["w2"][:2])
    assert list(got) == ["fusion", "stat", "dyn"] and all("plot_conf" not in m for m in got.values())
    for index, key in enumerate(got):  # get_pred_video.get_metrics: the fusion, the static model, the dynamic model
        ec.check_score(g, "video_abaw", index, got[key])
    alone = ev.score_models(ev.NumpyEngine(), g["audio_abaw_trues"], {"audio": g["audio_abaw_audio"]})
    assert list(alone) == ["audio"]
    ec.check_score(g, "audio_abaw", 0, alone["audio"])


def test_the_weight_figure_is_the_scripts_table():
    """get_weights_matrices.py:5-16: the eight rows [VS, VD] per emotion and "Mo", transposed."""
    from avcer_amd import fusion

    m = ws.weight_figure_matrix(fusion.WEIGHTS_V_1, fusion.WEIGHTS_V_2)
    assert m.shape == (2, 8) and m[0, 0] == 0.42633145 and m[1, 0] == 0.57366855 and m[0, 6] == 0.81048546
    assert list(m[:, 7]) == [0.36499999999999994, 0.22999999999999998]
    assert ws.weight_figure_matrix(fusion.WEIGHTS_AV_1, fusion.WEIGHTS_AV_2).shape == (3, 8)
    for (models, cls), (stem, title, (fw, fh), x_labels) in ws.WEIGHT_FIGURES.items():
        labels = (ws.WEIGHT_FIGURE_LABELS[0][:models], ws.WEIGHT_FIGURE_LABELS[1])
        plan = fg.matrix_plan(models, 8, "weights", 100 * fw, 100 * fh, labels, title, None, True, x_labels)  # the script's sizes are accepted
        fg.matrix_items(np.full((models, 8), 0.5), plan)
