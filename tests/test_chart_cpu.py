"""The prediction timeline chart without a GPU (avcer_amd/chart.py): the line rule and the traces against PIL's ImageDraw.line at
tolerance zero, the thinning rule, the decoration against ImageDraw, the file against Image.save, the rule number and file names,
and what is refused before any work."""
import ctypes
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageColor, ImageDraw

import chart_cases as cc
from annotate_pil import draw_pil
from avcer_amd import annotate as an
from avcer_amd import chart, jpeg
from avcer_amd import run as arun
from avcer_amd.fusion import COMPOUND_NAMES, MODEL_ORDER
from test_tracks_cpu import NoEngine


def pil_line(points, height, width):
    """bool [height, width]: ImageDraw.line(width=1) segment by segment on a blank canvas (one point: ImageDraw.point)."""
    im = Image.new("L", (width, height), 0)
    d = ImageDraw.Draw(im)
    if len(points) == 1:
        d.point(points[0], fill=255)
    for a, b in zip(points[:-1], points[1:]):
        d.line([a, b], fill=255, width=1)
    return np.array(im) > 0


# ---------------------------------------------------------------------------------------------------- the line rule
def test_line_rule_equals_pil_for_every_step_in_both_directions():
    """Every (dx, dy), 0 <= dx <= 12, -40 <= dy <= 40, from a to b and from b to a: a tie is stepped away from the start, so the
    two directions differ and both are PIL's."""
    differ = 0
    for dx in range(0, 13):
        for dy in range(-40, 41):
            a, b = (20, 50), (20 + dx, 50 + dy)
            masks = []
            for p, q in ((a, b), (b, a)):
                got = chart.runs_to_mask(*chart.line_runs([p[0]], [p[1]], [q[0]], [q[1]]), 100, 48)
                np.testing.assert_array_equal(got, pil_line([p, q], 100, 48), err_msg=f"{p} -> {q}")
                masks.append(got)
            differ += not np.array_equal(*masks)
    assert differ > 0  # e.g. (1, 10): the direction is part of the rule


def test_line_runs_takes_many_segments_at_once():
    rng = np.random.default_rng(3)
    xa, xb = rng.integers(0, 48, 200), rng.integers(0, 48, 200)
    ya, yb = rng.integers(0, 100, 200), rng.integers(0, 100, 200)
    want = np.zeros((100, 48), dtype=bool)
    for k in range(200):
        want |= pil_line([(int(xa[k]), int(ya[k])), (int(xb[k]), int(yb[k]))], 100, 48)
    np.testing.assert_array_equal(chart.runs_to_mask(*chart.line_runs(xa, ya, xb, yb), 100, 48), want)


# ---------------------------------------------------------------------------------------------------- the plan
def test_plan_geometry():
    p = cc.plan(10)
    assert (p.width, p.height) == (cc.WIDTH, cc.HEIGHT) and p.pw >= 8 and p.ph >= 14
    assert p.x0 > 0 and p.y0 > 0 and p.x0 + p.pw < p.width and p.y0 + p.ph < p.height
    assert list(p.yc) == [p.y0 + p.ph - 1 - ((2 * c + 1) * p.ph) // 14 for c in range(7)]
    assert all(p.y0 <= y < p.y0 + p.ph for y in p.yc) and list(p.yc) == sorted(p.yc, reverse=True) and len(set(p.yc)) == 7
    big = chart.chart_plan(750)
    assert (big.width, big.height) == (1200, 200) and big.pw > 900 and big.ph > 140
    # 64-bit columns: frame 0 in the first column, the last frame in the last one, and no overflow at 2^40 frames
    for T in (1, 2, p.pw, 1000, 1 << 40):
        q = p.with_T(T)
        assert q.col(0) == q.x0 + q.pw // (2 * T) and q.col(T - 1) == q.x0 + ((2 * T - 1) * q.pw) // (2 * T) < q.x0 + q.pw
    assert p.with_T(p.pw).path == chart.PATH_REDUCE and p.with_T(p.pw - 1).path == chart.PATH_SEGMENT
    assert chart.COLOURS == tuple(ImageColor.getrgb(n) for n in chart.COLOUR_NAMES)


@pytest.mark.parametrize("T", cc.lengths())
@pytest.mark.parametrize("kind", cc.TABLES)
def test_trace_equals_pil_segment_by_segment(kind, T):
    t, p, _ = cc.reference(kind, T)
    x = p.col(np.arange(T))
    for s in range(4):
        pts = [(int(x[i]), int(p.yc[int(t[s, i])])) for i in range(T)]
        np.testing.assert_array_equal(chart.trace_numpy(t[s], p), pil_line(pts, p.height, p.width), err_msg=f"series {s}")


@pytest.mark.parametrize("T", cc.lengths())
@pytest.mark.parametrize("kind", cc.TABLES)
def test_thinning_is_disjoint_and_covers_the_widened_trace(kind, T):
    t, p, got = cc.reference(kind, T)
    assert got.sum(axis=0).max() <= 1                                     # no two series on one pixel
    yy, xx = np.mgrid[0:p.height, 0:p.width]
    inside = (xx >= p.x0) & (xx < p.x0 + p.pw) & (yy >= p.y0) & (yy < p.y0 + p.ph)
    for s in range(4):
        tr = chart.trace_numpy(t[s], p)
        wide = tr.copy()
        wide[1:] |= tr[:-1]
        wide[:-1] |= tr[1:]
        np.testing.assert_array_equal(got[s], wide & inside & ((xx + yy) % 4 == s))
        assert got[s].any() or T == 1                                     # a lone point is 3 pixels: one residue goes without
    if kind == "constant":  # series 0 and 1 coincide and both stay visible; the union of coinciding series is their widened trace
        np.testing.assert_array_equal(chart.trace_numpy(t[0], p), chart.trace_numpy(t[1], p))
        assert T == 1 or (got[0].any() and got[1].any() and not (got[0] & got[1]).any())


def test_one_interval_per_column():
    """The bound the kernel's envelope rests on: in every column every series' trace is one run of rows."""
    for kind in cc.TABLES:
        for T in cc.lengths():
            t, p, _ = cc.reference(kind, T)
            for s in range(4):
                tr = chart.trace_numpy(t[s], p)
                starts = (tr[1:] & ~tr[:-1]).sum(axis=0) + tr[0]
                assert starts.max() <= 1, (kind, T, s)


# ---------------------------------------------------------------------------------------------------- the picture and the file
@pytest.mark.parametrize("T,kind", [(1, "constant"), (7, "ramp"), (1000, "random")])
def test_chart_is_pils_drawing_of_the_items_over_the_traces(T, kind):
    t, p, series = cc.reference(kind, T)
    base = cc.painted(series)
    want = draw_pil(base[None], p.items, p.masks)[0]
    got = chart.chart_numpy(t, p)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.uint8 and got.shape == (p.height, p.width, 3)
    # the decoration lies outside the plot rectangle: no trace pixel is drawn over
    np.testing.assert_array_equal(got[p.y0:p.y0 + p.ph, p.x0:p.x0 + p.pw], base[p.y0:p.y0 + p.ph, p.x0:p.x0 + p.pw])
    kinds = [int(k) for k in p.items["kind"]]
    assert kinds.count(an.OUTLINE) == 1 and kinds.count(an.MASK) == 7 + 3 + 4 and kinds.count(an.FILL) == 7 + 4
    cache = an.label_masks(chart.default_font(p.height))
    for name in COMPOUND_NAMES + MODEL_ORDER + (chart.TITLE, chart.X_TITLE):
        assert any(np.array_equal(m, cache.get(name)[0]) for m in p.masks), name
    assert any(np.array_equal(m, np.rot90(cache.get(chart.Y_TITLE)[0])) for m in p.masks)


def test_file_bytes_are_pils_save_of_the_picture():
    """The encoder's host half on the chart (forward_numpy + avcer_jpeg_write_batch): Image.save(quality=95, subsampling=2)."""
    from avcer_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(build.LIB)
    for name in ("avcer_jpeg_quant_tables", "avcer_jpeg_plan", "avcer_jpeg_write_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    t, p, _ = cc.reference("random", 1000)
    pic = chart.chart_numpy(t, p)
    coeffs, desc = jpeg.forward_numpy([pic], 95, 2)
    desc = desc.copy()
    out = np.zeros(623 * len(desc) + 420 * (coeffs.size // 64), dtype=np.uint8)
    offsets, need = jpeg.write_batch(lib, np.ascontiguousarray(coeffs.reshape(-1)), desc, out, 1)
    b = io.BytesIO()
    Image.fromarray(pic).save(b, "JPEG", quality=95, subsampling=2)
    assert out[int(offsets[0]):int(offsets[1])].tobytes() == b.getvalue()


# ---------------------------------------------------------------------------------------------------- names and refusals
def test_rule_number_and_file_names(tmp_path):
    assert chart.rule_name(True, False) == "Rule 2" and chart.rule_name(False, True) == "Rule 1"
    assert chart.rule_name(True, True) == "Rule 2"                         # run.py:281-284: the second `if` overwrites the first
    with pytest.raises(ValueError, match="ce_mask"):
        chart.rule_name(False, False)
    root = str(tmp_path)
    assert chart.plot_paths(root, "Rule 2") == [os.path.join(root, "pedicted_CEs_Rule 2.jpg")]
    assert chart.plot_paths(root, "Rule 1", (3, 0, 12)) == [os.path.join(root, "pedicted_CEs_Rule 1.jpg"),
                                                           os.path.join(root, "pedicted_CEs_Rule 1__t00.jpg"),
                                                           os.path.join(root, "pedicted_CEs_Rule 1__t12.jpg")]
    assert chart.check_plot_pred(False, "", False, False, None) is None     # off: nothing is looked at
    assert chart.check_plot_pred(True, root, True, False, (64, 96)) == ("Rule 2", (64, 96))


def test_bad_tables_and_plans_are_refused():
    p = cc.plan(5)
    for bad in (np.array([[0, 1, 2, 3, 7]]), np.array([[0, -1, 2, 3, 4]]), np.zeros((5, 5), dtype=np.int64), np.zeros((1, 4), dtype=np.int64),
                np.zeros((1, 5)), np.zeros(5, dtype=np.int64)):
        with pytest.raises(ValueError):
            chart.chart_numpy(bad, p)
    for T in (0, -3, True, 2.0):
        with pytest.raises(ValueError, match="T >= 1"):
            chart.chart_plan(T)
    for size in ((40, 64), (96, 10), (0, 64)):
        with pytest.raises(ValueError, match="plot rectangle|sides"):
            chart.chart_plan(10, *size)


BAD_OPTIONS = [
    (dict(path_save_results=""), "path_save_results"),
    (dict(path_save_results="X", ce_weights_type=False, ce_mask=False), "ce_mask"),
    (dict(path_save_results="X", plot_size=(10, 96)), "plot rectangle"),
    (dict(path_save_results="X", plot_size=7), "plot_size"),
]


@pytest.mark.parametrize("kw,match", BAD_OPTIONS, ids=[m for _, m in BAD_OPTIONS])
def test_the_option_is_refused_before_any_work(kw, match, tmp_path):
    from avcer_amd.dataset import VideoJob, run_dataset

    frames, wav, dets = np.zeros((2, 8, 8, 3), dtype=np.uint8), np.zeros(1600, dtype=np.float32), [np.zeros((0, 15), dtype=np.float32)] * 2
    kw = {k: (str(tmp_path / "res") if v == "X" else v) for k, v in kw.items()}

    def never():
        raise AssertionError("a job was loaded")

    jobs = [VideoJob("v", 2, 8, 8, 25, 1600, detections=dets, load=never)]
    for call in (lambda: arun.run_inference(NoEngine(), frames, wav, 25, detections=dets, flag_save_plot_pred=True, **kw),
                 lambda: arun.run_inference_file(NoEngine(), tmp_path / "missing.avi", detections=dets, flag_save_plot_pred=True, **kw),
                 lambda: arun.run_inference_file(NoEngine(), tmp_path / "missing.avi", detections=dets, flag_save_plot_pred=True, stream_frames=4, **kw),
                 lambda: run_dataset(NoEngine(), jobs, flag_save_plot_pred=True, **kw)):
        with pytest.raises(ValueError, match=match):
            call()
    assert not (tmp_path / "res").exists()
