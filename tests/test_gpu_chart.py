"""avcer_chart_series (csrc/chart.hip) against chart.series_numpy / chart.chart_numpy -- which tests/test_chart_cpu.py holds to PIL --
bit for bit: every length and table of tests/chart_cases.py, both envelope paths by name, batches, both table dtypes, a column
reduction of more than a thousand frames per column, a table whose indices pass 2^31, a background that must survive, and the
argument checks."""
import numpy as np
import pytest
import torch

import chart_cases as cc
from avcer_amd import chart

pytestmark = pytest.mark.gpu


def background(n, h, w, seed=0):
    """A picture of noise: whatever the kernel does not paint must come back as it went in."""
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def over(bg, series_mask):
    want = bg.copy()
    for s, m in enumerate(series_mask):
        want[m] = chart.COLOURS[s]
    return want


@pytest.mark.parametrize("T", cc.lengths())
@pytest.mark.parametrize("kind", cc.TABLES)
def test_series_equal_series_numpy(engine, kind, T):
    t, p, want = cc.reference(kind, T)
    bg = background(1, p.height, p.width, T)
    out = torch.from_numpy(bg).to(engine.device)
    td = torch.from_numpy(t.copy()).to(engine.device)
    assert engine.chart_series(td, [p], out) is out
    np.testing.assert_array_equal(out.cpu().numpy()[0], over(bg[0], want))
    assert torch.equal(td.cpu(), torch.from_numpy(t.copy()))
    # the whole chart: traces, then the decoration through annotate.draw
    np.testing.assert_array_equal(chart.render(engine, td, plan=p).cpu().numpy()[0], chart.chart_numpy(t, p))


def test_which_path_each_case_takes(engine):
    """T >= pw: a column reduces its frames over a wave; T < pw: a column evaluates the segment that crosses it."""
    pw = cc.plan(1).pw
    want = {1: chart.PATH_SEGMENT, 2: chart.PATH_SEGMENT, 7: chart.PATH_SEGMENT, pw - 1: chart.PATH_SEGMENT, pw: chart.PATH_REDUCE,
            pw + 1: chart.PATH_REDUCE, 3 * pw + 5: chart.PATH_REDUCE, 1000: chart.PATH_REDUCE}
    assert set(want) == set(cc.lengths())
    for T, path in want.items():
        assert engine.chart_path(T, pw) == path == cc.plan(T).path, chart.PATH_NAMES[path]
    assert engine.chart_path(300000, cc.plan(1, 256, 64).pw) == chart.PATH_REDUCE
    assert engine.lib.avcer_chart_path(0, 10) < 0 and engine.lib.avcer_chart_path(5, 0) < 0


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_a_batch_equals_its_single_calls(engine, dtype):
    """V = 3 charts of 1, 97 and 1000 frames (both paths) in ONE call; int32 and int64 tables give the same picture."""
    cases = [("random", 1), ("random", 97), ("random", 1000)]
    refs = [cc.reference(kind, T) for kind, T in cases]
    table = torch.from_numpy(np.concatenate([r[0] for r in refs], axis=1)).to(engine.device).to(dtype)
    plans = [r[1] for r in refs]
    bg = background(3, cc.HEIGHT, cc.WIDTH, 9)
    out = engine.chart_series(table, plans, torch.from_numpy(bg).to(engine.device)).cpu().numpy()
    at = 0
    for v, (t, p, want) in enumerate(refs):
        np.testing.assert_array_equal(out[v], over(bg[v], want), err_msg=f"chart {v}")
        one = engine.chart_series(table[:, at:at + p.T].contiguous(), [p], torch.from_numpy(bg[v:v + 1]).to(engine.device))
        np.testing.assert_array_equal(one.cpu().numpy()[0], out[v])
        at += p.T
    whole = chart.render(engine, table, T=[1, 97, 1000], plan=plans[0]).cpu().numpy()
    for v, (t, p, _) in enumerate(refs):
        np.testing.assert_array_equal(whole[v], chart.chart_numpy(t, p), err_msg=f"chart {v}")


def test_column_reduction_over_a_thousand_frames_per_column(engine):
    t, p, want = cc.reference("random", 300000, 256, 64)
    assert p.T // p.pw > 1000 and p.path == chart.PATH_REDUCE
    bg = background(1, 64, 256, 4)
    out = engine.chart_series(torch.from_numpy(t.copy()).to(engine.device), [p], torch.from_numpy(bg).to(engine.device))
    np.testing.assert_array_equal(out.cpu().numpy()[0], over(bg[0], want))
    # rare excursions: a column's interval is its min .. max, which one frame in a thousand decides
    rare = np.full((4, 300000), 3, dtype=np.int32)
    rare[0, 123456], rare[1, 299999], rare[2, 0], rare[3, 150000:150002] = 6, 0, 6, (0, 6)
    want = chart.series_numpy(rare, p)
    out = engine.chart_series(torch.from_numpy(rare).to(engine.device), [p], torch.from_numpy(bg).to(engine.device))
    np.testing.assert_array_equal(out.cpu().numpy()[0], over(bg[0], want))


def test_indices_past_2_to_the_31(engine):
    """A table of 4 x 720 000 000 int32 (11.5 GB): series 3 starts 2.16e9 elements in.  Chart 0 is all of it but the last 1000
    frames, class 0 throughout -- a level line, as any constant table of T >= pw gives --, chart 1 the last 1000 frames."""
    total = 720_000_000
    if torch.cuda.mem_get_info(engine.device)[0] < 16 * 2 ** 30:
        pytest.skip("needs 16 GB of free device memory")
    t, p1, want1 = cc.reference("random", 1000)
    table = torch.zeros((4, total), dtype=torch.int32, device=engine.device)
    table[:, total - 1000:] = torch.from_numpy(t.copy()).to(engine.device)
    p0 = p1.with_T(total - 1000)
    want0 = chart.series_numpy(np.zeros((4, 2 * p1.pw), dtype=np.int32), p1.with_T(2 * p1.pw))
    bg = background(2, cc.HEIGHT, cc.WIDTH, 2)
    out = engine.chart_series(table, [p0, p1], torch.from_numpy(bg).to(engine.device)).cpu().numpy()
    del table
    np.testing.assert_array_equal(out[0], over(bg[0], want0))
    np.testing.assert_array_equal(out[1], over(bg[1], want1))


def test_write_charts_files_are_pils(engine, tmp_path):
    import io

    from PIL import Image

    refs = [cc.reference("ramp", 7), cc.reference("random", 1000)]
    table = torch.from_numpy(np.concatenate([r[0] for r in refs], axis=1)).to(engine.device)
    for entropy in ("device", "host"):
        paths = [tmp_path / entropy / "a.jpg", tmp_path / entropy / "deep" / "b.jpg"]
        assert chart.write_charts(engine, table, paths, entropy=entropy, T=[7, 1000], plan=refs[0][1]) == [str(p) for p in paths]
        for path, (t, p, _) in zip(paths, refs):
            b = io.BytesIO()
            Image.fromarray(chart.chart_numpy(t, p)).save(b, "JPEG", quality=95, subsampling=2)
            assert path.read_bytes() == b.getvalue(), (entropy, path.name)


def test_errors_leave_the_engine_usable(engine):
    t, p, want = cc.reference("ramp", 7)
    td = torch.from_numpy(t.copy()).to(engine.device)
    white = np.full((1, p.height, p.width, 3), 255, dtype=np.uint8)

    def fresh(n=1):
        return torch.from_numpy(np.repeat(white, n, axis=0)).to(engine.device)

    def good():
        np.testing.assert_array_equal(engine.chart_series(td, [p], fresh()).cpu().numpy()[0], over(white[0], want))

    bad_class = t.copy()
    bad_class[2, 3] = 7
    bad_calls = [
        lambda: engine.chart_series(td.float(), [p], fresh()),                                # dtype
        lambda: engine.chart_series(td[:, ::2], [p.with_T(4)], fresh()),                      # not contiguous
        lambda: engine.chart_series(td[0], [p], fresh()),                                     # shape
        lambda: engine.chart_series(td.cpu(), [p], fresh()),                                  # not on the device
        lambda: engine.chart_series(torch.cat([td, td[:1]]), [p], fresh()),                   # five series
        lambda: engine.chart_series(td, [p.with_T(6)], fresh()),                              # plans do not fill the table
        lambda: engine.chart_series(td, [p], fresh(2)),                                       # one picture per chart
        lambda: engine.chart_series(td, [p], fresh()[:, :, :-1].contiguous()),                # another picture size
        lambda: engine.chart_series(td, [p], fresh(), colours=[(1, 2, 3)]),
        lambda: chart.render(engine, torch.from_numpy(bad_class).to(engine.device), plan=p),  # a class outside 0..6
        lambda: chart.render(engine, -td - 1, plan=p),
        lambda: chart.render(engine, td, T=[3, 3], plan=p),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
        good()
    # the C entry's own checks on the plan records
    host = p.record(0)
    dev = torch.from_numpy(host.view(np.uint8)).to(engine.device)
    out = fresh()
    ink = np.ascontiguousarray(chart.COLOURS, dtype=np.uint8).reshape(-1)

    def entry(rec=host, table=td.data_ptr(), elem=4, series=4, stride=7, h=p.height, w=p.width):
        return engine.lib.avcer_chart_series(engine.ctx, table, elem, series, stride, rec.ctypes.data, dev.data_ptr(), 1, out.data_ptr(), h, w,
                                             ink.ctypes.data, engine._stream())

    assert entry() == 0
    np.testing.assert_array_equal(out.cpu().numpy()[0], over(white[0], want))

    def broken(**kw):
        rec = host.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec

    for kw in (dict(table=None), dict(elem=2), dict(series=5), dict(series=0), dict(stride=0), dict(h=0), dict(w=16385),
               dict(rec=broken(pw=0)), dict(rec=broken(pw=p.width)), dict(rec=broken(ph=p.height)), dict(rec=broken(x0=-1)),
               dict(rec=broken(length=0)), dict(rec=broken(length=8)), dict(rec=broken(offset=1)), dict(rec=broken(offset=-1)),
               dict(rec=broken(yc=[p.y0 - 1] * 7)), dict(rec=broken(yc=[p.y0 + p.ph] * 7))):
        assert entry(**kw) == -1, kw
        assert len(engine.lib.avcer_last_error(engine.ctx)) > 0
        good()
