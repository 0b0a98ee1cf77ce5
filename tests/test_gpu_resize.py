"""avcer_resize_frames (csrc/resize.hip) against resize.resize_numpy -- which tests/test_resize_cpu.py holds to PIL -- at tolerance
zero: both forms by name, the chooser, batches of distinct frames, stripes for the clip, a guard band round the output, and the
argument checks."""
import numpy as np
import pytest
import torch

import guard_band as gb
from avcer_amd import resize as rs

pytestmark = pytest.mark.gpu

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
# (H, W, h2, w2): 3 * W odd and unaligned, no size a multiple of a tile; down, up, one axis each, 1 x 1, a long row
CASES = [(37, 53, 16, 16), (16, 16, 37, 53), (33, 47, 33, 20), (33, 47, 11, 47), (9, 7, 1, 1), (5, 300, 5, 7)]
_REF = {}


def batch(n, h, w, stripes=False):
    """n DISTINCT frames; with stripes, 0 / 255 rows in one frame and columns in the next (the clip's both ends, both axes)."""
    x = np.random.default_rng(h * 10007 + w * 31 + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if stripes:
        for i in range(n):
            if i % 2 == 0:
                x[i, ::2], x[i, 1::2] = 255, 0
            else:
                x[i, :, ::2], x[i, :, 1::2] = 255, 0
    return x


def ref(n, h, w, h2, w2, name, stripes):
    key = (n, h, w, h2, w2, name, stripes)
    if key not in _REF:
        x = batch(n, h, w, stripes)
        want = rs.resize_numpy(x, (h2, w2), name)
        want.setflags(write=False)
        _REF[key] = (x, want)
    return _REF[key]


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("h,w,h2,w2", CASES)
def test_kernel_equals_resize_numpy_in_both_forms(engine, h, w, h2, w2, name):
    for n in (1, 3):
        for stripes in (False, True):
            x, want = ref(n, h, w, h2, w2, name, stripes)
            xd = torch.from_numpy(x).to(engine.device)
            for form in (rs.FORM_CHOOSE, rs.FORM_FUSED, rs.FORM_TWO_PASS):
                got = engine.resize_frames(xd, (h2, w2), name, form=form)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h2, w2, 3)
                np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"n={n} stripes={stripes} form={form}")
            assert torch.equal(xd.cpu(), torch.from_numpy(x))


def test_the_chooser():
    """From the plan alone, no launch: 1080 -> 360 (and the 4 x bilinear, 3 x lanczos downscales the tile is sized for) take the fused
    form; a vertical support that cannot fit a tile takes the general one."""
    from avcer_amd import _lib

    lib = _lib.load()

    def form(a, b, name):
        tab = rs.resize_plan(a, b, name).packed()
        return lib.avcer_resize_form(tab.ctypes.data, b)

    assert form(1080, 360, "bilinear") == rs.FORM_FUSED
    assert form(1080, 270, "bilinear") == rs.FORM_FUSED and form(1080, 360, "lanczos") == rs.FORM_FUSED
    assert form(720, 360, "bilinear") == rs.FORM_FUSED and form(16, 37, "lanczos") == rs.FORM_FUSED
    assert form(600, 2, "lanczos") == rs.FORM_TWO_PASS
    assert lib.avcer_resize_form(None, 4) < 0 and form(600, 2, "lanczos") > 0


def test_support_too_tall_for_a_tile_takes_the_general_form(engine):
    """600 x 8 -> 2 x 8 lanczos: one output row reads 600 source rows.  The chooser's result equals the general form's and the
    statement; the fused form by name is refused, and the engine works on."""
    x, want = ref(2, 600, 8, 2, 8, "lanczos", False)
    xd = torch.from_numpy(x).to(engine.device)
    assert engine.resize_form(600, 2, "lanczos") == rs.FORM_TWO_PASS
    for form in (rs.FORM_CHOOSE, rs.FORM_TWO_PASS):
        np.testing.assert_array_equal(engine.resize_frames(xd, (2, 8), "lanczos", form=form).cpu().numpy(), want)
    with pytest.raises(Exception, match="fused form"):
        engine.resize_frames(xd, (2, 8), "lanczos", form=rs.FORM_FUSED)
    np.testing.assert_array_equal(engine.resize_frames(xd, (2, 8), "lanczos").cpu().numpy(), want)


def test_tile_edges_at_a_realistic_size(engine):
    """2 frames of 360 x 640 -> 120 x 213 bilinear: several tiles on both axes, the last ones cut, rows of 639 bytes."""
    x, want = ref(2, 360, 640, 120, 213, "bilinear", False)
    xd = torch.from_numpy(x).to(engine.device)
    assert engine.resize_form(360, 120, "bilinear") == rs.FORM_FUSED
    for form in (rs.FORM_FUSED, rs.FORM_TWO_PASS):
        np.testing.assert_array_equal(engine.resize_frames(xd, (120, 213), "bilinear", form=form).cpu().numpy(), want)


@pytest.mark.parametrize("form", [rs.FORM_FUSED, rs.FORM_TWO_PASS])
@pytest.mark.parametrize("h,w,h2,w2,name", [(37, 53, 16, 16, "lanczos"), (16, 16, 37, 53, "bicubic"), (33, 47, 11, 47, "bilinear"),
                                            (64, 128, 32, 64, "box")])
def test_guard_band(engine, h, w, h2, w2, name, form):
    """Nothing outside the output is written and all of it is (guard_band.check), with rows that are 4-byte aligned (64 * 3) and not."""
    x, want = ref(3, h, w, h2, w2, name, False)
    xd = torch.from_numpy(x).to(engine.device)
    out, = gb.check(lambda outs: engine.resize_frames(xd, (h2, w2), name, form=form, out=outs[0]),
                    [gb.Band("resized", (3, h2, w2, 3), torch.uint8, row_bytes=3 * w2)], inputs=[xd], device=engine.device)
    np.testing.assert_array_equal(out.numpy(), want)


def test_same_size_returns_the_batch_without_a_launch(engine):
    xd = torch.from_numpy(batch(2, 9, 7)).to(engine.device)
    assert rs.resize_frames(engine, xd, (9, 7), "lanczos") is xd
    out = torch.zeros_like(xd)
    assert engine.resize_frames(xd, (9, 7), "box", out=out) is out and torch.equal(out, xd)   # the identity tables copy


def test_errors_leave_the_engine_usable(engine):
    x, want = ref(1, 9, 7, 1, 1, "box", False)
    xd = torch.from_numpy(x).to(engine.device)

    def good():
        np.testing.assert_array_equal(engine.resize_frames(xd, (1, 1), "box").cpu().numpy(), want)

    bad_calls = [
        lambda: engine.resize_frames(xd.float(), (4, 4)),                                   # dtype
        lambda: engine.resize_frames(xd[:, :, ::2], (4, 4)),                                # not contiguous
        lambda: engine.resize_frames(xd[0], (4, 4)),                                        # shape
        lambda: engine.resize_frames(x, (4, 4)),                                            # not a device tensor
        lambda: engine.resize_frames(xd.cpu(), (4, 4)),
        lambda: engine.resize_frames(xd, (0, 4)),                                           # sides
        lambda: engine.resize_frames(xd, (4, 8193)),
        lambda: engine.resize_frames(xd, (4, 4), "hamming"),                                # filters
        lambda: engine.resize_frames(xd, (4, 4), "nearest"),
        lambda: engine.resize_frames(xd, (4, 4), out=torch.zeros(1, 4, 5, 3, dtype=torch.uint8, device=engine.device)),
        lambda: engine.resize_frames(xd, (4, 4), form=3),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
        good()
    # the C entry's own checks: a null pointer, a side out of range, a table that leaves the source
    lib, ctx = engine.lib, engine.ctx
    xp, yp = rs.resize_plan(7, 4, "box"), rs.resize_plan(9, 4, "box")
    xt, yt = xp.packed(), yp.packed()
    xd_t, yd_t = torch.from_numpy(xt).to(engine.device), torch.from_numpy(yt).to(engine.device)
    out = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=engine.device)

    def entry(src=xd.data_ptr(), h=9, w=7, h2=4, w2=4, xh=xt, yh=yt):
        return lib.avcer_resize_frames(ctx, src, 1, h, w, out.data_ptr(), h2, w2, xh.ctypes.data, xd_t.data_ptr(), xp.ksize, yh.ctypes.data,
                                       yd_t.data_ptr(), yp.ksize, 0, engine._stream())

    assert entry() == 0
    np.testing.assert_array_equal(out.cpu().numpy(), rs.resize_numpy(x, (4, 4), "box"))
    broken = xt.copy()
    broken[3] = 6          # first of the last output: 6 + count 2 > 7
    assert xp.first[3] == 5 and xp.count[3] == 2
    for kw in (dict(src=None), dict(h=0), dict(w=8193), dict(h2=0), dict(w2=8193), dict(xh=broken)):
        assert entry(**kw) == -1
        assert len(lib.avcer_last_error(ctx)) > 0
        good()
