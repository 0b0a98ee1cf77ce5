"""avcer_amd/resize.py on the CPU: resize_numpy -- the statement the kernel is tested against -- equals PIL.Image.resize at tolerance
zero for the four covered filters, resize_plan's refusals, the int-size rule, and ScaledDetector's mapping back to source pixels
with a stub detector (no device)."""
import numpy as np
import pytest
from PIL import Image

from avcer_amd import face_tiles as ft
from avcer_amd import resize as rs

PIL_FILTERS = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
               "lanczos": Image.Resampling.LANCZOS}
# (H, W, h2, w2): down, up, one axis each, 1 x 1, a long row, the unchanged size, a realistic frame
SIZES = [(360, 640, 120, 213), (37, 53, 16, 16), (16, 16, 37, 53), (33, 47, 33, 20), (33, 47, 11, 47), (9, 7, 1, 1), (5, 300, 5, 7),
         (64, 64, 64, 64)]


def picture(h, w, seed=0, stripes=False):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if stripes:  # 0 / 255 rows: bicubic and lanczos leave [0, 255] on both ends
        img[::2] = 255
        img[1::2] = 0
    return img


@pytest.mark.parametrize("name", sorted(PIL_FILTERS))
@pytest.mark.parametrize("h,w,h2,w2", SIZES)
def test_resize_numpy_equals_pil(h, w, h2, w2, name):
    for stripes in (False, True):
        img = picture(h, w, h * 1000 + w, stripes)
        want = np.asarray(Image.fromarray(img).resize((w2, h2), PIL_FILTERS[name]))
        got = rs.resize_numpy(img, (h2, w2), name)
        assert got.dtype == np.uint8 and got.shape == (h2, w2, 3)
        np.testing.assert_array_equal(got, want)


def test_stripes_reach_both_ends_of_the_clip():
    """Why the striped picture is in the list: upscaled, bicubic's and lanczos' sums leave [0, 255] on BOTH sides, so both ends of the
    clip decide pixels."""
    col = np.where(np.arange(16) % 2 == 0, 255, 0)
    for name in ("bicubic", "lanczos"):
        plan = rs.resize_plan(16, 37, name)
        sums = [(int((plan.kk[o, :plan.count[o]].astype(np.int64) * col[plan.first[o]:plan.first[o] + plan.count[o]]).sum()) + (1 << 21)) >> 22
                for o in range(37)]
        assert min(sums) < 0 and max(sums) > 255, name


def test_batch_and_unchanged_size():
    batch = np.stack([picture(33, 47, s) for s in (1, 2, 3)])
    got = rs.resize_numpy(batch, (11, 20), "bicubic")
    for i in range(3):
        np.testing.assert_array_equal(got[i], np.asarray(Image.fromarray(batch[i]).resize((20, 11), Image.Resampling.BICUBIC)))
    np.testing.assert_array_equal(rs.resize_numpy(batch, (33, 47), "lanczos"), batch)
    # the identity plan of an unchanged axis reproduces its input
    ident = rs.resize_plan(47, 47, "lanczos")
    assert ident.ksize == 1 and (ident.count == 1).all() and (ident.first == np.arange(47)).all() and (ident.kk == 1 << 22).all()
    np.testing.assert_array_equal(rs._pass(batch[0], ident, 1), batch[0])


def test_plan_tables_stay_inside_the_source():
    for (h, w, h2, w2) in SIZES + [(1080, 1920, 360, 640), (600, 8, 2, 8)]:
        for name in PIL_FILTERS:
            for a, b in ((h, h2), (w, w2)):
                p = rs.resize_plan(a, b, name)
                assert (p.first >= 0).all() and (p.count >= 1).all() and (p.count <= p.ksize).all() and (p.first + p.count <= a).all()
                assert p.packed().dtype == np.int32 and p.packed().shape == (b * (2 + p.ksize),)


def test_plan_refusals():
    for bad in ("hamming", "nearest", "area", "", None, 2):
        with pytest.raises(ValueError, match="box.*bilinear.*bicubic.*lanczos"):
            rs.resize_plan(10, 5, bad)
    for name in ("hamming", "nearest"):
        with pytest.raises(ValueError, match=name):
            rs.resize_plan(10, 5, name)
    for a, b in ((0, 5), (5, 0), (8193, 5), (5, 8193), (True, 5), (5.0, 5)):
        with pytest.raises(ValueError, match="1..8192"):
            rs.resize_plan(a, b, "box")
    assert rs.resize_plan(8192, 1, "box").ksize == 8193
    with pytest.raises(ValueError):
        rs.resize_numpy(np.zeros((4, 4, 3), np.float32), (2, 2))
    with pytest.raises(ValueError):
        rs.resize_numpy(np.zeros((4, 4, 3), np.uint8), (2, 2, 2))


def test_int_size_rule():
    assert rs.target_size(1080, 1920, 640) == (360, 640)
    assert rs.target_size(1920, 1080, 640) == (640, 360)
    assert rs.target_size(37, 53, 16) == (max(1, int(37 * 16 / 53 + 0.5)), 16) == (11, 16)
    assert rs.target_size(3, 1000, 10) == (1, 10)       # never below one pixel
    assert rs.target_size(37, 53, (16, 20)) == (16, 20)
    for bad in (0, -3, True, 2.5, "640", (1, 2, 3), (0, 5), (5.0, 5), None):
        with pytest.raises(ValueError, match="detect size"):
            rs.target_size(37, 53, bad)


class Stub:
    """A detector that returns fixed rows and records what it was given."""
    gflop_per_frame = 50.7
    kind = 1

    def __init__(self, rows):
        self.rows, self.seen, self.engine = rows, [], self

    def resize_frames(self, frames, size, filter):  # the engine's part: the stub is its own engine
        self.seen.append(("resize", tuple(frames.shape), tuple(size), filter))
        return frames[:, :size[0], :size[1]]

    device = "cpu"

    def batch(self, frames, rgb=False):
        self.seen.append(("batch", tuple(frames.shape), rgb))
        return [self.rows.copy() for _ in range(frames.shape[0])]

    def __call__(self, image, rgb=True):
        self.seen.append(("call", tuple(image.shape), rgb))
        return self.rows.copy()


@pytest.mark.parametrize("width", [15, 5])
def test_scaled_detector_maps_rows_back(width):
    rows = (np.arange(2 * width, dtype=np.float32).reshape(2, width) * np.float32(1.37) + np.float32(0.21))
    stub = Stub(rows)
    det = ft.ScaledDetector(stub, (11, 20), "lanczos")
    frames = np.zeros((3, 33, 47, 3), np.uint8)
    got = det.batch(frames, rgb=False)
    assert stub.seen == [("resize", (3, 33, 47, 3), (11, 20), "lanczos"), ("batch", (3, 11, 20, 3), False)]
    sx, sy = np.float32(47) / np.float32(20), np.float32(33) / np.float32(11)
    want = rows.copy()
    for c in range(width):
        if c in (0, 2, 5, 7, 9, 11, 13):
            want[:, c] = rows[:, c] * sx
        elif c in (1, 3, 6, 8, 10, 12, 14):
            want[:, c] = rows[:, c] * sy
    assert len(got) == 3
    for g in got:
        assert g.dtype == np.float32 and g.shape == (2, width)
        np.testing.assert_array_equal(g, want)
        np.testing.assert_array_equal(g[:, 4], rows[:, 4])   # the score is untouched
    np.testing.assert_array_equal(det(frames[0], rgb=True), want)
    assert stub.seen[-1] == ("call", (11, 20, 3), True)
    # priced at the network's work on the smaller copy; kind keeps run_dataset off the R50 constant
    assert det.kind != 1 and det.gflop_per_frame == pytest.approx(50.7 * (11 * 20) / (33 * 47))
    assert det.gflop_at(1080, 1920) == pytest.approx(50.7 * (11 * 20) / (1080 * 1920))


def test_scaled_detector_pass_through_and_refusals():
    rows = np.ones((1, 15), np.float32)
    frames = np.zeros((2, 33, 47, 3), np.uint8)
    for size in ((33, 47), 47, 4096):
        stub = Stub(rows)
        det = ft.ScaledDetector(stub, size)
        got = det.batch(frames, rgb=False)
        assert stub.seen == [("batch", (2, 33, 47, 3), False)]    # the identical call: nothing is resized, nothing is mapped
        np.testing.assert_array_equal(got[0], rows)
        assert det.gflop_per_frame == 50.7
    for size in ((34, 47), (33, 48), (66, 94), (11, 48)):
        with pytest.raises(ValueError, match="upscaling"):
            ft.ScaledDetector(Stub(rows), size).batch(frames)
    for bad in ("640", 0, True, (1, 2, 3), 1.5):
        with pytest.raises(ValueError, match="detect size"):
            ft.ScaledDetector(Stub(rows), bad)
    with pytest.raises(ValueError, match="lanczos"):
        ft.ScaledDetector(Stub(rows), 16, "hamming")
    # the options' check, as the entry points make it
    ft.check_detect_size(None, "bilinear", None, [rows])
    assert ft.scaled_detector(Stub(rows), None) .__class__ is Stub
    with pytest.raises(ValueError, match="nothing would use it"):
        ft.check_detect_size(16, "bilinear", None, [rows])
    with pytest.raises(ValueError, match="upscaling"):
        ft.check_detect_size((64, 64), "bilinear", Stub(rows), None, (33, 47))
    with pytest.raises(ValueError, match="detect size"):
        ft.check_detect_size("big", "bilinear", Stub(rows), None)
    with pytest.raises(ValueError, match="lanczos"):
        ft.check_detect_size(None, "cubic", Stub(rows), None)
