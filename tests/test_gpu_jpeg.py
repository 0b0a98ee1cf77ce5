"""The device half of the JPEG crop decoder (csrc/jpeg_decode.hip avcer_jpeg_tiles / avcer_jpeg_rgb, avcer_amd/jpeg.py) against
tests/golden/jpeg_crops.npz -- PIL's decode of each file, written on the machine that ran tests/golden/make_jpeg_golden.py.  For a
file the decoder supports no test here calls PIL's JPEG decoder: expected tiles are PIL's NEAREST resize of the golden RGB array."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from avcer_amd import jpeg, video_pipeline
from avcer_amd.engine import MODE_F16X3

pytestmark = pytest.mark.gpu
FALLBACKS = {"100x75_rgb_progressive", "40x30_png_named_jpg", "100x75_rgb_cut40", "40x30_cmyk"}


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("jpeg_crops")
    return [(str(n), g[f"jpg_{i}"].tobytes(), bool(g["handled"][i]), np.cumsum(g[f"rgbdx_{i}"], axis=1, dtype=np.uint8) if f"rgbdx_{i}" in g.files else None)  # undo_dx of make_jpeg_golden
            for i, n in enumerate(g["names"])]


@pytest.fixture(scope="module")
def supported(cases):
    """(names, files, golden RGB, expected tiles) of the supported fixtures; computed once, never written to."""
    keep = [c for c in cases if c[2]]
    tiles = np.stack([np.asarray(Image.fromarray(c[3]).resize((224, 224), Image.Resampling.NEAREST)) for c in keep])
    tiles.setflags(write=False)
    return [c[0] for c in keep], [c[1] for c in keep], [c[3] for c in keep], tiles


def _device_inputs(engine, blobs):
    """Host entropy pass into plain numpy buffers, copied to the device: what Engine.jpeg_tiles / jpeg_rgb take."""
    coeffs = np.zeros(64 * (sum(len(b) for b in blobs) + 1024), dtype=np.int16)
    desc = np.zeros(len(blobs), dtype=jpeg.DESC)
    jpeg.entropy_batch(engine.lib, blobs, coeffs, desc, 0, engine.ctx)
    used = int((desc["coef_block"] + desc["n_blocks"]).max())
    c = torch.from_numpy(coeffs[:64 * used]).to(engine.device)
    d = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(engine.device)
    return c, d, used, desc


def _tiles(engine, c, d, n, used):
    tiles, flags = engine.jpeg_tiles(c, d, n, used)
    assert not flags.cpu().numpy().any()
    return tiles.cpu().numpy()


def _canvas(engine, c, d, n, used, hmax, wmax):
    canvas, flags = engine.jpeg_rgb(c, d, n, used, hmax, wmax)
    assert not flags.cpu().numpy().any()
    return canvas.cpu().numpy()


def test_tiles_and_canvas_of_every_supported_fixture_in_one_call(engine, supported):
    names, blobs, rgbs, tiles = supported
    c, d, used, desc = _device_inputs(engine, blobs)
    assert (desc["status"] == jpeg.OK).all()
    got = _tiles(engine, c, d, len(blobs), used)
    for i, name in enumerate(names):
        np.testing.assert_array_equal(got[i], tiles[i], err_msg=name)
    hmax, wmax = max(r.shape[0] for r in rgbs), max(r.shape[1] for r in rgbs)
    canvas = _canvas(engine, c, d, len(blobs), used, hmax, wmax)
    for i, (name, rgb) in enumerate(zip(names, rgbs)):
        h, w = rgb.shape[:2]
        np.testing.assert_array_equal(canvas[i, :h, :w], rgb, err_msg=name)
        assert not canvas[i, h:].any() and not canvas[i, :, w:].any(), name
    # a canvas wider than every image, of odd width: rows that are no multiple of 4 bytes
    wide = _canvas(engine, c, d, len(blobs), used, hmax + 3, wmax + 2)
    np.testing.assert_array_equal(wide[:, :hmax, :wmax], canvas)
    assert not wide[:, hmax:].any() and not wide[:, :, wmax:].any()


def test_a_file_alone_equals_its_rows_of_the_batch_and_a_permutation_permutes(engine, supported):
    """Batch invariance.  The batch call's rows are the goldens (the test above holds them to that), so a file decoded alone is held
    to its golden too: every supported fixture, its tile and its full-size image in a canvas of exactly its own size."""
    names, blobs, rgbs, tiles = supported
    for i, (name, blob, rgb) in enumerate(zip(names, blobs, rgbs)):
        c, d, used, _ = _device_inputs(engine, [blob])
        np.testing.assert_array_equal(_tiles(engine, c, d, 1, used)[0], tiles[i], err_msg=name)
        np.testing.assert_array_equal(_canvas(engine, c, d, 1, used, rgb.shape[0], rgb.shape[1])[0], rgb, err_msg=name)
    perm = np.random.default_rng(3).permutation(len(blobs))
    c, d, used, _ = _device_inputs(engine, [blobs[i] for i in perm])
    np.testing.assert_array_equal(_tiles(engine, c, d, len(blobs), used), tiles[perm])
    hmax, wmax = max(r.shape[0] for r in rgbs), max(r.shape[1] for r in rgbs)
    canvas = _canvas(engine, c, d, len(blobs), used, hmax, wmax)
    for k, i in enumerate(perm):
        h, w = rgbs[i].shape[:2]
        np.testing.assert_array_equal(canvas[k, :h, :w], rgbs[i], err_msg=names[i])
        assert not canvas[k, h:].any() and not canvas[k, :, w:].any(), names[i]


def _pil_tile(blob):
    with Image.open(io.BytesIO(blob)) as img:
        return np.asarray(img.convert("RGB").resize((224, 224), Image.Resampling.NEAREST))


def test_decode_tiles_with_the_fallbacks_equals_the_pil_path_and_names_them(engine, cases, supported):
    ok = [c for c in cases if c[0] != "100x75_rgb_cut40"]
    got, paths = jpeg.decode_tiles(engine, [c[1] for c in ok])
    got = got.cpu().numpy()
    assert {c[0] for c, p in zip(ok, paths) if p == "pil"} == FALLBACKS - {"100x75_rgb_cut40"}
    assert set(paths) == {"device", "pil"}
    tiles = dict(zip(supported[0], supported[3]))
    for i, (name, blob, handled, rgb) in enumerate(ok):
        # a supported file against its golden; a fallback against the PIL lines themselves (that IS its path)
        np.testing.assert_array_equal(got[i], tiles[name] if handled else _pil_tile(blob), err_msg=name)
    (canvas, rects), cpaths = jpeg.decode_canvas(engine, [c[1] for c in ok])
    assert cpaths == paths
    canvas = canvas.cpu().numpy()
    for i, (name, blob, handled, rgb) in enumerate(ok):
        if not handled:
            with Image.open(io.BytesIO(blob)) as img:
                rgb = np.asarray(img.convert("RGB"))
        h, w = rgb.shape[:2]
        assert rects[i].tolist() == [i, 0, 0, w, h], name
        np.testing.assert_array_equal(canvas[i, :h, :w], rgb, err_msg=name)
        assert not canvas[i, h:].any() and not canvas[i, :, w:].any(), name
    # the truncated file: whatever PIL does with it is what the caller sees, through both paths
    cut = next(c[1] for c in cases if c[0] == "100x75_rgb_cut40")
    with pytest.raises(OSError):
        _pil_tile(cut)
    with pytest.raises(OSError):
        jpeg.decode_tiles(engine, [ok[0][1], cut])
    with pytest.raises(OSError):
        jpeg.decode_canvas(engine, [ok[0][1], cut])


def test_a_corrupt_table_raises_the_range_flag_and_the_file_goes_to_pil(engine, cases, supported):
    """A baseline file with two quantisation steps turned into 214 and 202: the stream parses, but the inverse DCT leaves the range
    in which libjpeg's C and SIMD code agree (tests/test_jpeg_host.py states the numbers).  The device flags it and leaves it zero, its
    neighbours in the batch are untouched, and decode_tiles / decode_canvas hand it to PIL."""
    names, blobs, _, tiles = supported
    k = names.index("7x9_rgb_s0_q95")
    wild = bytearray(blobs[k])
    wild[94], wild[381] = 0xD6, 0xCA
    batch = [blobs[0], bytes(wild), blobs[k]]
    c, d, used, desc = _device_inputs(engine, batch)
    assert (desc["status"] == jpeg.OK).all()
    got, flags = engine.jpeg_tiles(c, d, 3, used)
    assert flags.cpu().tolist() == [0, 1, 0]
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got[0], tiles[0])
    np.testing.assert_array_equal(got[2], tiles[k])
    assert not got[1].any()
    canvas, flags = engine.jpeg_rgb(c, d, 3, used, 9, 7)
    assert flags.cpu().tolist() == [0, 1, 0] and not canvas[1].cpu().numpy().any()
    out, paths = jpeg.decode_tiles(engine, batch)
    assert paths == ["device", "pil", "device"]
    np.testing.assert_array_equal(out[1].cpu().numpy(), _pil_tile(bytes(wild)))
    (canvas, rects), paths = jpeg.decode_canvas(engine, batch[1:])
    assert paths == ["pil", "device"] and rects.tolist() == [[0, 0, 0, 7, 9], [1, 0, 0, 7, 9]]
    with Image.open(io.BytesIO(bytes(wild))) as img:
        np.testing.assert_array_equal(canvas[0].cpu().numpy(), np.asarray(img.convert("RGB")))


@pytest.fixture(scope="module")
def eng(engine, sd_static, sd_dynamic):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    return engine


def test_crop_folder_through_the_device_readers_and_the_pipeline(eng, cases, tmp_path):
    """12 frames: two missing, one PNG under a .jpg name, one progressive file, eight baseline files of all three samplings and grey."""
    by = {c[0]: c[1] for c in cases}
    order = ["203x187_rgb_s2_q95", "100x75_rgb_s1_q95", None, "40x30_png_named_jpg", "100x75_rgb_s0_q95", "203x187_l_q95",
             "100x75_rgb_progressive", "52x37_rgb_s2_q95_rst3", None, "17x33_rgb_s2_q95", "40x40_rgb_s2_q95_exif_comment",
             "100x75_rgb_s2_q95_rstrow"]
    folder = tmp_path / "clip" / "00"
    os.makedirs(folder)
    for i, name in enumerate(order):
        if name is not None:
            (folder / f"{i:06d}.jpg").write_bytes(by[name])
    path = str(tmp_path / "clip")
    frames, present = video_pipeline.read_face_dir(path, 12)
    dframes, dpresent = video_pipeline.read_face_dir_device(eng, path, 12)
    assert dframes.is_cuda and dpresent.tolist() == present.tolist() == [n is not None for n in order]
    np.testing.assert_array_equal(dframes.cpu().numpy(), frames)
    canvas, rects = video_pipeline.read_face_crops(path, [0, 3, 6, 9])
    dcanvas, drects = video_pipeline.read_face_crops_device(eng, path, [0, 3, 6, 9])
    np.testing.assert_array_equal(dcanvas.cpu().numpy(), canvas)
    np.testing.assert_array_equal(drects, rects)
    with pytest.raises(FileNotFoundError):
        video_pipeline.read_face_dir_device(eng, str(tmp_path / "nowhere"), 12)
    with pytest.raises(ValueError):
        video_pipeline.preprocess_video_and_predict(eng, path, str(tmp_path), 5, 12, decode="cv2")

    out = {}
    for decode in ("pil", "device"):
        save = str(tmp_path / decode)
        d0, s0 = video_pipeline.preprocess_video_and_predict(eng, path, save, 5, 12, mode=MODE_F16X3, decode=decode)
        d1, s1 = video_pipeline.preprocess_video_and_predict(eng, path, save, 5, 12, mode=MODE_F16X3, flag_heatmaps=True, decode=decode)
        np.testing.assert_array_equal(d0, d1)
        np.testing.assert_array_equal(s0, s1)
        hdir = os.path.join(save, "clip", "heatmaps_static")
        out[decode] = (d0, s0, {n: open(os.path.join(hdir, n), "rb").read() for n in sorted(os.listdir(hdir))})
    np.testing.assert_array_equal(out["device"][0], out["pil"][0])
    np.testing.assert_array_equal(out["device"][1], out["pil"][1])
    assert out["device"][2] and out["device"][2] == out["pil"][2]
    # the default is the device path
    d, s = video_pipeline.preprocess_video_and_predict(eng, path, str(tmp_path / "default"), 5, 12, mode=MODE_F16X3)
    np.testing.assert_array_equal(d, out["pil"][0])
    np.testing.assert_array_equal(s, out["pil"][1])


def test_300_tiny_files_in_one_call(engine):
    """300 files of 8 x 8 to 24 x 24 pixels, encoded here (PIL's ENCODER only): several images per kernel-A workgroup and planes
    of one to nine blocks, so an index that mixes up images or MCU-padded planes cannot stay hidden.  All 300 go through ONE launch
    of each kernel (there is no multi-launch path: the grid grows with the blocks and the pixels).

    Expected: jpeg.pixels_numpy on the same coefficients.  That is a restatement of the kernels and no PIL golden -- PIL's decoder
    may not run here, and 300 goldens would not fit the archive -- so it is independent of the kernels only through the CPU suite:
    tests/test_jpeg_host.py holds pixels_numpy to PIL's decode bit for bit on every fixture and on 200 random files drawn from the
    same sizes-and-parameters grid as these."""
    rng = np.random.default_rng(11)
    blobs = []
    for t in range(300):
        w, h = int(rng.integers(8, 25)), int(rng.integers(8, 25))
        mode = "L" if t % 6 == 0 else "RGB"
        a = rng.integers(0, 256, (h, w, 3) if mode == "RGB" else (h, w)).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(a, mode).save(b, "JPEG", quality=(95, 75, 20)[t % 3], subsampling=int(rng.integers(0, 3)))
        blobs.append(b.getvalue())
    c, d, used, desc = _device_inputs(engine, blobs)
    assert (desc["status"] == jpeg.OK).all()
    want = jpeg.pixels_numpy(c.cpu().numpy(), desc)
    got = _tiles(engine, c, d, 300, used)
    canvas = _canvas(engine, c, d, 300, used, 24, 24)
    for i, rgb in enumerate(want):
        h, w = rgb.shape[:2]
        np.testing.assert_array_equal(canvas[i, :h, :w], rgb, err_msg=f"file {i}")
        assert not canvas[i, h:].any() and not canvas[i, :, w:].any()
        np.testing.assert_array_equal(got[i], np.asarray(Image.fromarray(rgb).resize((224, 224), Image.Resampling.NEAREST)),
                                      err_msg=f"file {i}")
    tiles, paths = jpeg.decode_tiles(engine, blobs)
    assert paths == ["device"] * 300
    np.testing.assert_array_equal(tiles.cpu().numpy(), got)
