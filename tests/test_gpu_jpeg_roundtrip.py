"""The JPEG round trip on the device (csrc/jpeg_encode.hip avcer_jpeg_roundtrip_tiles / _rgb, avcer_amd/jpeg.py roundtrip_tiles /
roundtrip_canvas) and the option built on it (`via_jpeg` of VideoTiler.process, `faces_via_jpeg` of run_inference and run_dataset):
the visual models see a face crop as the reference's stage 1 does, read back from the JPEG file stage 0 writes of it.  Held to PIL's
own round trip (Image.save -> Image.open, NEAREST to 224 for the tiles), to the composition of the encoder and the decoder that
were there before, and to the read-back path through real files.  No case has a tolerance."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from avcer_amd import face_tiles, heatmaps, jpeg, video_pipeline
from avcer_amd.engine import MODE_F16X3, MODE_FP32

pytestmark = pytest.mark.gpu

SUBSAMPLINGS = [0, 1, 2]
QUALITIES = [1, 50, 95, 100]
# (slot, x0, y0, x1, y1) in a [3, 64, 96, 3] source: the sizes 1x1, 1x17, 8x8, 9x7, 16x16, 17x15, 33x47 (w x h), every slot, and
# between them every edge of the tensor: left and top (1x1), right and bottom (1x17, 17x15), right and top (8x8), left and bottom
# (9x7), top (33x47), none (16x16)
SMALL = [(0, 0, 0, 1, 1), (1, 95, 47, 96, 64), (2, 88, 0, 96, 8), (0, 0, 57, 9, 64), (1, 40, 24, 56, 40), (2, 79, 49, 96, 64),
         (0, 31, 0, 64, 47)]
# 250x301 in a [1, 320, 320, 3] source, against its right and bottom edges: wider and taller than one 224-sample stride
LARGE = [(0, 70, 19, 320, 320)]


def _sources(shape):
    """(uniform u8 noise, a smooth gradient that differs from slot to slot) of `shape`; never written to."""
    rng = np.random.default_rng(shape[1] * 1000 + shape[2])
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    n, h, w, _ = shape
    ss, yy, xx = np.mgrid[0:n, 0:h, 0:w]
    grad = np.stack([xx * 255.0 / (w - 1), yy * 255.0 / (h - 1), ((xx + yy) * 255.0 / (w + h - 2) + 40 * ss) % 256], axis=3)
    grad = np.rint(grad).astype(np.uint8)
    noise.setflags(write=False)
    grad.setflags(write=False)
    return noise, grad


@pytest.fixture(scope="module")
def sources():
    """[(name, src u8 [N,H,W,3] on the host, the same on the device, rects)]"""
    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    out = []
    for shape, rects in (((3, 64, 96, 3), SMALL), ((1, 320, 320, 3), LARGE)):
        for name, src in zip(("noise", "gradient"), _sources(shape)):
            out.append((f"{name} {shape}", src, dev(src), rects))
    return out


def _pil_file(rgb, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(b, "JPEG", quality=int(quality), subsampling=int(subsampling))
    return b.getvalue()


def _pil_roundtrip(rgb, quality, subsampling):
    """(Image.open(file).convert("RGB"), its NEAREST resize to 224 x 224) of the file PIL writes of `rgb`."""
    with Image.open(io.BytesIO(_pil_file(rgb, quality, subsampling))) as img:
        full = img.convert("RGB")
        return np.array(full), np.asarray(full.resize((224, 224), Image.Resampling.NEAREST))


def _crops(src, rects, bgr):
    return [src[s, y0:y1, x0:x1, ::-1] if bgr else src[s, y0:y1, x0:x1] for s, x0, y0, x1, y1 in rects]


def _low_level(engine, src_dev, rects, quality, subsampling, bgr, keep=False, edit=None):
    """plan on the host, then the two native calls: (tiles, canvas, flags of both, coefficients of the first or None, DESC records)."""
    rects = np.asarray(rects, dtype=np.int32).reshape(-1, 5)
    desc, blocks = jpeg.plan(engine.lib, [(r[3] - r[1], r[4] - r[2]) for r in rects], quality, subsampling)
    assert (desc["status"] == jpeg.OK).all()
    if edit is not None:
        edit(desc)
    d_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(engine.device)
    r_dev = torch.from_numpy(rects).to(engine.device)
    n = len(rects)
    tiles, f1, coeffs = engine.jpeg_roundtrip_tiles(src_dev, r_dev, d_dev, n, blocks, bgr=bgr, keep_coeffs=keep)
    canvas, f2, _ = engine.jpeg_roundtrip_rgb(src_dev, r_dev, d_dev, n, blocks, int(desc["height"].max()), int(desc["width"].max()), bgr=bgr)
    return tiles, canvas, f1.cpu().numpy(), f2.cpu().numpy(), coeffs, desc, d_dev, blocks


# ---------------------------------------------------------------------------------------------------- (a) PIL, (b) flags
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_tiles_and_canvas_are_pils_round_trip(engine, sources, subsampling, quality):
    for name, src, src_dev, rects in sources:
        for bgr in (False, True):
            tiles = jpeg.roundtrip_tiles(engine, src_dev, rects, bgr=bgr, quality=quality, subsampling=subsampling)
            canvas, crects = jpeg.roundtrip_canvas(engine, src_dev, rects, bgr=bgr, quality=quality, subsampling=subsampling)
            assert tuple(tiles.shape) == (len(rects), 224, 224, 3) and tiles.dtype == torch.uint8
            tiles, canvas = tiles.cpu().numpy(), canvas.cpu().numpy()
            assert crects.tolist() == [[i, 0, 0, r[3] - r[1], r[4] - r[2]] for i, r in enumerate(rects)]
            for i, crop in enumerate(_crops(src, rects, bgr)):
                what = f"{name} image {i} {rects[i]} bgr {bgr} q{quality} s{subsampling}"
                full, tile = _pil_roundtrip(crop, quality, subsampling)
                h, w = full.shape[:2]
                np.testing.assert_array_equal(tiles[i], tile, err_msg=what)
                np.testing.assert_array_equal(canvas[i, :h, :w], full, err_msg=what)
                assert not canvas[i, h:].any() and not canvas[i, :, w:].any(), what


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_no_flag_is_raised_by_an_encoders_own_coefficients(engine, sources, subsampling, quality):
    for name, src, src_dev, rects in sources:
        for bgr in (False, True):
            _, _, f1, f2, _, _, _, _ = _low_level(engine, src_dev, rects, quality, subsampling, bgr)
            assert not f1.any() and not f2.any(), f"{name} bgr {bgr} q{quality} s{subsampling}: flags {f1.tolist()} {f2.tolist()}"


def test_a_descriptor_the_plan_did_not_write_is_flagged_and_yields_zeros(engine, sources):
    """The geometry is left alone (nothing is read or stored through a wrong one here): image 2's two chroma tables differ, which
    avcer_jpeg_plan never writes.  Its flag is 1, its outputs zero; its neighbours are served."""
    name, src, src_dev, rects = sources[0]

    def edit(desc):
        desc["qt"][2, 2, 5] += 1

    tiles, canvas, f1, f2, _, _, _, _ = _low_level(engine, src_dev, rects, 95, 2, False, edit=edit)
    good = jpeg.roundtrip_tiles(engine, src_dev, rects).cpu().numpy()
    assert f1.tolist() == f2.tolist() == [0, 0, 1, 0, 0, 0, 0]
    tiles, canvas = tiles.cpu().numpy(), canvas.cpu().numpy()
    assert not tiles[2].any() and not canvas[2].any()
    for i in (0, 1, 3, 4, 5, 6):
        np.testing.assert_array_equal(tiles[i], good[i])


# ---------------------------------------------------------------------------------------------------- (c) composition
@pytest.mark.parametrize("quality,subsampling", [(95, 2), (50, 1), (100, 0)])
def test_round_trip_is_decode_of_encode_and_its_coefficients_are_the_encoders(engine, sources, quality, subsampling):
    for name, src, src_dev, rects in sources:
        for bgr in (False, True):
            what = f"{name} bgr {bgr} q{quality} s{subsampling}"
            blobs = jpeg.encode_images(engine, src_dev, rects, bgr=bgr, quality=quality, subsampling=subsampling)
            tiles, coeffs, d_dev, desc = jpeg.roundtrip_tiles(engine, src_dev, rects, bgr=bgr, quality=quality, subsampling=subsampling,
                                                              keep_coeffs=True)
            for entropy in ("host", "device"):
                want, paths = jpeg.decode_tiles(engine, blobs, entropy=entropy)
                assert paths == ["device"] * len(rects)
                np.testing.assert_array_equal(tiles.cpu().numpy(), want.cpu().numpy(), err_msg=f"{what} entropy {entropy}")
            (canvas, _), c2, _, _ = jpeg.roundtrip_canvas(engine, src_dev, rects, bgr=bgr, quality=quality, subsampling=subsampling,
                                                          keep_coeffs=True)
            np.testing.assert_array_equal(canvas.cpu().numpy(), jpeg.decode_canvas(engine, blobs)[0][0].cpu().numpy(), err_msg=what)
            blocks = int((desc["coef_block"] + desc["n_blocks"]).max())
            r_dev = torch.from_numpy(np.asarray(rects, dtype=np.int32)).to(engine.device)
            fwd = engine.jpeg_forward(src_dev, r_dev, d_dev, len(rects), blocks, bgr=bgr).cpu().numpy().reshape(-1, 64)
            for c in (coeffs, c2):
                np.testing.assert_array_equal(c.cpu().numpy().reshape(-1, 64)[:blocks], fwd[:blocks], err_msg=what)
            for entropy in ("host", "device"):
                assert jpeg.files_from_coeffs(engine, coeffs, d_dev, desc, entropy=entropy) == blobs, f"{what} entropy {entropy}"
            for blob, crop in zip(blobs, _crops(src, rects, bgr)):
                assert blob == _pil_file(crop, quality, subsampling), what


# ---------------------------------------------------------------------------------------------------- (d) - (g) the option
@pytest.fixture(scope="module")
def clip():
    """12 BGR frames of 96 x 128 and scripted detections: track 00 in frames 0..10, a second track from frame 2 on, frame 11 with the
    second track alone."""
    rng = np.random.default_rng(47)
    yy, xx = np.mgrid[0:96, 0:128]
    bgr = np.stack([np.stack([np.sin(xx / (9.0 + c + t)) * 60 + np.cos(yy / (11.0 - c)) * 50 + 128 for c in range(3)], axis=2) for t in range(12)])
    bgr = np.clip(np.rint(bgr + rng.normal(0, 5, bgr.shape)), 0, 255).astype(np.uint8)
    dets = []
    for t in range(12):
        d = [[10.4 + 2 * t, 8.2 + t, 51.7 + 2 * t, 60.3 + t, 0.99]] if t < 11 else []
        if t >= 2:
            d.append([70.0 + t, 30.5, 111.0 + t, 85.9 - t, 0.95])
        dets.append(np.array(d, dtype=np.float32).reshape(-1, 5))
    return bgr, dets


@pytest.fixture(scope="module")
def eng(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


def _wav(frames=12, seed=99):
    from avcer_amd import synth

    return synth.waveforms(seed, 1, int(frames / 25 * 16000))[0]


RESULT_KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")


def _files(paths):
    return [open(p, "rb").read() for p in paths]


@pytest.mark.parametrize("mode", [MODE_F16X3, MODE_FP32])
def test_run_inference_equals_the_read_back_of_the_folder_it_writes(eng, clip, tmp_path, mode):
    from avcer_amd import run as arun

    bgr, dets = clip
    on = arun.run_inference(eng, bgr, _wav(), 25, detections=dets, mode=mode, name_video="clip", path_save_faces=str(tmp_path / "on"),
                            faces_via_jpeg=True)
    off = arun.run_inference(eng, bgr, _wav(), 25, detections=dets, mode=mode, name_video="clip", path_save_faces=str(tmp_path / "off"))
    rec = on["records"]
    assert sorted(set(rec[:, 1].tolist())) == [0, 1] and 11 not in rec[rec[:, 1] == 0, 0] and len(rec) == 21
    assert [os.path.relpath(p, tmp_path / "on") for p in on["face_files"]] == [os.path.relpath(p, tmp_path / "off") for p in off["face_files"]]
    assert _files(on["face_files"]) == _files(off["face_files"])
    dyn, stat = video_pipeline.preprocess_video_and_predict(eng, str(tmp_path / "on" / "clip"), fps=25, total_frames=12, mode=mode,
                                                            decode="device")
    np.testing.assert_array_equal(on["static_probs"], stat)
    np.testing.assert_array_equal(on["dynamic_logits"], dyn)
    assert not np.array_equal(on["static_probs"], off["static_probs"])  # the quantiser is seen by the network
    # without the folder: the same tiles, the same results
    bare = arun.run_inference(eng, bgr, _wav(), 25, detections=dets, mode=mode, faces_via_jpeg=True)
    assert "face_files" not in bare
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(bare[k], on[k], err_msg=k)


@pytest.mark.parametrize("model", heatmaps.MODELS)
def test_heat_map_base_is_the_linear_resize_of_the_read_back_crop(eng, clip, tmp_path, model):
    from avcer_amd import run as arun

    bgr, dets = clip
    on = arun.run_inference(eng, bgr, _wav(), 25, detections=dets, mode=MODE_FP32, name_video="clip", path_save_faces=str(tmp_path),
                            faces_via_jpeg=True, flag_heatmaps=True, model_heatmaps=model)
    folder = str(tmp_path / "clip")
    frames, present = video_pipeline.read_face_dir_device(eng, folder, 12)
    stat, dyn, cam, fidx, rows, cls = heatmaps.visual_forward_cam(eng, frames, present, 25, MODE_FP32, model)
    assert fidx.tolist() == [0, 5, 10]
    canvas, rects = video_pipeline.read_face_crops_device(eng, folder, fidx)
    base = eng.crop_resize_linear(canvas, rects, swap_rb=False)
    want = eng.cam_render(cam, rows, cls, base, heatmaps.JET_BGR, heatmaps.IMAGE_WEIGHT).cpu().numpy()
    assert on["heatmaps"][0].tolist() == [0, 5, 10]
    np.testing.assert_array_equal(on["heatmaps"][1], want)
    np.testing.assert_array_equal(on["static_probs"], stat.cpu().numpy())
    raw = arun.run_inference(eng, bgr, _wav(), 25, detections=dets, mode=MODE_FP32, flag_heatmaps=True, model_heatmaps=model)
    assert not np.array_equal(raw["heatmaps"][1], want)


def test_video_tiler_via_jpeg(eng, clip, tmp_path):
    bgr, dets = clip
    records, tiles = face_tiles.VideoTiler(eng).process(bgr, dets, via_jpeg=True)
    rec2, tiles2 = face_tiles.VideoTiler(eng).process(bgr, dets, save_path=str(tmp_path), video_name="v", entropy="device", via_jpeg=True)
    np.testing.assert_array_equal(records, rec2)
    np.testing.assert_array_equal(tiles.cpu().numpy(), tiles2.cpu().numpy())
    for i, (f, t, x0, y0, x1, y1) in enumerate(records):
        rgb = bgr[f, y0:y1, x0:x1, ::-1]
        np.testing.assert_array_equal(tiles[i].cpu().numpy(), _pil_roundtrip(rgb, 95, 2)[1], err_msg=str(records[i]))
        assert (tmp_path / "v" / f"{t:02d}" / f"{f:06d}.jpg").read_bytes() == _pil_file(rgb, 95, 2)


@pytest.mark.parametrize("mode", [MODE_F16X3, MODE_FP32])
def test_run_dataset_equals_run_inference_video_by_video(eng, clip, mode):
    from avcer_amd import run as arun
    from avcer_amd.dataset import VideoJob, run_dataset

    bgr, dets = clip
    jobs, want = [], []
    for k, t in enumerate((12, 9, 11)):
        frames, wav = np.ascontiguousarray(bgr[:t, :, ::-1] if k == 1 else bgr[:t]), _wav(t, 100 + k)
        jobs.append(VideoJob(f"v{k}", t, 96, 128, 25, len(wav), detections=dets[:t], load=lambda frames=frames, wav=wav: (frames, wav)))
        want.append(arun.run_inference(eng, frames, wav, 25, detections=dets[:t], mode=mode, faces_via_jpeg=True))
    got = run_dataset(eng, jobs, mode=mode, faces_via_jpeg=True)
    plain = run_dataset(eng, jobs, mode=mode)
    for g, w, p in zip(got, want, plain):
        for k in RESULT_KEYS:
            np.testing.assert_array_equal(g[k], w[k], err_msg=f"{g['name']} {k}")
        assert not np.array_equal(g["static_probs"], p["static_probs"])


def test_option_off_is_the_call_without_the_keyword(eng, clip, monkeypatch):
    from avcer_amd import run as arun

    def never(*a, **k):
        raise AssertionError("the round trip ran with the option off")

    bgr, dets = clip
    eng.gemm_stats(reset=True)
    plain = arun.run_inference(eng, bgr, _wav(), 25, detections=dets, mode=MODE_F16X3, flag_heatmaps=True)
    stats = eng.gemm_stats(reset=True)
    monkeypatch.setattr(eng, "jpeg_roundtrip_tiles", never)
    monkeypatch.setattr(eng, "jpeg_roundtrip_rgb", never)
    off = arun.run_inference(eng, bgr, _wav(), 25, detections=dets, mode=MODE_F16X3, flag_heatmaps=True, faces_via_jpeg=False)
    assert eng.gemm_stats(reset=True) == stats
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(off[k], plain[k], err_msg=k)
    np.testing.assert_array_equal(off["heatmaps"][1], plain["heatmaps"][1])


def test_refusals_come_before_any_work(eng, clip, sources, monkeypatch):
    from avcer_amd import run as arun
    from avcer_amd.dataset import VideoJob, run_dataset

    def never(*a, **k):
        raise AssertionError("work was done before the refusal")

    for name in ("track_faces", "jpeg_roundtrip_tiles", "jpeg_roundtrip_rgb", "jpeg_forward", "audio_forward", "static_forward", "crop_tiles"):
        monkeypatch.setattr(eng, name, never)
    bgr, dets = clip
    _, src, src_dev, rects = sources[0]
    for bad in ("yes", 1, None, "device"):
        with pytest.raises(ValueError, match="via_jpeg"):
            arun.run_inference(eng, bgr, _wav(), 25, detections=dets, faces_via_jpeg=bad)
        with pytest.raises(ValueError, match="via_jpeg"):
            face_tiles.VideoTiler(eng).process(bgr, dets, via_jpeg=bad)
        with pytest.raises(ValueError, match="via_jpeg"):
            run_dataset(eng, [VideoJob("v", 12, 96, 128, 25, 7680, detections=dets, load=never)], faces_via_jpeg=bad)
    for fn in (jpeg.roundtrip_tiles, jpeg.roundtrip_canvas):
        for kw in ({"quality": 0}, {"quality": 101}, {"subsampling": 3}, {"subsampling": -1}):
            with pytest.raises(ValueError):
                fn(eng, src_dev, rects, **kw)
        with pytest.raises(ValueError, match="image 1"):  # an empty crop keeps the encoder's error
            fn(eng, src_dev, [(0, 0, 0, 8, 8), (0, 5, 5, 5, 9)])
        with pytest.raises(ValueError, match="image 0"):
            fn(eng, src_dev, [(3, 0, 0, 8, 8)])
    assert tuple(jpeg.roundtrip_tiles(eng, src_dev, np.zeros((0, 5), dtype=np.int32)).shape) == (0, 224, 224, 3)
