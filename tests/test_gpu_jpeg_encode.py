"""The JPEG encoder on the device (csrc/jpeg_encode.hip avcer_jpeg_forward, avcer_amd/jpeg.py encode_images) and what is built on it
(face_tiles.write_face_crops, heatmaps.write_heatmaps with an engine).  The kernel is held to its numpy statement
(jpeg.forward_numpy, which tests/test_jpeg_encode_host.py holds to PIL's files) coefficient for coefficient, the files to the bytes
PIL writes: tests/golden/jpeg_encode.npz for the fixtures, PIL's encoder on this machine elsewhere.  No case has a tolerance."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from avcer_amd import face_tiles, heatmaps, jpeg, video_pipeline

pytestmark = pytest.mark.gpu


def _pil(rgb, quality=95, subsampling=2):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(b, "JPEG", quality=int(quality), subsampling=int(subsampling))
    return b.getvalue()


@pytest.fixture(scope="module")
def fixtures(golden):
    g = golden("jpeg_encode")
    return [(str(n), g[f"rgb_{i}"], int(g["quality"][i]), int(g["subsampling"][i]), g[f"jpg_{i}"].tobytes()) for i, n in enumerate(g["names"])]


@pytest.fixture(scope="module")
def frames():
    """u8 [2,48,64,3]: smooth waves plus noise, two different slots.  Never written to."""
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:48, 0:64]
    a = np.stack([np.stack([np.sin(xx / (5.0 + 2 * c + t) + c) * 70 + np.cos(yy / (7.0 - c)) * 50 + 128 for c in range(3)], axis=2)
                  for t in range(2)])
    a = np.clip(np.rint(a + rng.normal(0, 6, a.shape)), 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


def _kernel(engine, src, rects, quality, subsampling, bgr=False):
    """plan on the host, descriptors and rectangles to the device, ONE launch: (coefficients int16 [blocks, 64], DESC records)."""
    rects = np.asarray(rects, dtype=np.int32).reshape(-1, 5)
    desc, blocks = jpeg.plan(engine.lib, [(r[3] - r[1], r[4] - r[2]) for r in rects], quality, subsampling)
    assert (desc["status"] == jpeg.OK).all()
    d_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(engine.device)
    out = engine.jpeg_forward(torch.from_numpy(np.array(src)).to(engine.device), torch.from_numpy(rects).to(engine.device),
                              d_dev, len(rects), blocks, bgr=bgr)
    return out.cpu().numpy().reshape(-1, 64), desc


def _check(engine, src, rects, quality, subsampling, bgr=False):
    """Kernel coefficients == forward_numpy of the crops; encode_images bytes == PIL's bytes for the crops."""
    crops = [src[s, y0:y1, x0:x1, ::-1] if bgr else src[s, y0:y1, x0:x1] for s, x0, y0, x1, y1 in rects]
    got, desc = _kernel(engine, src, rects, quality, subsampling, bgr)
    want, wd = jpeg.forward_numpy(crops, quality, subsampling)
    assert desc.tobytes() == wd.tobytes()
    for i, d in enumerate(desc):
        a, b = int(d["coef_block"]), int(d["coef_block"] + d["n_blocks"])
        np.testing.assert_array_equal(got[a:b], want[a:b], err_msg=f"image {i}: {rects[i]} q{quality} s{subsampling}")
    blobs = jpeg.encode_images(engine, torch.from_numpy(np.array(src)), rects, bgr=bgr, quality=quality, subsampling=subsampling)
    for i, crop in enumerate(crops):
        assert blobs[i] == _pil(crop, quality, subsampling), f"image {i}: {rects[i]} q{quality} s{subsampling}"
    return blobs


def test_fixtures_kernel_equals_numpy_and_files_equal_the_committed_bytes(engine, fixtures):
    for name, rgb, q, s, blob in fixtures:
        h, w = rgb.shape[:2]
        got, desc = _kernel(engine, rgb[None], [(0, 0, 0, w, h)], q, s)
        want, _ = jpeg.forward_numpy([rgb], q, s)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert jpeg.encode_images(engine, rgb[None], [(0, 0, 0, w, h)], quality=q, subsampling=s) == [blob], name


@pytest.mark.parametrize("subsampling", [2, 1])
def test_widths_around_one_and_two_mcus(engine, frames, subsampling):
    """Right-edge replication, and an odd count of luma blocks in a row: a dummy block."""
    _check(engine, frames, [(0, 3, 2, 3 + w, 2 + 24) for w in (15, 16, 17, 31, 32, 33)], 95, subsampling)


def test_heights_even_and_no_multiple_of_16_odd_and_whole(engine, frames):
    """The bottom edge under 4:2:0: the last DOWNSAMPLED chroma row is repeated, not the last input row (38 and 40); an odd
    height completes its row group first (37); 48 has no edge."""
    _check(engine, frames, [(0, 4, 48 - h, 4 + 40, 48) for h in (38, 40, 37, 48)], 95, 2)


@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_one_pixel_feeds_a_whole_mcu(engine, frames, subsampling):
    _check(engine, frames, [(1, 9, 7, 10, 8), (1, 9, 7, 10, 24), (1, 9, 7, 26, 8)], 75, subsampling)


def test_odd_x0_in_slot_1_of_a_bgr_tensor(engine, frames):
    """Rows that start at odd byte offsets, slot indexing, the channel order."""
    rects = [(1, 1, 0, 18, 33), (1, 5, 3, 57, 40), (1, 63, 47, 64, 48), (0, 7, 1, 47, 39)]
    for s in (0, 2):
        _check(engine, frames, rects, 95, s, bgr=True)


@pytest.mark.parametrize("subsampling", [0, 2])
def test_nine_unequal_images_in_one_launch_then_one(engine, frames, subsampling):
    """3 to 72 blocks an image: a wave's 8 blocks span images, the search for a block's image is exercised at both ends."""
    sizes = [(1, 1), (40, 38), (8, 8), (17, 33), (9, 5), (64, 24), (16, 16), (3, 40), (33, 17)]
    rects = [(i % 2, 0, 0, w, h) for i, (w, h) in enumerate(sizes)]
    _check(engine, frames, rects, 95, subsampling)
    _check(engine, frames, rects[1:2], 95, subsampling)
    _check(engine, frames, rects[:1], 95, subsampling)


@pytest.mark.parametrize("quality", [100, 1])
def test_bilevel_content_at_both_ends_of_the_quality_scale(engine, quality):
    """The largest coefficients there are, divided by 8 (q = 1) and by 8 * 255."""
    rng = np.random.default_rng(37)
    src = (rng.integers(0, 2, (1, 40, 40, 3)) * 255).astype(np.uint8)
    for s in (0, 1, 2):
        _check(engine, src, [(0, 0, 0, 40, 40), (0, 1, 2, 18, 35)], quality, s)


def test_empty_and_outside_rectangles_raise_before_anything_is_encoded(engine, frames):
    with pytest.raises(ValueError, match="image 1"):
        jpeg.encode_images(engine, frames, [(0, 0, 0, 8, 8), (0, 5, 5, 5, 9)])
    with pytest.raises(ValueError, match="image 0"):
        jpeg.encode_images(engine, frames, [(0, 60, 0, 65, 8)])
    with pytest.raises(ValueError, match="image 0"):
        jpeg.encode_images(engine, frames, [(2, 0, 0, 8, 8)])
    assert jpeg.encode_images(engine, frames, np.zeros((0, 5), dtype=np.int32)) == []


@pytest.fixture(scope="module")
def video():
    """A scripted video: 6 BGR frames of 96 x 128 and per-frame detections of 2 tracks (the second appears in frame 2)."""
    rng = np.random.default_rng(41)
    yy, xx = np.mgrid[0:96, 0:128]
    bgr = np.stack([np.stack([np.sin(xx / (9.0 + c + t)) * 60 + np.cos(yy / (11.0 - c)) * 50 + 128 for c in range(3)], axis=2) for t in range(6)])
    bgr = np.clip(np.rint(bgr + rng.normal(0, 5, bgr.shape)), 0, 255).astype(np.uint8)
    dets = []
    for t in range(6):
        d = [[10.4 + 2 * t, 8.2 + t, 51.7 + 2 * t, 60.3 + t, 0.99]]
        if t >= 2:
            d.append([70.0 + t, 30.5, 111.0 + t, 85.9 - t, 0.95])
        dets.append(np.array(d, dtype=np.float32))
    return bgr, dets


def test_face_folders_of_a_scripted_video_are_pils_files_and_read_back_as_pils_tiles(engine, video, tmp_path):
    """The reference's folder layout, every file byte-identical to the PIL write of its crop, and read_face_dir_device of a folder
    equal to the PIL read of PIL-written files."""
    bgr, dets = video
    tiler = face_tiles.VideoTiler(engine)
    records, tiles = tiler.process(bgr, dets, save_path=str(tmp_path / "faces"), video_name="clip")
    assert len(records) == 10 and sorted(set(records[:, 1].tolist())) == [0, 1]
    plain_records, plain_tiles = face_tiles.VideoTiler(engine).process(bgr, dets)
    np.testing.assert_array_equal(records, plain_records)
    np.testing.assert_array_equal(tiles.cpu().numpy(), plain_tiles.cpu().numpy())
    root = tmp_path / "faces" / "clip"
    assert sorted(os.listdir(root)) == ["00", "01"]
    assert sorted(os.listdir(root / "00")) == [f"{t:06d}.jpg" for t in range(6)]
    assert sorted(os.listdir(root / "01")) == [f"{t:06d}.jpg" for t in range(2, 6)]
    pil_root = tmp_path / "pil" / "clip"
    for f, t, x0, y0, x1, y1 in records:
        want = _pil(bgr[f, y0:y1, x0:x1, ::-1])
        assert (root / f"{t:02d}" / f"{f:06d}.jpg").read_bytes() == want, (f, t)
        os.makedirs(pil_root / f"{t:02d}", exist_ok=True)
        (pil_root / f"{t:02d}" / f"{f:06d}.jpg").write_bytes(want)
    paths = face_tiles.write_face_crops(engine, torch.from_numpy(bgr).to(engine.device), records, str(tmp_path / "again"), "clip")
    assert paths == face_tiles.face_crop_paths(records, str(tmp_path / "again"), "clip")
    assert [open(p, "rb").read() for p in paths] == [(root / f"{t:02d}" / f"{f:06d}.jpg").read_bytes() for f, t in records[:, :2]]
    for track in ("00", "01"):
        got, present = video_pipeline.read_face_dir_device(engine, str(root), 6, track=track)
        want, wpresent = video_pipeline.read_face_dir(str(pil_root), 6, track=track)
        assert present.tolist() == wpresent.tolist()
        np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_heat_maps_written_through_the_engine_are_the_files_pil_writes(engine, tmp_path):
    rng = np.random.default_rng(43)
    yy, xx = np.mgrid[0:224, 0:224]
    imgs = np.stack([np.stack([np.sin(xx / (19.0 + c + t)) * 70 + np.cos(yy / (23.0 - c)) * 50 + 128 for c in range(3)], axis=2) for t in range(5)])
    imgs = np.clip(np.rint(imgs + rng.normal(0, 4, imgs.shape)), 0, 255).astype(np.uint8)
    idx = [0, 5, 10, 15, 40]
    a = heatmaps.write_heatmaps(str(tmp_path / "pil"), idx, imgs)
    b = heatmaps.write_heatmaps(str(tmp_path / "dev"), idx, torch.from_numpy(imgs).to(engine.device), engine=engine)
    assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b] == [f"{i:06d}.jpg" for i in idx]
    for p, q in zip(a, b):
        assert open(p, "rb").read() == open(q, "rb").read(), p
    # a host array with an engine, and a device tensor without one, take the PIL loop
    c = heatmaps.write_heatmaps(str(tmp_path / "host"), idx, imgs, engine=engine)
    d = heatmaps.write_heatmaps(str(tmp_path / "none"), idx, torch.from_numpy(imgs).to(engine.device))
    for p, q, r in zip(a, c, d):
        assert open(p, "rb").read() == open(q, "rb").read() == open(r, "rb").read()


def test_run_inference_writes_the_face_folders_when_asked_and_changes_nothing_else(engine, video, sd_static, sd_dynamic, sd_audio, tmp_path):
    from avcer_amd import run as arun
    from avcer_amd import synth
    from avcer_amd.engine import MODE_F16X3

    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    bgr, dets = video
    wav = synth.waveforms(99, 1, int(6 / 25 * 16000))[0]
    plain = arun.run_inference(engine, bgr, wav, 25, detections=dets, mode=MODE_F16X3)
    out = arun.run_inference(engine, bgr, wav, 25, detections=dets, mode=MODE_F16X3, name_video="clip", path_save_faces=str(tmp_path))
    assert "face_files" not in plain and sorted(os.listdir(tmp_path / "clip")) == ["00", "01"]
    assert out["face_files"] == face_tiles.face_crop_paths(out["records"], str(tmp_path), "clip") and len(out["face_files"]) == 10
    for p, (f, t, x0, y0, x1, y1) in zip(out["face_files"], out["records"]):
        assert open(p, "rb").read() == _pil(bgr[f, y0:y1, x0:x1, ::-1]), p
    for k in ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "records"):
        np.testing.assert_array_equal(out[k], plain[k], err_msg=k)
