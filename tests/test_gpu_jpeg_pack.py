"""The entropy coder on the device (csrc/jpeg_pack.hip avcer_jpeg_pack, Engine.jpeg_pack, jpeg.encode_images(entropy="device")) against
its oracle, the host writer avcer_jpeg_write_batch (which tests/test_jpeg_encode_host.py holds to PIL's files): bytes, offsets and
statuses are equal for the crafted set and the images of tests/jpeg_pack_cases.py (tests/test_jpeg_pack_host.py shows what these
hold), and for the three callers that write files.  No case has a tolerance."""
import os

import numpy as np
import pytest
import torch

import jpeg_pack_cases as cases
from avcer_amd import face_tiles, heatmaps, jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crafted(engine):
    """(names, coefficients, DESC records, and the host writer's files, offsets, statuses and bytes needed).  Never written to."""
    names, coeffs, desc, want = cases.crafted(engine.lib)
    blobs, offsets, status, need = cases.host_write(engine.lib, coeffs, desc)
    np.testing.assert_array_equal(status, want)
    return names, coeffs, desc, blobs, offsets, status, need


def _pack(engine, coeffs, desc, cap=None):
    """Engine.jpeg_pack of host arrays: (files, offsets, statuses, bytes needed, the whole output buffer)."""
    n, blocks = len(desc), coeffs.size // 64
    c = torch.from_numpy(np.ascontiguousarray(coeffs.reshape(-1))).to(engine.device)
    d = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(engine.device)
    cap = 623 * n + 420 * blocks if cap is None else cap
    out, offsets, status, need = engine.jpeg_pack(c, d, n, blocks, cap)
    out, offsets, status = out.cpu().numpy(), offsets.cpu().numpy(), status.cpu().numpy()
    assert offsets[0] == 0 and (np.diff(offsets) >= 0).all() and offsets[-1] <= cap
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)], offsets, status, int(need.item()), out


def test_crafted_set_in_one_call_equals_the_host_writer(engine, crafted):
    names, coeffs, desc, blobs, offsets, status, need = crafted
    got, goff, gstatus, gneed, _ = _pack(engine, coeffs, desc)
    np.testing.assert_array_equal(gstatus, status)
    for n, a, b in zip(names, got, blobs):
        assert a == b, n
    np.testing.assert_array_equal(goff, offsets)
    assert gneed == need


def test_a_file_is_the_same_alone_and_in_reverse_order(engine, crafted):
    names, coeffs, desc, blobs, _, status, _ = crafted
    for i, n in enumerate(names):
        c, d = cases.subset(coeffs, desc, [i])
        got, _, gstatus, _, _ = _pack(engine, c, d)
        assert got == [blobs[i]] and gstatus[0] == status[i], n
    order = list(range(len(names)))[::-1]
    c, d = cases.subset(coeffs, desc, order)
    got, _, gstatus, _, _ = _pack(engine, c, d)
    assert got == blobs[::-1]
    np.testing.assert_array_equal(gstatus, status[::-1])
    # the same storage with the descriptors alone reversed: coef_block descends
    got, _, gstatus, _, _ = _pack(engine, coeffs, desc[::-1].copy())
    assert got == blobs[::-1]
    np.testing.assert_array_equal(gstatus, status[::-1])


@pytest.mark.parametrize("quality", [1, 95, 100])
@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_images_device_equals_host_equals_pil(engine, quality, subsampling):
    imgs = cases.image_groups()[(quality, subsampling)]
    src, rects = cases.canvas(imgs)
    want = [cases.pil_bytes(im, quality, subsampling) for im in imgs]
    kw = dict(quality=quality, subsampling=subsampling)
    assert jpeg.encode_images(engine, src, rects, entropy="host", **kw) == want
    assert jpeg.encode_images(engine, src, rects, entropy="device", **kw) == want
    for i in (0, 3, len(imgs) - 1):  # then one
        assert jpeg.encode_images(engine, src, rects[i:i + 1], entropy="device", **kw) == want[i:i + 1]


def test_bgr_source_with_an_odd_x0_in_slot_1(engine):
    rng = np.random.default_rng(31)
    src = rng.integers(0, 256, (2, 48, 64, 3)).astype(np.uint8)
    rects = [(1, 1, 0, 18, 33), (1, 5, 3, 57, 40), (1, 63, 47, 64, 48), (0, 7, 1, 47, 39)]
    want = [cases.pil_bytes(src[s, y0:y1, x0:x1, ::-1]) for s, x0, y0, x1, y1 in rects]
    assert jpeg.encode_images(engine, src, rects, bgr=True, entropy="device") == want
    assert jpeg.encode_images(engine, src, rects, bgr=True) == want


def test_one_byte_short_the_last_file_that_does_not_fit_has_no_bytes_and_encode_images_repeats(engine, crafted, monkeypatch):
    names, coeffs, desc, blobs, offsets, status, need = crafted
    cap = int(offsets[-1]) - 1
    hblobs, hoff, hstatus, hneed = cases.host_write(engine.lib, coeffs, desc, cap=cap)
    got, goff, gstatus, gneed, out = _pack(engine, coeffs, desc, cap=cap)
    np.testing.assert_array_equal(gstatus, hstatus)
    np.testing.assert_array_equal(goff, hoff)
    assert got == hblobs and gneed == hneed == need
    short = np.nonzero(gstatus == cases.R_NO_SPACE)[0]
    last = max(i for i in range(len(names)) if status[i] == 0)
    assert short.tolist() == [last] and got[:last] == blobs[:last] and got[last] == b""
    # encode_images: noise at quality 100 takes far more than the 40 bytes a block of the first guess
    calls = []
    pack = engine.jpeg_pack
    monkeypatch.setattr(engine, "jpeg_pack", lambda *a: calls.append(a[-1]) or pack(*a))
    imgs = cases.image_groups()[(100, 0)]
    src, rects = cases.canvas(imgs)
    want = [cases.pil_bytes(im, 100, 0) for im in imgs]
    assert jpeg.encode_images(engine, src, rects, quality=100, subsampling=0, entropy="device") == want
    assert len(calls) == 2 and calls[0] < sum(len(b) for b in want) == calls[1]


@pytest.fixture(scope="module")
def video():
    """A scripted video: 12 BGR frames of 96 x 128 and per-frame detections of 2 tracks (the second appears in frame 3)."""
    rng = np.random.default_rng(41)
    yy, xx = np.mgrid[0:96, 0:128]
    bgr = np.stack([np.stack([np.sin(xx / (9.0 + c + t)) * 60 + np.cos(yy / (11.0 - c)) * 50 + 128 for c in range(3)], axis=2) for t in range(12)])
    bgr = np.clip(np.rint(bgr + rng.normal(0, 5, bgr.shape)), 0, 255).astype(np.uint8)
    dets = []
    for t in range(12):
        d = [[10.4 + 2 * t, 8.2 + t, 51.7 + 2 * t, 60.3 + t, 0.99]]
        if t >= 3:
            d.append([70.0 + t, 30.5, 111.0 + t, 85.9 - t, 0.95])
        dets.append(np.array(d, dtype=np.float32))
    return bgr, dets


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_face_folders_are_the_same_file_for_file(engine, video, tmp_path):
    bgr, dets = video
    records, tiles = face_tiles.VideoTiler(engine).process(bgr, dets, save_path=str(tmp_path / "host"), video_name="clip")
    drecords, dtiles = face_tiles.VideoTiler(engine).process(bgr, dets, save_path=str(tmp_path / "dev"), video_name="clip", entropy="device")
    np.testing.assert_array_equal(records, drecords)
    np.testing.assert_array_equal(tiles.cpu().numpy(), dtiles.cpu().numpy())
    a, b = _tree(tmp_path / "host"), _tree(tmp_path / "dev")
    assert len(a) == len(records) == 21 and sorted({os.path.dirname(k) for k in a}) == ["clip/00", "clip/01"]
    assert a == b
    paths = face_tiles.write_face_crops(engine, torch.from_numpy(bgr).to(engine.device), records, str(tmp_path / "again"), "clip", entropy="device")
    assert _tree(tmp_path / "again") == a and len(paths) == 21
    with pytest.raises(ValueError, match="entropy"):
        face_tiles.write_face_crops(engine, torch.from_numpy(bgr).to(engine.device), records, str(tmp_path / "no"), "clip", entropy="gpu")


def test_heat_maps_are_the_same_file_for_file(engine, tmp_path):
    rng = np.random.default_rng(43)
    yy, xx = np.mgrid[0:224, 0:224]
    imgs = np.stack([np.stack([np.sin(xx / (19.0 + c + t)) * 70 + np.cos(yy / (23.0 - c)) * 50 + 128 for c in range(3)], axis=2) for t in range(4)])
    imgs = torch.from_numpy(np.clip(np.rint(imgs + rng.normal(0, 4, imgs.shape)), 0, 255).astype(np.uint8)).to(engine.device)
    idx = [0, 5, 10, 40]
    a = heatmaps.write_heatmaps(str(tmp_path / "host"), idx, imgs, engine=engine)
    b = heatmaps.write_heatmaps(str(tmp_path / "dev"), idx, imgs, engine=engine, entropy="device")
    assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b] == [f"{i:06d}.jpg" for i in idx]
    assert _tree(tmp_path / "host") == _tree(tmp_path / "dev")
    assert open(b[0], "rb").read() == cases.pil_bytes(imgs[0].cpu().numpy()[..., ::-1])


def test_run_inference_with_the_device_coder_returns_the_same_tables_and_writes_the_same_files(engine, video, sd_static, sd_dynamic, sd_audio, tmp_path):
    from avcer_amd import run as arun
    from avcer_amd import synth
    from avcer_amd.engine import MODE_F16X3

    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    bgr, dets = video
    wav = synth.waveforms(99, 1, int(12 / 25 * 16000))[0]
    with pytest.raises(ValueError, match="jpeg_entropy"):
        arun.run_inference(engine, bgr, wav, 25, detections=dets, mode=MODE_F16X3, jpeg_entropy="bogus")
    plain = arun.run_inference(engine, bgr, wav, 25, detections=dets, mode=MODE_F16X3)
    host = arun.run_inference(engine, bgr, wav, 25, detections=dets, mode=MODE_F16X3, name_video="clip", path_save_faces=str(tmp_path / "host"),
                              jpeg_entropy="host")
    dev = arun.run_inference(engine, bgr, wav, 25, detections=dets, mode=MODE_F16X3, name_video="clip", path_save_faces=str(tmp_path / "dev"),
                             jpeg_entropy="device")
    assert len(dev["face_files"]) == 21 and _tree(tmp_path / "dev") == _tree(tmp_path / "host")
    for k in ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "records"):
        np.testing.assert_array_equal(dev[k], plain[k], err_msg=k)
        np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
