"""detect_size=: the detector on a smaller copy of the frames (face_tiles.ScaledDetector) against the unwrapped detector fed
PIL-resized frames, through run_inference and run_inference_file, and the refusals -- all raised before any launch."""
import io

import numpy as np
import pytest
from PIL import Image

from avcer_amd import avi, synth
from avcer_amd import face_tiles as ft
from avcer_amd import run as arun
from avcer_amd.engine import MODE_F16X3, Engine

pytestmark = pytest.mark.gpu

KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")
X_COLS, Y_COLS = (0, 2, 5, 7, 9, 11, 13), (1, 3, 6, 8, 10, 12, 14)


@pytest.fixture(scope="module")
def sd_mnet():
    return synth.to_torch(synth.retina_mnet_state_dict(42))


@pytest.fixture(scope="module")
def eng(sd_mnet, sd_static, sd_dynamic, sd_audio):
    """An engine of this module's own (the session's keeps whatever detector other modules loaded), with every model loaded."""
    e = Engine(0)
    try:
        e.load_static(sd_static)
        e.load_dynamic(sd_dynamic)
        e.load_audio(sd_audio)
        yield e
    finally:
        e.close()


@pytest.fixture(scope="module")
def det(eng, sd_mnet):
    return ft.RetinaFacePredictor(eng, sd_mnet, threshold=0.9, mode=MODE_F16X3)


def pil_small(frames, h2, w2, f=Image.Resampling.BILINEAR):
    return np.stack([np.asarray(Image.fromarray(fr).resize((w2, h2), f)) for fr in frames])


def mapped(rows, h, w, h2, w2):
    rows = np.array(rows, dtype=np.float32)
    sx, sy = np.float32(w) / np.float32(w2), np.float32(h) / np.float32(h2)
    for c in range(rows.shape[1]):
        if c in X_COLS:
            rows[:, c] = rows[:, c] * sx
        elif c in Y_COLS:
            rows[:, c] = rows[:, c] * sy
    return rows


def assert_same(a, b, what=""):
    for key in KEYS:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key)
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what} {key}")


def test_wrapper_equals_the_detector_on_pil_resized_frames(eng, det):
    frames = synth.video_frames(21, 4, 192, 256)
    got = ft.ScaledDetector(det, (96, 128)).batch(frames, rgb=False)
    want = det.batch(pil_small(frames, 96, 128), rgb=False)
    assert sum(len(r) for r in want) > 0
    for g, r in zip(got, want):
        assert g.dtype == np.float32 and g.shape == r.shape
        np.testing.assert_array_equal(g, mapped(r, 192, 256, 96, 128))
    one = ft.ScaledDetector(det, 128, "lanczos")   # the int rule gives (96, 128) as well
    np.testing.assert_array_equal(one(frames[1], rgb=False),
                                  mapped(det(pil_small(frames[1:2], 96, 128, Image.Resampling.LANCZOS)[0], rgb=False), 192, 256, 96, 128))
    assert one.gflop_per_frame == pytest.approx(det.gflop_per_frame / 4) and one.kind != 1


def test_pass_through(eng, det):
    frames = synth.video_frames(22, 2, 192, 256)
    want = [r.copy() for r in det.batch(frames, rgb=False)]
    for size in ((192, 256), 4096):
        got = ft.ScaledDetector(det, size).batch(frames, rgb=False)
        for g, r in zip(got, want):
            np.testing.assert_array_equal(g, r)


def test_s3fd_rows(sd_static):
    """[k,5] rows: only the box is mapped.  The copy is 64 x 96, the smallest frame S3FD's own predictor tests use."""
    sd = synth.to_torch(synth.s3fd_state_dict(42))
    e = Engine(0)
    try:
        pred = ft.S3FDPredictor(e, sd, threshold=0.05, mode=MODE_F16X3)
        frames = synth.video_frames(3, 2, 128, 192)
        got = ft.ScaledDetector(pred, (64, 96)).batch(frames, rgb=False)
        want = pred.batch(pil_small(frames, 64, 96), rgb=False)
        for g, r in zip(got, want):
            assert g.shape == r.shape and g.shape[1] == 5
            np.testing.assert_array_equal(g, mapped(r, 128, 192, 64, 96))
    finally:
        e.close()


def test_run_inference(eng, det):
    frames = synth.video_frames(13, 12, 192, 256)
    wav = synth.waveforms(99, 1, int(12 / 25 * 16000))[0]
    dets = ft.ScaledDetector(det, (96, 128)).batch(frames, rgb=False)
    assert sum(len(d) for d in dets) > 0
    a = arun.run_inference(eng, frames, wav, 25, detector=det, mode=MODE_F16X3, detect_size=(96, 128))
    b = arun.run_inference(eng, frames, wav, 25, detections=dets, mode=MODE_F16X3)
    assert_same(a, b, "detect_size against its own detections")
    assert (a["records"][:, 2:] >= 0).all() and a["records"][:, 4].max() <= 255 and a["records"][:, 5].max() <= 191
    c = arun.run_inference(eng, frames, wav, 25, detector=det, mode=MODE_F16X3, detect_size=None)
    d = arun.run_inference(eng, frames, wav, 25, detector=det, mode=MODE_F16X3)
    assert_same(c, d, "detect_size=None against no keyword")


def test_run_inference_file_streamed(eng, det, tmp_path):
    frames = synth.video_frames(13, 12, 192, 256)
    blobs = []
    for fr in frames:
        buf = io.BytesIO()
        Image.fromarray(fr).save(buf, "JPEG", quality=92, subsampling=2)
        blobs.append(buf.getvalue())
    pcm = np.random.default_rng(5).integers(-20000, 20000, (int(12 / 25 * 44100), 2)).astype(np.int16)
    path = str(avi.write_avi(tmp_path / "clip.avi", blobs, 25, 1, pcm))
    ref = arun.run_inference_file(eng, path, detector=det, mode=MODE_F16X3, detect_size=(96, 128))
    got = arun.run_inference_file(eng, path, detector=det, mode=MODE_F16X3, detect_size=(96, 128), stream_frames=5)
    assert_same(got, ref, "stream_frames=5")


def test_refusals_come_before_any_launch(eng, det, tmp_path):
    """Every refusal is raised with the launch log still empty (the audio branch, the detector and the visual models all launch
    logged kernels, so an empty log means nothing ran).  run_inference_file refuses a bad value before the file is opened -- the path
    does not exist -- and an upscale once the container has named the frame size, before any decode."""
    frames = synth.video_frames(13, 2, 192, 256)
    wav = synth.waveforms(99, 1, 1280)[0]
    dets = [np.zeros((0, 15), np.float32)] * 2
    buf = io.BytesIO()
    Image.fromarray(frames[0]).save(buf, "JPEG", quality=92, subsampling=2)
    clip = str(avi.write_avi(tmp_path / "two.avi", [buf.getvalue()] * 2, 25, 1, np.zeros((3528, 2), np.int16)))
    cases = ((dict(detector=det, detect_size=(384, 512)), "upscaling"),
             (dict(detector=det, detect_size=(96, 512)), "upscaling"),
             (dict(detections=dets, detect_size=(96, 128)), "nothing would use it"),
             (dict(detector=det, detect_size="small"), "detect size"),
             (dict(detector=det, detect_size=1.5), "detect size"),
             (dict(detector=det, detect_size=True), "detect size"),
             (dict(detector=det, detect_size=(96, 128), detect_filter="hamming"), "lanczos"))
    eng.profile_enable(True)
    try:
        eng.profile_read_launches()
        for kw, match in cases:
            with pytest.raises(ValueError, match=match):
                arun.run_inference(eng, frames, wav, 25, mode=MODE_F16X3, **kw)
            for stream in (None, 1):
                with pytest.raises(ValueError, match=match):
                    arun.run_inference_file(eng, clip if match == "upscaling" else str(tmp_path / "never_opened.avi"), mode=MODE_F16X3,
                                            stream_frames=stream, **kw)
        assert eng.profile_read_launches() == []
    finally:
        eng.profile_enable(False)
