"""Motion-JPEG recordings on the GPU: avcer_jpeg_frames against PIL (tolerance zero, guard bands around the batch),
jpeg.decode_frames across its options, run.run_inference_file against run_inference on PIL-decoded frames, and
dataset.video_job_from_avi through run_dataset.  Sizes are the smallest at which the frame kernel can go wrong: partial MCUs on both
edges, rows of 3 W bytes that are no multiple of 16 or of 4, an exact-MCU size, one wider than a workgroup's 256 pieces of a
row... and a picture of at most two chroma columns, which libjpeg replicates instead of filtering."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import guard_band as gb
from avcer_amd import avi, jpeg
from avcer_amd import run as arun
from avcer_amd.dataset import run_dataset, video_job_from_avi
from avcer_amd.engine import MODE_F16X3
from test_avi_cpu import KINDS, cut_dht, jpeg_file, pcm_of

pytestmark = pytest.mark.gpu

SIZES = ((50, 38), (33, 17), (16, 16), (64, 48), (130, 70), (4, 3))   # (w, h)


def pil_rgb(blob):
    return np.array(Image.open(io.BytesIO(bytes(blob))).convert("RGB"))


def pil_frames(blobs, bgr=True):
    x = np.stack([pil_rgb(b) for b in blobs])
    return np.ascontiguousarray(x[..., ::-1]) if bgr else x


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


# ---------------------------------------------------------------------------------------------------- avcer_jpeg_frames
@pytest.mark.parametrize("w,h", SIZES)
def test_frames_kernel_equals_pil_inside_guard_bands(engine, w, h):
    for k, (kind, sub) in enumerate(KINDS):
        blobs = [jpeg_file(w, h, 1000 * w + 10 * k + i, sub) for i in range(5)]
        want = np.stack([pil_rgb(b) for b in blobs])
        for n in (1, 5):
            c_dev, d_dev, used, desc = jpeg._to_device(engine, blobs[:n], 2)
            assert (desc["status"] == jpeg.OK).all()
            for bgr in (False, True):
                flags = []

                def run(outs):
                    flags.append(engine.jpeg_frames(c_dev, d_dev, n, used, h, w, bgr=bgr, out=outs[0])[1])

                got, = gb.check(run, [gb.Band("frames", (n, h, w, 3), torch.uint8, row_bytes=3 * w)], inputs=(c_dev, d_dev),
                                device=engine.device)
                assert all(int(f.abs().sum()) == 0 for f in flags), (kind, n, bgr)
                ref = want[:n, :, :, ::-1] if bgr else want[:n]
                np.testing.assert_array_equal(got.numpy(), ref, err_msg=f"{kind} {w}x{h} n={n} bgr={bgr}")


def test_frames_kernel_at_every_alignment_of_the_batch(engine):
    """The batch may start at any byte: the aligned pieces then fall elsewhere in every row."""
    w, h, n = 33, 17, 3
    blobs = [jpeg_file(w, h, 50 + i, 2) for i in range(n)]
    want = pil_frames(blobs)
    c_dev, d_dev, used, _ = jpeg._to_device(engine, blobs, 2)
    size = n * h * w * 3
    for off in range(16):
        buf = torch.full((256 + size + 256,), 0xA5, dtype=torch.uint8, device=engine.device)
        out = buf[64 + off:64 + off + size].view(n, h, w, 3)
        engine.jpeg_frames(c_dev, d_dev, n, used, h, w, bgr=True, out=out)
        host = buf.cpu().numpy()
        assert (host[:64 + off] == 0xA5).all() and (host[64 + off + size:] == 0xA5).all(), off
        np.testing.assert_array_equal(host[64 + off:64 + off + size].reshape(n, h, w, 3), want, err_msg=str(off))


def test_a_file_of_another_size_is_flagged_and_zero(engine):
    w, h = 50, 38
    blobs = [jpeg_file(w, h, 70 + i, (2, 1, 0, None, 2)[i]) for i in range(5)]
    blobs[2] = jpeg_file(33, 17, 9, 2)
    c_dev, d_dev, used, desc = jpeg._to_device(engine, blobs, 2)
    assert (desc["status"] == jpeg.OK).all()
    flags = []

    def run(outs):
        flags.append(engine.jpeg_frames(c_dev, d_dev, 5, used, h, w, bgr=True, out=outs[0])[1])

    got, = gb.check(run, [gb.Band("frames", (5, h, w, 3), torch.uint8, row_bytes=3 * w)], inputs=(c_dev, d_dev), device=engine.device)
    assert flags[0].cpu().tolist() == [0, 0, 2, 0, 0]
    got = got.numpy()
    assert not got[2].any()
    for i in (0, 1, 3, 4):
        np.testing.assert_array_equal(got[i], pil_rgb(blobs[i])[..., ::-1], err_msg=str(i))
    with pytest.raises(ValueError):
        engine.jpeg_frames(c_dev, d_dev, 5, used, h, w, out=torch.empty(5, h, w + 1, 3, dtype=torch.uint8, device=engine.device))


# ---------------------------------------------------------------------------------------------------- decode_frames
@pytest.fixture(scope="module")
def clip():
    """Nine frames of 50 x 38 as a video may hold them: every sampling, DHT-less twins of two of them, one progressive frame."""
    w, h = 50, 38
    blobs = [jpeg_file(w, h, 300 + i, sub) for i, (_, sub) in enumerate(KINDS)]
    blobs += [cut_dht(blobs[0]), cut_dht(blobs[3]), jpeg_file(w, h, 310, 2, progressive=True), jpeg_file(w, h, 311, 2, optimize=True),
              jpeg_file(w, h, 312, 1)]
    return w, h, blobs, pil_frames(blobs)


def test_decode_frames_does_not_depend_on_its_options(engine, clip):
    w, h, blobs, want = clip
    for entropy in ("host", "device"):
        for per in (2, 64):
            for threads in (1, 16):
                frames, paths = jpeg.decode_frames(engine, blobs, h, w, entropy=entropy, threads=threads, frames_per_pass=per)
                assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (9, h, w, 3)
                assert paths == ["device"] * 6 + ["pil"] + ["device"] * 2, (entropy, per, threads, paths)
                np.testing.assert_array_equal(frames.cpu().numpy(), want, err_msg=f"{entropy} {per} {threads}")
    # DHT-less frames match their DHT-carrying twins (and so PIL's decode of the twin)
    np.testing.assert_array_equal(want[4], want[0])
    np.testing.assert_array_equal(want[5], want[3])
    rgb, _ = jpeg.decode_frames(engine, [memoryview(b) for b in blobs], h, w, bgr=False)
    np.testing.assert_array_equal(rgb.cpu().numpy(), want[..., ::-1])
    # without the default tables such a frame is the header pass's refusal, and PIL's to read
    _, paths = jpeg.decode_frames(engine, blobs, h, w, std_tables=False)
    assert paths[4] == paths[5] == "pil" and paths[0] == "device"
    empty, paths = jpeg.decode_frames(engine, [], h, w)
    assert tuple(empty.shape) == (0, h, w, 3) and paths == []


def test_decode_frames_names_the_frame_it_cannot_read(engine, clip):
    w, h, blobs, _ = clip
    bad = list(blobs)
    bad[3] = b"RIFF not a jpeg at all" * 4
    for entropy in ("host", "device"):
        with pytest.raises(OSError, match="frame 3"):
            jpeg.decode_frames(engine, bad, h, w, entropy=entropy, frames_per_pass=2)
    other = list(blobs)
    other[7] = jpeg_file(33, 17, 1, 2)
    with pytest.raises(OSError, match="frame 7.*33 x 17"):
        jpeg.decode_frames(engine, other, h, w)
    with pytest.raises(ValueError, match="entropy"):
        jpeg.decode_frames(engine, blobs, h, w, entropy="bogus")
    frames, _ = jpeg.decode_frames(engine, blobs, h, w)                 # and the engine decodes on after the failures
    assert frames.shape[0] == 9


# ---------------------------------------------------------------------------------------------------- whole recordings
KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")


def recording(tmp_path, name, w, h, n, rate, scale, pcm, seed):
    blobs = [jpeg_file(w, h, seed + i, 2, quality=92) for i in range(n)]
    blobs[1] = cut_dht(blobs[1])
    path = avi.write_avi(tmp_path / f"{name}.avi", blobs, rate, scale, pcm)
    dets = [np.array([[w // 8 + (t % 3), h // 8, w - w // 8 + (t % 3), h - h // 8] + [0.99] + [0] * 10], dtype=np.float32) for t in range(n)]
    return str(path), blobs, dets


def assert_same(got, ref):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


def test_run_inference_file_equals_run_inference_on_pil_frames(engine_all, tmp_path):
    pcm = pcm_of(44100, 2, seed=5)
    path, blobs, dets = recording(tmp_path, "talk", 64, 48, 12, 30000, 1001, pcm, 400)
    frames = pil_frames(blobs)
    got = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3)
    ref = arun.run_inference(engine_all, frames, pcm, 29, detections=dets, mode=MODE_F16X3, wav_sr=44100, name_video="talk")
    assert_same(got, ref)                                               # fps defaults to int(rate / scale) = 29
    assert got["real_time_factor"] > 0
    got = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, fps=25, frames_per_pass=5)
    assert_same(got, arun.run_inference(engine_all, frames, pcm, 25, detections=dets, mode=MODE_F16X3, wav_sr=44100))
    mute = str(avi.write_avi(tmp_path / "mute.avi", blobs, 25))
    with pytest.raises(ValueError, match="no audio stream"):
        arun.run_inference_file(engine_all, mute, detections=dets)
    got = arun.run_inference_file(engine_all, mute, detections=dets, mode=MODE_F16X3, wav=pcm, wav_sr=44100)
    assert_same(got, arun.run_inference(engine_all, frames, pcm, 25, detections=dets, mode=MODE_F16X3, wav_sr=44100))
    odd = str(avi.write_avi(tmp_path / "odd.avi", blobs, 25, pcm=pcm, audio_rate=12345))
    with pytest.raises(ValueError, match="12345"):
        arun.run_inference_file(engine_all, odd, detections=dets)
    with pytest.raises(ValueError, match="detector"):
        arun.run_inference_file(engine_all, path)


def test_video_jobs_from_avi_files_through_run_dataset(engine_all, tmp_path):
    a = recording(tmp_path, "a", 64, 48, 12, 25, 1, pcm_of(44100, 2, seed=6), 500)
    b = recording(tmp_path, "b", 50, 38, 9, 30000, 1001, pcm_of(24000, 1, seed=7).reshape(-1, 1), 600)
    # (without `engine`, load() decodes on the youngest engine alive for the device)
    jobs = [video_job_from_avi(a[0], detections=a[2]), video_job_from_avi(b[0], detections=b[2], engine=engine_all)]
    assert [(j.name, j.n_frames, j.height, j.width, j.fps, j.n_samples, j.wav_sr) for j in jobs] == \
        [("a", 12, 48, 64, 25, 44100, 44100), ("b", 9, 38, 50, 29, 24000, 44100)]
    res = run_dataset(engine_all, jobs, mode=MODE_F16X3)
    for got, (p, _, d) in zip(res, (a, b)):
        assert_same(got, arun.run_inference_file(engine_all, p, detections=d, mode=MODE_F16X3))
    with pytest.raises(ValueError, match="no audio stream"):
        video_job_from_avi(avi.write_avi(tmp_path / "mute.avi", a[1], 25))
