"""Long and lossless recordings through run.run_inference_file: uncompressed BGR AVI files (24-bit bottom-up, 32-bit top-down in OpenDML
segments) give, bit for bit, run_inference on the frames themselves, in memory and streamed; a Motion-JPEG OpenDML file gives what the
plain file gives; the result video written in OpenDML segments holds the plain result video's frames and sound.  12 frames of 64 x 48,
the smallest size whole recordings run at (tests/test_gpu_avi.py), supplied detections, synthetic models."""
import numpy as np
import pytest

from avcer_amd import avi
from avcer_amd import run as arun
from avcer_amd.dataset import run_dataset, video_job_from_avi
from avcer_amd.engine import MODE_F16X3
from test_avi_cpu import jpeg_file, pcm_of, picture

pytestmark = pytest.mark.gpu

W, H, N, RATE = 64, 48, 12, 25
KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


@pytest.fixture(scope="module")
def clip():
    """The frames (BGR), the sound, the detections -- and the reference: run_inference on the frames themselves, computed once."""
    frames = np.stack([picture(W, H, 300 + i)[..., ::-1] for i in range(N)])
    pcm = pcm_of(44100, 2, seed=8)
    dets = [np.array([[W // 8 + (t % 3), H // 8, W - W // 8 + (t % 3), H - H // 8] + [0.99] + [0] * 10], dtype=np.float32) for t in range(N)]
    return np.ascontiguousarray(frames), pcm, dets


@pytest.fixture(scope="module")
def reference(engine_all, clip):
    frames, pcm, dets = clip
    return arun.run_inference(engine_all, frames, pcm, RATE, detections=dets, mode=MODE_F16X3, wav_sr=44100)


def assert_same(got, ref, what=""):
    for key in KEYS:
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (what, key)
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")


@pytest.mark.parametrize("bits,bottom_up,opendml", [(24, True, False), (32, False, True)])
def test_raw_files_give_run_inference_on_the_frames(engine_all, clip, reference, tmp_path, bits, bottom_up, opendml):
    frames, pcm, dets = clip
    kw = dict(opendml=True, segment_bytes=6 * 64 * 48 * 4, index_segments=8) if opendml else {}
    path = avi.write_avi_raw(tmp_path / "raw.avi", frames, RATE, pcm=pcm, bits=bits, bottom_up=bottom_up, **kw)
    if opendml:
        assert (tmp_path / "raw.avi").read_bytes().count(b"AVIX") >= 2                     # three segments or more
        with pytest.raises(ValueError, match="AVIX"):
            arun.run_inference_file(engine_all, path, detections=dets, opendml=False)
    got = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3)
    assert_same(got, reference, "in memory")
    assert got["real_time_factor"] > 0
    got = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, stream_frames=5, frames_per_pass=2)
    assert_same(got, reference, "stream_frames=5")
    job = video_job_from_avi(path, detections=dets, engine=engine_all)
    assert (job.n_frames, job.height, job.width, job.fps, job.n_samples, job.wav_sr) == (N, H, W, RATE, 44100, 44100)
    assert_same(run_dataset(engine_all, [job], mode=MODE_F16X3)[0], reference, "run_dataset")


def test_a_motion_jpeg_opendml_file_gives_what_the_plain_file_gives(engine_all, clip, tmp_path):
    _, pcm, dets = clip
    blobs = [jpeg_file(W, H, 300 + i, 2, quality=92) for i in range(N)]
    plain = avi.write_avi(tmp_path / "plain.avi", blobs, RATE, pcm=pcm)
    odml = avi.write_avi(tmp_path / "odml.avi", blobs, RATE, pcm=pcm, opendml=True, segment_bytes=40000, index_segments=16)
    assert (tmp_path / "odml.avi").read_bytes().count(b"AVIX") >= 2
    ref = arun.run_inference_file(engine_all, plain, detections=dets, mode=MODE_F16X3)
    assert_same(arun.run_inference_file(engine_all, odml, detections=dets, mode=MODE_F16X3), ref, "in memory")
    assert_same(arun.run_inference_file(engine_all, odml, detections=dets, mode=MODE_F16X3, stream_frames=5), ref, "stream_frames=5")


def test_the_result_video_in_opendml_segments(engine_all, clip, tmp_path):
    frames, pcm, dets = clip
    path = avi.write_avi_raw(tmp_path / "raw.avi", frames, RATE, pcm=pcm)
    kw = dict(detections=dets, mode=MODE_F16X3, video_panel=True)
    ref = arun.run_inference_file(engine_all, path, path_save_video=str(tmp_path / "plain_out.avi"), **kw)
    got = arun.run_inference_file(engine_all, path, path_save_video=str(tmp_path / "odml_out.avi"), video_opendml=True,
                                  video_segment_bytes=30000, stream_frames=5, **kw)
    assert_same(got, ref)
    assert got["result_video"] == str(tmp_path / "odml_out.avi")
    assert (tmp_path / "odml_out.avi").read_bytes().count(b"AVIX") >= 2
    with pytest.raises(ValueError, match="indx|AVIX"):
        avi.open_avi(tmp_path / "odml_out.avi")
    with avi.open_avi(tmp_path / "odml_out.avi", opendml=True) as a, avi.open_avi(tmp_path / "plain_out.avi") as b:
        assert (a.n_frames, a.width, a.height, a.rate, a.scale) == (b.n_frames, b.width, b.height, b.rate, b.scale) == (N, W, H, RATE, 1)
        assert [bytes(f) for f in a.frames] == [bytes(f) for f in b.frames]
        np.testing.assert_array_equal(a.pcm, b.pcm)
        np.testing.assert_array_equal(a.pcm, pcm)
