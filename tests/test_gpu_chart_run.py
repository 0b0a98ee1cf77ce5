"""`flag_save_plot_pred` on run.run_inference / run.run_inference_file / dataset.run_dataset: the prediction timeline chart written
behind the fusion, from the class tables on the device.

The claim for every file: its bytes are PIL's Image.save(quality=95, subsampling=2) of chart.chart_numpy of the call's own av / vs /
vd / a tables; and the option changes nothing else -- the tables and every other file are those of the call without it.

The clip: 40 frames of 64 x 48 (the smallest frames the run tests use) with 1.6 s of 44.1 kHz stereo sound, two faces present
throughout: tracks 00 and 01."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from avcer_amd import avi, chart, synth
from avcer_amd import run as arun
from avcer_amd.dataset import VideoJob, run_dataset
from avcer_amd.engine import MODE_F16X3
from avcer_amd.fusion import MODEL_ORDER
from test_avi_cpu import jpeg_file, pcm_of
from test_gpu_stream import tree

pytestmark = pytest.mark.gpu

W, H, FRAMES = 64, 48, 40
KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")
SMALL = (64, 256)  # plot_size of most cases: the picture of tests/chart_cases.py, wider
NAME = "pedicted_CEs_Rule 2.jpg"


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


def detections(n=FRAMES):
    dets = []
    for t in range(n):
        dets.append(np.array([[4 + t % 3, 5, 28 + t % 3, 41, 0.99] + [0] * 10,                   # face A: track 00
                              [36, 6 + t % 2, 60, 40 + t % 2, 0.98] + [0] * 10], dtype=np.float32))  # face B: track 01
    return dets


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    root = tmp_path_factory.mktemp("chart")
    blobs = [jpeg_file(W, H, 300 + i, 2, quality=92) for i in range(FRAMES)]
    bgr = np.ascontiguousarray(np.stack([np.array(Image.open(io.BytesIO(b)).convert("RGB"))[..., ::-1] for b in blobs]))
    pcm = pcm_of(70560, 2, seed=5)
    return dict(bgr=bgr, pcm=pcm, path=str(avi.write_avi(root / "pair.avi", blobs, 25, 1, pcm)))


def want_bytes(out, size=(200, 1200)):
    """PIL's file of the CPU statement's picture of a result dict's four tables."""
    table = np.stack([out[name.lower()] for name in MODEL_ORDER])
    pic = chart.chart_numpy(table, chart.chart_plan(table.shape[1], width=size[1], height=size[0]))
    b = io.BytesIO()
    Image.fromarray(pic).save(b, "JPEG", quality=95, subsampling=2)
    return b.getvalue()


def same(got, ref, what=""):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")


def test_run_inference_writes_the_chart_and_changes_nothing_else(engine_all, clip, tmp_path):
    kw = dict(detections=detections(), wav_sr=44100, mode=MODE_F16X3, flag_save_prob=True, name_video="pair")
    off = arun.run_inference(engine_all, clip["bgr"], clip["pcm"], 25, path_save_results=str(tmp_path / "off"), **kw)
    on = arun.run_inference(engine_all, clip["bgr"], clip["pcm"], 25, path_save_results=str(tmp_path / "on"), flag_save_plot_pred=True, **kw)
    assert "plot_pred" not in off and on["plot_pred"] == str(tmp_path / "on" / NAME)
    same(on, off)
    assert set(on) == set(off) | {"plot_pred"}
    files_on, files_off = tree(tmp_path / "on"), tree(tmp_path / "off")
    assert set(files_on) == set(files_off) | {NAME}
    for name, data in files_off.items():
        assert files_on[name] == data, name
    assert files_on[NAME] == want_bytes(on)                                            # the default picture, 1200 x 200
    assert Image.open(io.BytesIO(files_on[NAME])).size == (1200, 200)
    # Rule 1, and a picture size of the caller's
    r1 = arun.run_inference(engine_all, clip["bgr"], clip["pcm"], 25, detections=detections(), wav_sr=44100, mode=MODE_F16X3, ce_weights_type=False,
                            ce_mask=True, path_save_results=str(tmp_path / "r1"), flag_save_plot_pred=True, plot_size=SMALL)
    assert r1["plot_pred"] == str(tmp_path / "r1" / "pedicted_CEs_Rule 1.jpg") and sorted(os.listdir(tmp_path / "r1")) == ["pedicted_CEs_Rule 1.jpg"]
    assert (tmp_path / "r1" / "pedicted_CEs_Rule 1.jpg").read_bytes() == want_bytes(r1, SMALL)


def test_a_chart_per_selected_track(engine_all, clip, tmp_path):
    kw = dict(detections=detections(), wav_sr=44100, mode=MODE_F16X3, tracks="all")
    off = arun.run_inference(engine_all, clip["bgr"], clip["pcm"], 25, **kw)
    on = arun.run_inference(engine_all, clip["bgr"], clip["pcm"], 25, path_save_results=str(tmp_path), flag_save_plot_pred=True, plot_size=SMALL, **kw)
    assert list(on["tracks"]) == [0, 1] == list(off["tracks"])
    same(on, off)
    assert sorted(os.listdir(tmp_path)) == [NAME, "pedicted_CEs_Rule 2__t01.jpg"]
    assert on["plot_pred"] == on["tracks"][0]["plot_pred"] == str(tmp_path / NAME)
    assert on["tracks"][1]["plot_pred"] == str(tmp_path / "pedicted_CEs_Rule 2__t01.jpg")
    for k in (0, 1):
        for key in ("av", "vs", "vd", "a"):
            np.testing.assert_array_equal(on["tracks"][k][key], off["tracks"][k][key])
        with open(on["tracks"][k]["plot_pred"], "rb") as f:
            assert f.read() == want_bytes(on["tracks"][k], SMALL), f"track {k}"


def test_streamed_call_writes_the_same_bytes(engine_all, clip, tmp_path):
    kw = dict(detections=detections(), mode=MODE_F16X3, flag_save_plot_pred=True, plot_size=SMALL)
    whole = arun.run_inference_file(engine_all, clip["path"], path_save_results=str(tmp_path / "whole"), **kw)
    parts = arun.run_inference_file(engine_all, clip["path"], path_save_results=str(tmp_path / "parts"), stream_frames=16, **kw)
    same(parts, whole)
    assert whole["plot_pred"] == str(tmp_path / "whole" / NAME) and parts["plot_pred"] == str(tmp_path / "parts" / NAME)
    data = (tmp_path / "whole" / NAME).read_bytes()
    assert data == want_bytes(whole, SMALL) and (tmp_path / "parts" / NAME).read_bytes() == data


def test_run_dataset_writes_every_videos_single_call_bytes(engine_all, clip, tmp_path):
    """3 unequal videos, one batched chart call for the set: each file is that video's own run_inference file."""
    specs = (("long", 40, 25), ("mid", 33, 30), ("short", 9, 25))
    wavs = {name: synth.waveforms(60 + i, 1, int(n / fps * 16000))[0] for i, (name, n, fps) in enumerate(specs)}
    jobs = [VideoJob(name, n, H, W, fps, len(wavs[name]), detections=detections(n), load=lambda name=name, n=n: (clip["bgr"][:n], wavs[name]))
            for name, n, fps in specs]
    off = run_dataset(engine_all, jobs, mode=MODE_F16X3)
    got = run_dataset(engine_all, jobs, mode=MODE_F16X3, path_save_results=str(tmp_path / "set"), flag_save_plot_pred=True, plot_size=SMALL)
    assert sorted(tree(tmp_path / "set")) == sorted(os.path.join(name, NAME) for name, _, _ in specs)
    for job, res, res_off in zip(jobs, got, off):
        same(res, res_off, job.name)
        assert "plot_pred" not in res_off and res["plot_pred"] == str(tmp_path / "set" / job.name / NAME)
        one = arun.run_inference(engine_all, clip["bgr"][:job.n_frames], wavs[job.name], job.fps, detections=job.detections, mode=MODE_F16X3,
                                 name_video=job.name, path_save_results=str(tmp_path / "one" / job.name), flag_save_plot_pred=True, plot_size=SMALL)
        data = (tmp_path / "one" / job.name / NAME).read_bytes()
        assert (tmp_path / "set" / job.name / NAME).read_bytes() == data == want_bytes(one, SMALL), job.name
