"""run.run_inference against the building blocks it no longer calls.

The in-memory and the streamed call share one pass loop (run._run), so "streamed equals in memory" (tests/test_gpu_stream.py)
compares the loop with itself.  Here the loop is held against the independent statement of the pipeline: VideoTiler.process ->
track_clip's dense clip -> visual_forward / heatmaps.visual_forward_cam -> audio_forward -> fusion.fuse -> replicate_per_frame, on
test_gpu_stream.py's own clip (37 frames of 64 x 48, two faces, track 00 gone from frame 31, 3 s of sound), at 25 and 30 frames per
second, in MODE_F16X3 and MODE_FP32.  Every comparison is bit for bit.  Beside it: the failure path of AVPipeline.clip_records'
side stream, and preprocess_video_and_predict's range-contract guard on its plain path."""
import numpy as np
import pytest
import torch

from avcer_amd import audio_pipeline as ap
from avcer_amd import avi, fusion, heatmaps, jpeg
from avcer_amd import pipeline as apipe
from avcer_amd import run as arun
from avcer_amd import synth
from avcer_amd import video_pipeline as vp
from avcer_amd.engine import MODE_F16X3, MODE_FP32
from avcer_amd.face_tiles import VideoTiler, track_clip
from test_gpu_stream import FRAMES, KEYS, assert_same, clips, detections, engine_all  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CASES = [(25, MODE_F16X3), (25, MODE_FP32), (30, MODE_F16X3), (30, MODE_FP32)]


@pytest.fixture(scope="module")
def decoded(engine_all, clips):
    """The clip's frames, decoded once (the frames do not depend on the rate), and its source audio."""
    with avi.open_avi(clips[0][25]) as a:
        frames, _ = jpeg.decode_frames(engine_all, a.frames, a.height, a.width, bgr=True)
        return frames, np.array(a.pcm), int(a.audio_rate)


def run(engine, decoded, rate, mode, **kw):
    """run_inference on the decoded clip; the mode asked for is the mode that ran."""
    frames, pcm, audio_rate = decoded
    before = engine.x3_fallbacks
    out = arun.run_inference(engine, kw.pop("frames", frames), pcm, rate, detections=detections(), wav_sr=audio_rate, mode=mode, **kw)
    assert engine.x3_fallbacks == before
    return out


def audio_and_fusion(engine, decoded, stat, dyn, rate, mode):
    _, pcm, audio_rate = decoded
    win_logits, lo, hi = ap.audio_forward(engine, torch.from_numpy(pcm).to(engine.device), 16000, rate, 4, 0.5, "mean", mode, wav_sr=audio_rate)
    prob, am = fusion.fuse(engine, stat, dyn, win_logits, lo, hi, None, (1, 1, 1), True, False)  # run_inference's defaults
    rows, at = ap.replicate_per_frame(win_logits.cpu().numpy(), lo, hi)
    want = {name.lower(): am.cpu().numpy()[i] for i, name in enumerate(fusion.MODEL_ORDER)}
    want.update(compound_prob=prob.cpu().numpy(), static_probs=stat.cpu().numpy(), dynamic_logits=dyn.cpu().numpy(), audio_rows=rows, audio_frames=at)
    return want


@pytest.mark.parametrize("via_jpeg", [False, True])
@pytest.mark.parametrize("rate,mode", CASES)
def test_run_inference_equals_the_chain_of_building_blocks(engine_all, decoded, rate, mode, via_jpeg):
    eng, frames = engine_all, decoded[0]
    got = run(eng, decoded, rate, mode, faces_via_jpeg=via_jpeg)
    records, tiles = VideoTiler(eng).process(frames, detections(), via_jpeg=via_jpeg)
    assert len(records) == 31 + 18 and set(records[:, 1]) == {0, 1, 2}
    stat, dyn = vp.visual_forward(eng, *track_clip(records, tiles, 0, FRAMES), rate, mode)
    want = audio_and_fusion(eng, decoded, stat, dyn, rate, mode)
    want["records"] = records
    assert_same(got, want, f"{rate} {mode} {via_jpeg}")


@pytest.mark.parametrize("rate,mode", CASES)
def test_heat_maps_equal_visual_forward_cam_and_cam_render(engine_all, decoded, rate, mode):
    """The overlays as the in-memory call composed them before it shared the pass loop: the maps of visual_forward_cam on the dense
    clip, the base image one crop_resize_linear call over the heat-map frames' rectangles (of the round-tripped crops with
    faces_via_jpeg), one cam_render call."""
    eng, frames = engine_all, decoded[0]
    for via_jpeg in (False, True):
        records, tiles = VideoTiler(eng).process(frames, detections(), via_jpeg=via_jpeg)
        clip, present = track_clip(records, tiles, 0, FRAMES)
        for model in heatmaps.MODELS:
            got = run(eng, decoded, rate, mode, faces_via_jpeg=via_jpeg, flag_heatmaps=True, model_heatmaps=model)
            stat, dyn, cam, fidx, rows, cls = heatmaps.visual_forward_cam(eng, clip, present, rate, mode, model)
            assert fidx.tolist() == list(range(0, 31, vp.lstm_step(rate)))
            r00 = records[records[:, 1] == 0]
            pick = r00[np.searchsorted(r00[:, 0], fidx)]
            assert pick[:, 0].tolist() == fidx.tolist()
            rects = torch.from_numpy(pick[:, [0, 2, 3, 4, 5]].astype(np.int32))
            if via_jpeg:
                base = eng.crop_resize_linear(*jpeg.roundtrip_canvas(eng, frames, rects, bgr=True), swap_rb=False)
            else:
                base = eng.crop_resize_linear(frames, rects, swap_rb=True)
            want = eng.cam_render(cam, rows, cls, base, heatmaps.JET_BGR, heatmaps.IMAGE_WEIGHT).cpu().numpy()
            what = f"{rate} {mode} {via_jpeg} {model}"
            assert got["heatmaps"][0].dtype == np.int32 and got["heatmaps"][1].dtype == np.uint8, what
            np.testing.assert_array_equal(got["heatmaps"][0], fidx, err_msg=what)
            np.testing.assert_array_equal(got["heatmaps"][1], want, err_msg=what)
            np.testing.assert_array_equal(got["static_probs"], stat.cpu().numpy(), err_msg=what)
            np.testing.assert_array_equal(got["dynamic_logits"], dyn.cpu().numpy(), err_msg=what)


@pytest.mark.parametrize("rate,mode", CASES)
def test_frames_as_numpy_host_tensor_and_device_tensor(engine_all, decoded, rate, mode):
    frames = decoded[0]
    on_device = run(engine_all, decoded, rate, mode)
    host = frames.cpu()
    assert frames.is_cuda and not host.is_cuda
    for what, given in (("host tensor", host), ("numpy", host.numpy())):
        got = run(engine_all, decoded, rate, mode, frames=given)
        assert set(got) == set(on_device)
        assert_same(got, on_device, what)


def test_clip_records_joins_the_audio_branch_when_the_visual_branch_fails(engine_all, sd_static, sd_dynamic, sd_audio, monkeypatch):
    """A host exception in the visual branch (nothing faults on the device) unwinds through the side stream's join: the audio
    launches already queued do not outlive the call, so the next call on the same pipeline is a fresh pipeline's, and no count of
    theirs is charged to it."""
    eng = engine_all
    pipe = apipe.AVPipeline.__new__(apipe.AVPipeline)
    pipe.engine, pipe.mode, pipe.overlap_branches = eng, MODE_F16X3, True
    n, t = 4, 10
    frames = torch.from_numpy(synth.face_frames(411, n * t).reshape(n, t, 224, 224, 3)).to(eng.device)
    wav = torch.from_numpy(synth.waveforms(412, n, 32000)).to(eng.device)
    before = eng.x3_fallbacks

    def broken(*a, **kw):
        raise RuntimeError("the visual branch failed")

    with monkeypatch.context() as mp:
        mp.setattr(apipe, "visual_forward", broken)
        with pytest.raises(RuntimeError, match="the visual branch failed"):
            pipe.clip_records(frames, wav, 25)
    got = pipe.clip_records(frames, wav, 25)
    assert eng.x3_fallbacks == before
    fresh = apipe.AVPipeline(eng.device.index, state_dicts=(sd_static, sd_dynamic, sd_audio), mode=MODE_F16X3)
    try:
        assert fresh.overlap_branches and fresh.engine is not eng
        want = fresh.clip_records(frames, wav, 25)
        assert len(got) == len(want) == 3 and fresh.engine.x3_fallbacks == 0
        for g, w in zip(got, want):
            assert g.shape == w.shape and torch.equal(g, w)
    finally:
        fresh.engine.close()
        torch.cuda.set_device(eng.device)


def test_preprocess_video_and_predict_is_guarded_without_heat_maps(engine_all, decoded, sd_static, tmp_path):
    """test_gpu_stream.py's armed static model (fc1 x 1e6) leaves fp16's range: in MODE_F16X3 the plain path counts one fallback and
    returns the MODE_FP32 tables.  Unarmed the counter stays put and the tables are visual_forward's on the folder's tiles."""
    eng = engine_all
    run(eng, decoded, 25, MODE_FP32, path_save_faces=str(tmp_path), name_video="talk")
    folder = str(tmp_path / "talk")
    tiles, present = vp.read_face_dir_device(eng, folder, FRAMES)
    assert present.tolist() == [t < 31 for t in range(FRAMES)]
    for fps in (25, 30):
        before = eng.x3_fallbacks
        dyn, stat = vp.preprocess_video_and_predict(eng, folder, fps=fps, total_frames=FRAMES, mode=MODE_F16X3)
        assert eng.x3_fallbacks == before
        want = vp.visual_forward(eng, tiles, present, fps, MODE_F16X3)
        np.testing.assert_array_equal(stat, want[0].cpu().numpy())
        np.testing.assert_array_equal(dyn, want[1].cpu().numpy())
    armed = dict(sd_static)
    armed["fc1.weight"], armed["fc1.bias"] = sd_static["fc1.weight"] * 1.0e6, sd_static["fc1.bias"] * 1.0e6
    try:
        eng.load_static(armed)
        for fps in (25, 30):
            before = eng.x3_fallbacks
            dyn, stat = vp.preprocess_video_and_predict(eng, folder, fps=fps, total_frames=FRAMES, mode=MODE_F16X3)
            assert eng.x3_fallbacks == before + 1
            dyn32, stat32 = vp.preprocess_video_and_predict(eng, folder, fps=fps, total_frames=FRAMES, mode=MODE_FP32)
            assert eng.x3_fallbacks == before + 1
            np.testing.assert_array_equal(stat, stat32)
            np.testing.assert_array_equal(dyn, dyn32)
            assert np.isfinite(stat).all()
    finally:
        eng.load_static(sd_static)
