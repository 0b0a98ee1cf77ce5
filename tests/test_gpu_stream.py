"""run.run_inference_file(stream_frames=N): a recording run through the pipeline in passes of N frames returns, bit for bit, what the
in-memory call returns -- the dict, the CSV files, the face folders, the heat maps, the result video -- and never holds more than one
pass of decoded frames.

The clip: 37 frames of 64 x 48 (the smallest size tests/test_gpu_avi.py runs whole recordings at) with two faces.  Face A is the
first detection of frame 0, so it is track 00; face B ends on frame 20 and is missed on frames 11-13.  The tracker never revives an
id (SimpleFaceTracker drops a tracklet the frame it is not matched; a face that comes back is a NEW track), so track 00 can be
absent only from some frame to the end: here from frame 31 on, the last frame included, with the pass border of N = 5 at frame 35
inside that stretch; B's gap makes it a third track from frame 14 on, so the records change shape across pass borders.  A presence
mask with a hole in the MIDDLE (frames 11-13) and at the end is run through the shared window entry
(video_pipeline.visual_from_static) against visual_forward directly.  N = 10 cuts an LSTM window at both frame rates (the window
ending at frame 10 / 12 reads features of the pass before)."""
import math
import os
import weakref

import numpy as np
import pytest
import torch

from avcer_amd import avi, jpeg, synth
from avcer_amd import run as arun
from avcer_amd import video_pipeline as vp
from avcer_amd.engine import MODE_F16X3, MODE_FP32
from test_avi_cpu import jpeg_file, pcm_of

pytestmark = pytest.mark.gpu

W, H, FRAMES = 64, 48, 37
KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")
PASSES = (1, 5, 10, 16, 37, 64)


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


def detections(track00_until=31):
    dets = []
    for t in range(FRAMES):
        rows = []
        if t < track00_until:
            rows.append([4 + t % 3, 5, 28 + t % 3, 41, 0.99] + [0] * 10)                    # face A: track 00
        if t <= 20 and t not in (11, 12, 13):
            rows.append([36, 6 + t % 2, 60, 40 + t % 2, 0.98] + [0] * 10)                   # face B: track 01, then 02 from frame 14
        dets.append(np.array(rows, dtype=np.float32).reshape(-1, 15))
    return dets


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """The clip at 25 and at 30 frames per second (the LSTM's frame stride 5 and 6), 3 s of sound: 7 audio windows, the last one
    empty (NaN logits)."""
    root = tmp_path_factory.mktemp("stream")
    blobs = [jpeg_file(W, H, 700 + i, 2, quality=92) for i in range(FRAMES)]
    pcm = pcm_of(132300, 2, seed=11)
    return {rate: str(avi.write_avi(root / f"talk{rate}.avi", blobs, rate, 1, pcm)) for rate in (25, 30)}, blobs, pcm


def assert_same(got, ref, what=""):
    for key in KEYS:
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (what, key)
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")


def tree(root):
    """{relative path: bytes} of every file under root, and the paths in sorted order."""
    out = {}
    for folder, _, names in os.walk(root):
        for n in names:
            p = os.path.join(folder, n)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


# ---------------------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("rate", [25, 30])
def test_streamed_equals_in_memory_for_every_pass_size(engine_all, clips, rate):
    path = clips[0][rate]
    dets = detections()
    ref = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3)
    assert ref["records"][:, 1].max() == 2 and not (ref["records"][ref["records"][:, 1] == 0][:, 0] >= 31).any()
    assert vp.lstm_step(rate) == rate // 5
    for n in PASSES:
        got = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, stream_frames=n)
        assert_same(got, ref, f"stream_frames={n}")
        assert set(got) == set(ref) and got["real_time_factor"] > 0


def test_window_entry_equals_visual_forward_with_holes_in_the_track(engine_all):
    """video_pipeline.visual_from_static on the static CNN's outputs computed in PASSES of 5 frames = visual_forward on the clip, for
    a presence mask no tracker run can give: absent on frames 11-13 (the window restarts at 14 / 15 / 18) and on the last frame
    (hold-last), and one that starts absent (zero rows)."""
    tiles = torch.from_numpy(synth.face_frames(5, FRAMES)).to(engine_all.device)
    for fps in (25, 30):
        for gone in ((11, 12, 13, 36), (0, 1, 2, 20), ()):
            present = np.ones(FRAMES, dtype=bool)
            present[list(gone)] = False
            want = vp.visual_forward(engine_all, tiles, present, fps, MODE_F16X3)
            probs, feats = [], []
            for a in range(0, FRAMES, 5):
                sel = torch.from_numpy(np.flatnonzero(present[a:a + 5]) + a).to(engine_all.device)
                _, p, f = engine_all.static_forward(tiles.index_select(0, sel), MODE_F16X3)
                probs.append(p)
                feats.append(f)
            got = vp.visual_from_static(engine_all, torch.cat(probs), torch.cat(feats), present, fps, MODE_F16X3)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (fps, gone)
    with pytest.raises(ValueError, match="present frames"):
        vp.visual_from_static(engine_all, probs[0], feats[0], np.ones(FRAMES, dtype=bool), 25)


# ---------------------------------------------------------------------------------------------------- options
@pytest.mark.parametrize("model", ["static", "dynamic"])
def test_heat_maps_streamed(engine_all, clips, tmp_path, model):
    path, dets = clips[0][25], detections()
    kw = dict(detections=dets, mode=MODE_F16X3, flag_heatmaps=True, model_heatmaps=model)
    ref = arun.run_inference_file(engine_all, path, path_save_results=str(tmp_path / "ref"), **kw)
    assert ref["heatmaps"][0].tolist() == list(range(0, 31, 5)) and ref["heatmaps"][1].shape == (7, 224, 224, 3)
    for n in (5, 10, 16):
        got = arun.run_inference_file(engine_all, path, path_save_results=str(tmp_path / f"s{n}"), stream_frames=n, **kw)
        assert_same(got, ref, f"{model} {n}")
        for a, b in zip(got["heatmaps"], ref["heatmaps"]):
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a, b, err_msg=f"{model} {n}")
        assert tree(tmp_path / f"s{n}") == tree(tmp_path / "ref") and len(tree(tmp_path / "ref")) == 7


@pytest.mark.parametrize("via_jpeg", [False, True])
def test_face_folders_and_csv_files_streamed(engine_all, clips, tmp_path, via_jpeg):
    path, dets = clips[0][30], detections()
    kw = dict(detections=dets, mode=MODE_F16X3, faces_via_jpeg=via_jpeg, flag_save_prob=True, flag_heatmaps=via_jpeg)

    def call(name, **more):
        out = arun.run_inference_file(engine_all, path, path_save_faces=str(tmp_path / name / "faces"),
                                      path_save_results=str(tmp_path / name / "res"), **kw, **more)
        return out, [os.path.relpath(p, tmp_path / name) for p in out["face_files"]]

    ref, ref_files = call("ref")
    assert len(ref_files) == len(ref["records"]) == 31 + 18
    for n, entropy in ((5, "host"), (16, "device")):
        got, files = call(f"s{n}", stream_frames=n, jpeg_entropy=entropy)
        assert_same(got, ref, f"{via_jpeg} {n}")
        assert files == ref_files                                                   # the same paths in the same order
        assert tree(tmp_path / f"s{n}") == tree(tmp_path / "ref")                   # faces, CSV files (and heat maps) byte for byte
        if via_jpeg:
            np.testing.assert_array_equal(got["heatmaps"][1], ref["heatmaps"][1])
    names = sorted(tree(tmp_path / "ref"))
    assert sum(n.endswith(".csv") for n in names) == 3 and sum(n.startswith("faces") for n in names) == 49
    # streamed and not via the files: the results of the plain call
    if via_jpeg:
        plain = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, faces_via_jpeg=True, stream_frames=10)
        assert_same(plain, ref, "via_jpeg without files")


def test_result_video_streamed(engine_all, clips, tmp_path):
    path, dets = clips[0][25], detections()
    kw = dict(detections=dets, mode=MODE_F16X3, video_panel=True)
    ref = arun.run_inference_file(engine_all, path, path_save_video=str(tmp_path / "ref.avi"), **kw)
    got = arun.run_inference_file(engine_all, path, path_save_video=str(tmp_path / "s5.avi"), stream_frames=5, **kw)
    assert_same(got, ref)
    assert got["result_video"] == str(tmp_path / "s5.avi")
    assert (tmp_path / "s5.avi").read_bytes() == (tmp_path / "ref.avi").read_bytes()
    with avi.open_avi(tmp_path / "s5.avi") as a:
        assert (a.n_frames, a.width, a.height, a.rate, a.scale) == (FRAMES, W, H, 25, 1)
        np.testing.assert_array_equal(a.pcm, clips[2])


def test_audio_windows_per_pass_changes_nothing(engine_all, clips):
    path, dets = clips[0][25], detections()
    ref = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3)
    rows = ref["audio_rows"]
    from avcer_amd.audio_pipeline import chunk_spans

    starts, ends, _, _ = chunk_spans(48000, 16000, 25, 4, 0.5)
    assert len(starts) == 7 and ends[-1] == starts[-1]                              # 7 windows, the last one empty: NaN logits
    for per in (1, 3, 128):
        got = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, stream_frames=16, audio_windows_per_pass=per)
        assert_same(got, ref, f"audio_windows_per_pass={per}")
    for bad in (0, -2, True, 1.5):
        with pytest.raises(ValueError, match="audio_windows_per_pass"):
            arun.run_inference_file(engine_all, path, detections=dets, stream_frames=16, audio_windows_per_pass=bad)


# ---------------------------------------------------------------------------------------------------- bounded memory
def test_no_more_than_one_pass_of_frames_is_alive(engine_all, clips, tmp_path, monkeypatch):
    path, dets = clips[0][25], detections()
    real = jpeg.decode_frames
    asked, alive, stale = [], [], []

    def spy(engine, blobs, *a, **kw):
        stale.append(sum(r() is not None for r in alive[:-1]))                      # passes before the previous one still referenced
        asked.append(len(blobs))
        frames, paths = real(engine, blobs, *a, **kw)
        alive.append(weakref.ref(frames))
        return frames, paths

    monkeypatch.setattr(jpeg, "decode_frames", spy)
    arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, stream_frames=5, flag_heatmaps=True)
    per_sweep = math.ceil(FRAMES / 5)
    assert asked == [5] * (per_sweep - 1) + [2] and max(asked) <= 5
    assert stale == [0] * per_sweep
    del asked[:], alive[:], stale[:]
    arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, stream_frames=5, path_save_video=str(tmp_path / "v.avi"),
                            path_save_faces=str(tmp_path / "faces"), faces_via_jpeg=True)
    assert asked == ([5] * (per_sweep - 1) + [2]) * 2                                # the second sweep: the result video
    assert stale == [0] * (2 * per_sweep)
    assert sum(r() is not None for r in alive) == 0                                  # and nothing outlives the call


# ---------------------------------------------------------------------------------------------------- arguments and failures
def test_bad_stream_frames_raise_before_the_file_is_opened(engine_all, clips, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("open_avi was called")

    monkeypatch.setattr(avi, "open_avi", never)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="stream_frames"):
            arun.run_inference_file(engine_all, clips[0][25], detections=detections(), stream_frames=bad)


def test_refusals_come_before_the_first_decode(engine_all, clips, tmp_path, monkeypatch):
    path, dets, (_, blobs, pcm) = clips[0][25], detections(), clips
    monkeypatch.setattr(jpeg, "decode_frames", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("decoded")))
    mute = str(avi.write_avi(tmp_path / "mute.avi", blobs, 25))
    odd = str(avi.write_avi(tmp_path / "odd.avi", blobs, 25, pcm=pcm, audio_rate=12345))
    for file, kw, match in ((mute, {}, "no audio stream"), (odd, {}, "12345"), (path, dict(window=60), "max_tokens"),
                            (path, dict(detections=None), "detector"), (path, dict(video_model="x"), "video_model"),
                            (path, dict(flag_heatmaps=True, model_heatmaps="x"), "model_heatmaps"), (path, dict(jpeg_entropy="x"), "jpeg_entropy"),
                            (path, dict(faces_via_jpeg=1), "faces_via_jpeg"), (path, dict(detections=dets[:5]), "one detection array per frame")):
        with pytest.raises(ValueError, match=match):
            arun.run_inference_file(engine_all, file, **{"detections": dets, "stream_frames": 5, **kw})
    with pytest.raises(TypeError, match="no_such_option"):
        arun.run_inference_file(engine_all, path, detections=dets, stream_frames=5, no_such_option=1)


def test_no_track_00_raises_at_the_end_and_leaves_the_engine_clean(engine_all, clips):
    path = clips[0][25]
    nobody = [np.zeros((0, 15), dtype=np.float32)] * FRAMES
    with pytest.raises(FileNotFoundError) as want:
        arun.run_inference_file(engine_all, path, detections=nobody, mode=MODE_F16X3)
    with pytest.raises(FileNotFoundError) as got:
        arun.run_inference_file(engine_all, path, detections=nobody, mode=MODE_F16X3, stream_frames=5)
    assert str(got.value) == str(want.value)
    # nothing of the failed call is left queued: an ordinary call on the same engine is right, in memory and streamed
    dets = detections()
    ref = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_FP32)
    with pytest.raises(FileNotFoundError):
        arun.run_inference_file(engine_all, path, detections=nobody, mode=MODE_F16X3, stream_frames=16)
    assert_same(arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_FP32), ref)
    assert_same(arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_FP32, stream_frames=16), ref)
    # a zero-area detection in the third pass names the frame of the whole video
    bad = list(dets)
    bad[12] = np.array([[10, 10, 10, 30, 0.9] + [0] * 10], dtype=np.float32)
    with pytest.raises(ValueError, match="^frame 12: a zero-area detection"):
        arun.run_inference_file(engine_all, path, detections=bad, mode=MODE_F16X3, stream_frames=5)


def test_overflow_repeats_the_streamed_sweep_in_fp32(engine_all, clips, sd_static, tmp_path):
    """A static model whose fc1 is scaled by 1e6 hands the LSTM features far outside fp16's range: the x3 pass counts an overflow
    and the whole call is repeated in fp32 (Engine.guarded) -- streamed too, with the same result, and the face files written once."""
    path, dets, eng = clips[0][25], detections(), engine_all
    armed = dict(sd_static)
    armed["fc1.weight"], armed["fc1.bias"] = sd_static["fc1.weight"] * 1.0e6, sd_static["fc1.bias"] * 1.0e6
    try:
        eng.load_static(armed)
        before = eng.x3_fallbacks
        ref = arun.run_inference_file(eng, path, detections=dets, mode=MODE_F16X3)
        assert eng.x3_fallbacks == before + 1, "the armed model must overflow fp16 in the in-memory call"
        assert_same(ref, arun.run_inference_file(eng, path, detections=dets, mode=MODE_FP32), "fp32")
        for n in (5, 16):
            got = arun.run_inference_file(eng, path, detections=dets, mode=MODE_F16X3, stream_frames=n, path_save_faces=str(tmp_path / f"f{n}"))
            assert_same(got, ref, f"armed {n}")
            assert len(got["face_files"]) == len(ref["records"]) == len(tree(tmp_path / f"f{n}"))
        assert eng.x3_fallbacks == before + 3
        assert np.isfinite(ref["static_probs"]).all()
    finally:
        eng.load_static(sd_static)
