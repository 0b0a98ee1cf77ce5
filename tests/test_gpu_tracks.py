"""`tracks=` on run.run_inference / run.run_inference_file / annotate.write_result_video: the visual models and the fusion on every
selected face track of a recording, inside one call.

For a track k the claim is identity, bit for bit and in the same arithmetic mode, with what the code gives when that track is fed
to it alone as the reference would read it from a folder named `00`: `visual_forward(engine, *track_clip(records, tiles, k, T), fps,
mode)` and `fusion.fuse` on those tables and the call's window logits.

The clip: 40 frames of 160 x 120 with 25 600 samples of sound at 16 kHz (four windows of 4 s), three faces in disjoint corners that
move by a pixel per frame.  Face A is there throughout but on frames 11-13, face B on frames 7-29, face C on frame 20 alone.  The
tracker never revives an id, so A comes back as a new track: the track numbers are taken from `records`."""
import io
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from avcer_amd import avi, fusion, synth
from avcer_amd import run as arun
from avcer_amd import video_pipeline as vp
from avcer_amd.audio_pipeline import audio_forward, chunk_spans
from avcer_amd.engine import MODE_F16X3, MODE_FP32
from avcer_amd.face_tiles import VideoTiler, track_clip
from avcer_amd.fusion import MODEL_ORDER
from test_avi_cpu import jpeg_file, pcm_of
from test_gpu_annotate import oracle_files

pytestmark = pytest.mark.gpu

W, H, FRAMES, SAMPLES = 160, 120, 40, 25600
TOP = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")
PER_TRACK = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "present")
A_GONE, B_SPAN, C_AT = (11, 12, 13), range(7, 30), 20


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


def detections():
    dets = []
    for t in range(FRAMES):
        rows = []
        if t not in A_GONE:
            rows.append([4 + t, 4, 44 + t, 50, 0.99] + [0] * 10)                          # face A: top left, moving right
        if t in B_SPAN:
            rows.append([100 - t, 64, 138 - t, 112, 0.98] + [0] * 10)                    # face B: bottom, moving left
        if t == C_AT:
            rows.append([112, 6, 152, 52, 0.97] + [0] * 10)                              # face C: top right, one frame
        dets.append(np.array(rows, dtype=np.float32).reshape(-1, 15))
    return dets


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """The frames as JPEG files, as PIL decodes them (BGR), the sound at 16 kHz, and the recording at 25 and 30 frames per second
    with 70 560 stereo samples at 44.1 kHz: 25 600 samples at 16 kHz."""
    root = tmp_path_factory.mktemp("tracks")
    blobs = [jpeg_file(W, H, 900 + i, 2, quality=92) for i in range(FRAMES)]
    bgr = np.stack([np.array(Image.open(io.BytesIO(b)).convert("RGB"))[..., ::-1] for b in blobs])
    pcm = pcm_of(70560, 2, seed=17)
    paths = {rate: str(avi.write_avi(root / f"three{rate}.avi", blobs, rate, 1, pcm)) for rate in (25, 30)}
    starts, _, _, _ = chunk_spans(SAMPLES, 16000, 25, 4, 0.5)
    assert len(starts) == 4
    return dict(bgr=np.ascontiguousarray(bgr), wav=synth.waveforms(23, 1, SAMPLES)[0], pcm=pcm, paths=paths, blobs=blobs)


_REFERENCE = {}


def reference(engine, clip, fps, mode):
    """{track: its tables by the per-track path of the code as it stands}, computed once per (fps, mode) and never modified; and the
    records."""
    key = (fps, mode)
    if key not in _REFERENCE:
        frames = torch.from_numpy(clip["bgr"]).to(engine.device)
        records, tiles = VideoTiler(engine).process(frames, detections())
        wav = torch.from_numpy(clip["wav"]).to(engine.device)
        win_logits, lo, hi = audio_forward(engine, wav, 16000, fps, 4, 0.5, "mean", mode)
        per = {}
        for k in sorted(set(records[:, 1].tolist())):
            frames_k, present = track_clip(records, tiles, k, FRAMES)
            stat, dyn = vp.visual_forward(engine, frames_k, present, fps, mode)
            prob, am = fusion.fuse(engine, stat, dyn, win_logits, lo, hi, None, (1, 1, 1), True, False)   # run_inference's defaults
            am = am.cpu().numpy()
            one = {name.lower(): am[i] for i, name in enumerate(MODEL_ORDER)}
            one.update(compound_prob=prob.cpu().numpy(), static_probs=stat.cpu().numpy(), dynamic_logits=dyn.cpu().numpy(), present=present)
            for v in one.values():
                v.setflags(write=False)
            per[k] = one
        _REFERENCE[key] = (per, records)
    return _REFERENCE[key]


def who(records):
    """(track of face A's first stretch, of face B, of face C, of face A behind its gap), read off the records."""
    def track_at(frame, x0):
        hit = records[(records[:, 0] == frame) & (records[:, 2] == x0)]
        assert len(hit) == 1
        return int(hit[0, 1])

    return track_at(0, 4), track_at(7, 93), track_at(C_AT, 112), track_at(39, 43)


def same_track(got, want, what):
    assert set(got) == set(PER_TRACK), what
    for key in PER_TRACK:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


def same_top(got, want, what="", keys=TOP):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


def same_call(got, want, what=""):
    same_top(got, want, what)
    assert list(got["tracks"]) == list(want["tracks"]), what
    for k in want["tracks"]:
        same_track(got["tracks"][k], want["tracks"][k], f"{what} track {k}")


def tree(root):
    out = {}
    for folder, _, names in os.walk(root):
        for n in names:
            p = os.path.join(folder, n)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


def run(engine, clip, fps=25, mode=MODE_F16X3, **kw):
    return arun.run_inference(engine, clip["bgr"], clip["wav"], fps, detections=detections(), mode=mode, **kw)


# ---------------------------------------------------------------------------------------------------- 1, 2: the tables
@pytest.mark.parametrize("fps,mode", [(25, MODE_F16X3), (25, MODE_FP32), (30, MODE_F16X3)])
def test_all_tracks_equal_the_per_track_path(engine_all, clip, fps, mode):
    before = engine_all.x3_fallbacks
    want, records = reference(engine_all, clip, fps, mode)
    a0, b, c, a1 = who(records)
    assert a0 == 0 and len({a0, b, c, a1}) == 4 and sorted(want) == sorted({a0, b, c, a1})     # the gap made face A two tracks
    assert want[a0]["present"].tolist() == [t < 11 for t in range(FRAMES)]
    assert want[b]["present"].tolist() == [t in B_SPAN for t in range(FRAMES)]
    assert want[c]["present"].tolist() == [t == C_AT for t in range(FRAMES)]
    assert want[a1]["present"].tolist() == [t >= 14 for t in range(FRAMES)]
    got = run(engine_all, clip, fps, mode, tracks="all")
    assert engine_all.x3_fallbacks == before                                                   # the mode asked for is the mode compared
    assert list(got["tracks"]) == sorted(want)
    for k in want:
        same_track(got["tracks"][k], want[k], f"track {k}")
    assert not np.array_equal(got["tracks"][b]["static_probs"], got["tracks"][a1]["static_probs"])
    plain = run(engine_all, clip, fps, mode)
    assert "tracks" not in plain
    same_top(got, plain, "all against None")
    assert set(got) == set(plain) | {"tracks"}
    zero = run(engine_all, clip, fps, mode, tracks=[0])
    same_top(zero, plain, "[0] against None")
    assert list(zero["tracks"]) == [0] and set(zero) == set(plain) | {"tracks"}
    same_track(zero["tracks"][0], want[0], "[0]")
    # every returned table has storage of its own: editing the top level in place leaves the per-track entry alone
    tables = [got[key] for key in TOP[:7]] + [one[key] for one in got["tracks"].values() for key in PER_TRACK]
    assert not any(np.shares_memory(a, b) for i, a in enumerate(tables) for b in tables[i + 1:])


def test_the_order_given_is_honoured_and_the_first_track_is_the_top_level(engine_all, clip):
    want, records = reference(engine_all, clip, 25, MODE_F16X3)
    _, b, _, _ = who(records)
    got = run(engine_all, clip, tracks=[b, 0])
    assert list(got["tracks"]) == [b, 0]
    same_track(got["tracks"][b], want[b], "B")
    same_track(got["tracks"][0], want[0], "00")
    same_top(got, want[b], "top level", keys=PER_TRACK[:-1])
    plain = run(engine_all, clip)
    same_top(got, plain, "the video's own keys", keys=("audio_rows", "audio_frames", "records"))
    assert not np.array_equal(got["static_probs"], plain["static_probs"])


# ---------------------------------------------------------------------------------------------------- 3: streamed
@pytest.mark.parametrize("rate", [25, 30])
def test_streamed_equals_in_memory(engine_all, clip, tmp_path, rate):
    path, dets = clip["paths"][rate], detections()
    kw = dict(detections=dets, mode=MODE_F16X3, tracks="all", flag_save_prob=True, video_panel=True)
    ref = arun.run_inference_file(engine_all, path, path_save_results=str(tmp_path / "ref"), path_save_video=str(tmp_path / "ref.avi"), **kw)
    assert len(ref["tracks"]) == 4 and ref["audio_rows"].shape[0] > 0
    names = sorted(tree(tmp_path / "ref"))
    stem = f"three{rate}"
    tails = [""] + [f"__t{k:02d}" for k in list(ref["tracks"])[1:]]                         # the first track under today's names
    assert names == sorted([f"{kind}__{stem}{tail}.csv" for kind in ("static", "dynamic") for tail in tails] +
                           [os.path.join("audio", f"{stem}{tail}.csv") for tail in tails])
    for n in (16, 7):
        got = arun.run_inference_file(engine_all, path, path_save_results=str(tmp_path / f"s{n}"), path_save_video=str(tmp_path / f"s{n}.avi"),
                                      stream_frames=n, **kw)
        same_call(got, ref, f"stream_frames={n}")
        assert tree(tmp_path / f"s{n}") == tree(tmp_path / "ref")
        assert (tmp_path / f"s{n}.avi").read_bytes() == (tmp_path / "ref.avi").read_bytes()
    # a list, in an order of its own, streamed: the kept state is that of the named tracks alone
    order = [who(ref["records"])[3], 0]
    listed = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, tracks=order, stream_frames=7)
    assert list(listed["tracks"]) == order
    for k in order:
        same_track(listed["tracks"][k], ref["tracks"][k], f"listed {k}")
    # the CSV files of the first track are those of the plain call
    arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_F16X3, flag_save_prob=True, path_save_results=str(tmp_path / "plain"))
    plain = tree(tmp_path / "plain")
    assert len(plain) == 3 and all(tree(tmp_path / "ref")[name] == data for name, data in plain.items())


# ---------------------------------------------------------------------------------------------------- 4: the result video
def test_result_video_labels_every_selected_track(engine_all, clip, tmp_path):
    path, dets = clip["paths"][25], detections()
    kw = dict(detections=dets, mode=MODE_F16X3, video_model="vs")
    got = arun.run_inference_file(engine_all, path, path_save_video=str(tmp_path / "all.avi"), tracks="all", **kw)
    j = [m.lower() for m in MODEL_ORDER].index("vs")
    pred = {k: one["vs"] for k, one in got["tracks"].items()}
    prob = {k: one["compound_prob"][j] for k, one in got["tracks"].items()}
    want = avi.build_avi(oracle_files(clip["bgr"], got["records"], pred, prob, 90, 2), 25, 1, clip["pcm"], 44100)
    assert (tmp_path / "all.avi").read_bytes() == want
    arun.run_inference_file(engine_all, path, path_save_video=str(tmp_path / "none.avi"), **kw)
    none = (tmp_path / "none.avi").read_bytes()
    assert none == avi.build_avi(oracle_files(clip["bgr"], got["records"], pred[0], prob[0], 90, 2), 25, 1, clip["pcm"], 44100)
    assert none != want                                                                       # the other tracks' labels were drawn
    # a list: the unselected tracks keep a bare box, and the panel is the first track's
    _, b, _, _ = who(got["records"])
    arun.run_inference_file(engine_all, path, path_save_video=str(tmp_path / "b.avi"), tracks=[b, 0], video_panel=True, **kw)
    two = avi.build_avi(oracle_files(clip["bgr"], got["records"], {b: pred[b], 0: pred[0]}, {b: prob[b], 0: prob[0]}, 90, 2, panel=True), 25, 1,
                        clip["pcm"], 44100)
    assert (tmp_path / "b.avi").read_bytes() == two


# ---------------------------------------------------------------------------------------------------- 5: the folders
@pytest.mark.parametrize("mode", [MODE_F16X3, MODE_FP32])
def test_every_track_equals_the_read_back_of_its_own_folder(engine_all, clip, tmp_path, mode):
    got = run(engine_all, clip, 25, mode, tracks="all", faces_via_jpeg=True, path_save_faces=str(tmp_path / "faces"), name_video="clip")
    assert len(got["face_files"]) == len(got["records"]) and len(got["tracks"]) == 4
    raw = run(engine_all, clip, 25, mode, tracks="all")
    for k, one in got["tracks"].items():
        # the reference reads `<faces>/00` alone: the track's folder under that name
        shutil.copytree(tmp_path / "faces" / "clip" / f"{k:02d}", tmp_path / f"as00_{k}" / "clip" / "00")
        dyn, stat = vp.preprocess_video_and_predict(engine_all, str(tmp_path / f"as00_{k}" / "clip"), fps=25, total_frames=FRAMES, mode=mode)
        np.testing.assert_array_equal(one["static_probs"], stat, err_msg=f"track {k}")
        np.testing.assert_array_equal(one["dynamic_logits"], dyn, err_msg=f"track {k}")
        assert not np.array_equal(one["static_probs"], raw["tracks"][k]["static_probs"])       # the quantiser is seen by the network


# ---------------------------------------------------------------------------------------------------- 6: errors
def test_errors_leave_the_engine_clean(engine_all, clip, tmp_path, monkeypatch):
    path, dets = clip["paths"][25], detections()
    ref = run(engine_all, clip, mode=MODE_FP32)
    ref_file = arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_FP32)
    absent = int(ref["records"][:, 1].max()) + 3
    # in memory: before the visual models run
    with monkeypatch.context() as m:
        m.setattr(engine_all, "static_forward", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("the static CNN ran")))
        with pytest.raises(FileNotFoundError, match=f"no face track {absent:02d}") as in_memory:
            run(engine_all, clip, tracks=[0, absent])
    same_top(run(engine_all, clip, mode=MODE_FP32), ref, "behind the absent track")
    # streamed: at the end of the sweep, the same words
    with pytest.raises(FileNotFoundError) as streamed:
        arun.run_inference_file(engine_all, path, detections=dets, tracks=[0, absent], stream_frames=16)
    assert str(streamed.value) == str(in_memory.value)
    same_top(arun.run_inference_file(engine_all, path, detections=dets, mode=MODE_FP32, stream_frames=16), ref_file, "behind the streamed one")
    # nobody in the picture: "all" has no track, None keeps its own words
    nobody = [np.zeros((0, 15), dtype=np.float32)] * FRAMES
    for more in ({}, {"stream_frames": 7}):
        with pytest.raises(FileNotFoundError, match="no face track \\("):
            arun.run_inference_file(engine_all, path, detections=nobody, tracks="all", **more)
        with pytest.raises(FileNotFoundError, match="no face track 00 \\(os.listdir\\(<faces>/00\\) fails in the reference, get_prob_video.py:79\\)$"):
            arun.run_inference_file(engine_all, path, detections=nobody, **more)
    same_top(run(engine_all, clip, mode=MODE_FP32), ref, "behind nobody")
    # heat maps stay with track 00
    with pytest.raises(ValueError, match="flag_heatmaps.*tracks|tracks.*flag_heatmaps"):
        run(engine_all, clip, tracks="all", flag_heatmaps=True)
    with pytest.raises(ValueError, match="flag_heatmaps.*tracks|tracks.*flag_heatmaps"):
        arun.run_inference_file(engine_all, path, detections=dets, tracks=[0], flag_heatmaps=True, stream_frames=16)
    same_top(run(engine_all, clip, mode=MODE_FP32), ref, "behind the refusal")
    same_call(run(engine_all, clip, tracks="all"), run(engine_all, clip, tracks="all"), "twice")
