"""run_dataset(stream_frames=N): a set of recordings whose frames arrive in passes of N returns, bit for bit (NaN equal to NaN: the
empty-tail audio window), what the in-memory call of the same jobs returns -- every key of every video, the pass sizes, the files --
and holds one frame pass of one video instead of the whole clip.

The set: three AVI files written here, `five` (5 frames of 96 x 96, Motion-JPEG, 25 fps), `dib` (37 frames of 64 x 80, 24-bit bottom-up
DIB, 30 fps) and `talk` (70 frames of 96 x 96, Motion-JPEG, 25 fps; 3 s of sound for 2.8 s of video, so its last audio window is empty),
each with 44.1 kHz stereo PCM.  Face A is the first detection of a video, hence its track 00; the tracker never revives an id, so A
can be absent only from some frame to the end: in `talk` for the last 20 frames.  Face B comes (frame 10), is missed (18-20) and
goes (30), so the records change shape across pass borders.  5 + 37 + 50 = 92 tiles of track 00 with max_frames_per_pass=32: the
first static pass ends inside `dib` (and inside a frame pass), the second spans `dib` and `talk`."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from avcer_amd import avi, synth
from avcer_amd import face_tiles as ft
from avcer_amd import run as arun
from avcer_amd.dataset import VideoJob, run_dataset, video_job_from_avi
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine
from test_avi_cpu import jpeg_file, pcm_of

pytestmark = pytest.mark.gpu

KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")
SIZES = (1, 7, 16, 64, 1000)
NAMES = ("five", "dib", "talk")
SMALL = (64, 256)  # plot_size, as tests/test_gpu_chart_run.py


@pytest.fixture(scope="module")
def eng(sd_static, sd_dynamic, sd_audio):
    """An engine of this module's own (the session's keeps whatever detector other modules loaded), with every model loaded."""
    e = Engine(0)
    try:
        e.load_static(sd_static)
        e.load_dynamic(sd_dynamic)
        e.load_audio(sd_audio)
        yield e
    finally:
        e.close()


def faces(n, w, h, a_from=0, a_until=None, b=()):
    """Per-frame detections: face A on frames [a_from, a_until), face B on the frames `b`."""
    a_until = n if a_until is None else a_until
    out = []
    for t in range(n):
        rows = []
        if a_from <= t < a_until:
            rows.append([w // 16 + t % 3, h // 10, w // 2 + t % 3, 3 * h // 4, 0.99] + [0] * 10)
        if t in b:
            rows.append([w // 2 + 6, h // 8 + t % 2, w - 4, 5 * h // 8 + t % 2, 0.98] + [0] * 10)
        out.append(np.array(rows, dtype=np.float32).reshape(-1, 15))
    return out


B_TALK = tuple(t for t in range(10, 31) if t not in (18, 19, 20))


def script(talk_from=0, talk_until=50, talk_b=B_TALK, dib=True):
    return [faces(5, 96, 96), faces(37, 64, 80, a_until=37 if dib else 0, b=range(5, 21) if dib else ()),
            faces(70, 96, 96, talk_from, talk_until, talk_b)]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    root = tmp_path_factory.mktemp("set")
    mjpg = lambda n, seed: [jpeg_file(96, 96, seed + i, 2, quality=92) for i in range(n)]
    return [str(avi.write_avi(root / "five.avi", mjpg(5, 300), 25, 1, pcm_of(8820, 2, seed=5))),
            str(avi.write_avi_raw(root / "dib.avi", synth.video_frames(31, 37, 80, 64), 30, 1, pcm_of(54390, 2, seed=6))),
            str(avi.write_avi(root / "talk.avi", mjpg(70, 400), 25, 1, pcm_of(132300, 2, seed=7)))]


def jobs_of(eng, paths, dets):
    return [video_job_from_avi(p, detections=d, engine=eng) for p, d in zip(paths, dets)]


class Scripted:
    """A detector that answers from a script: the arrays of the frames it is shown, in the order the set shows them."""

    def __init__(self, dets):
        self.rows, self.at = [d for video in dets for d in video], 0

    def batch(self, frames, rgb=False):
        n = int(frames.shape[0])
        out, self.at = self.rows[self.at:self.at + n], self.at + n
        assert len(out) == n
        return out


def assert_same(got, ref, what=""):
    for key in KEYS:
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (what, key)
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{what} {key}")  # NaN equals NaN here


def assert_same_sets(got, ref, what=""):
    assert [g["name"] for g in got] == [r["name"] for r in ref] and got.passes == ref.passes, (what, got.passes, ref.passes)
    for g, r in zip(got, ref):
        assert set(g) == set(r), what
        if "error" not in r:
            assert_same(g, r, f"{what} {r['name']}")


def tree(root):
    out = {}
    for folder, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(folder, n), "rb") as f:
                out[os.path.relpath(os.path.join(folder, n), root)] = f.read()
    return out


# ---------------------------------------------------------------------------------------------------- 1, 2: bit identity
@pytest.mark.parametrize("mode", [MODE_F16X3, MODE_FP32])
def test_same_bits_for_every_pass_size(eng, paths, mode):
    jobs = jobs_of(eng, paths, script())
    ref = run_dataset(eng, jobs, mode=mode, max_frames_per_pass=32)
    assert [r["name"] for r in ref] == list(NAMES) and ref.passes["static"] == [32, 32, 28]
    assert np.isnan(ref[2]["audio_rows"]).any() and ref[2]["records"][:, 1].max() == 2
    assert not (ref[2]["records"][ref[2]["records"][:, 1] == 0][:, 0] >= 50).any()
    for n in SIZES:
        got = run_dataset(eng, jobs, mode=mode, max_frames_per_pass=32, stream_frames=n)
        assert_same_sets(got, ref, f"stream_frames={n}")
        assert got.real_time_factor > 0


def test_same_bits_as_the_single_file_path(eng, paths):
    dets = script()
    got = run_dataset(eng, jobs_of(eng, paths, dets), mode=MODE_F16X3, max_frames_per_pass=32, stream_frames=16)
    assert_same(got[2], arun.run_inference_file(eng, paths[2], detections=dets[2], mode=MODE_F16X3, stream_frames=16), "talk")


# ---------------------------------------------------------------------------------------------------- 3: a real detector
@pytest.fixture(scope="module")
def det(eng):
    return ft.RetinaFacePredictor(eng, synth.to_torch(synth.retina_mnet_state_dict(42)), threshold=0.9, mode=MODE_F16X3)


@pytest.fixture(scope="module")
def det_clip(tmp_path_factory):
    """24 frames of 192 x 256, the frames tests/test_gpu_detect_size.py streams the MobileNet-0.25 detector over, kept exact (DIB)."""
    frames = np.concatenate([synth.video_frames(13, 12, 192, 256)] * 2)
    return str(avi.write_avi_raw(tmp_path_factory.mktemp("det") / "seen.avi", frames, 25, 1, pcm_of(42336, 2, seed=8)))


@pytest.mark.parametrize("detect_size", [None, (96, 128)])
def test_a_real_detector_across_pass_boundaries(eng, det, det_clip, detect_size):
    jobs = [video_job_from_avi(det_clip, engine=eng)]
    ref = run_dataset(eng, jobs, det, mode=MODE_F16X3, detect_size=detect_size)
    assert len(ref[0]["records"]) > 0
    got = run_dataset(eng, jobs, det, mode=MODE_F16X3, detect_size=detect_size, stream_frames=8)
    assert_same_sets(got, ref, f"detect_size={detect_size}")


# ---------------------------------------------------------------------------------------------------- 4, 5: the track is known late
@pytest.mark.parametrize("how", ["given", "detector"])
def test_track_00_first_appears_in_a_late_pass(eng, paths, how):
    dets = script(talk_from=40, talk_until=70, talk_b=range(45, 61))          # nobody in front of frame 40: A is the first track there too
    jobs = jobs_of(eng, paths, dets if how == "given" else [None] * 3)
    ref = run_dataset(eng, jobs, Scripted(dets) if how == "detector" else None, mode=MODE_F16X3, max_frames_per_pass=32)
    r00 = ref[2]["records"][ref[2]["records"][:, 1] == 0]
    assert r00[0, 0] == 40 and len(r00) == 30
    got = run_dataset(eng, jobs, Scripted(dets) if how == "detector" else None, mode=MODE_F16X3, max_frames_per_pass=32, stream_frames=16)
    assert_same_sets(got, ref, how)


@pytest.mark.parametrize("how", ["given", "detector"])
def test_a_video_that_never_has_track_00(eng, paths, how):
    dets = script(dib=False)
    jobs = jobs_of(eng, paths, dets if how == "given" else [None] * 3)
    detector = lambda: Scripted(dets) if how == "detector" else None
    with pytest.raises(FileNotFoundError, match="dib") as want:
        run_dataset(eng, jobs, detector(), mode=MODE_F16X3)
    with pytest.raises(FileNotFoundError, match="dib") as got:
        run_dataset(eng, jobs, detector(), mode=MODE_F16X3, stream_frames=16)
    assert str(got.value) == str(want.value)
    ref = run_dataset(eng, jobs, detector(), mode=MODE_F16X3, skip_failed=True)
    part = run_dataset(eng, jobs, detector(), mode=MODE_F16X3, skip_failed=True, stream_frames=16)
    assert set(part[1]) == {"name", "error"} and isinstance(part[1]["error"], FileNotFoundError) and part[1]["name"] == "dib"
    assert_same_sets(part, ref, how)
    assert eng.x3_overflow_count(reset=False) == 0


# ---------------------------------------------------------------------------------------------------- 6: options
def test_options_ride_along(eng, paths, tmp_path):
    jobs = jobs_of(eng, paths, script())
    kw = dict(mode=MODE_F16X3, max_frames_per_pass=32, faces_via_jpeg=True, flag_save_prob=True, flag_save_plot_pred=True, plot_size=SMALL)
    ref = run_dataset(eng, jobs, path_save_results=str(tmp_path / "ref"), **kw)
    got = run_dataset(eng, jobs, path_save_results=str(tmp_path / "got"), stream_frames=16, **kw)
    for g, r in zip(got, ref):
        assert_same(g, r, r["name"])
        assert os.path.relpath(g["plot_pred"], tmp_path / "got") == os.path.relpath(r["plot_pred"], tmp_path / "ref")
    assert got.passes == ref.passes
    files = tree(tmp_path / "ref")
    assert sum(f.endswith(".csv") for f in files) == 9 and sum(f.endswith(".jpg") for f in files) == 3
    assert tree(tmp_path / "got") == files                                    # CSV files and charts, byte for byte
    plain = run_dataset(eng, jobs, mode=MODE_F16X3, max_frames_per_pass=32)
    assert not np.array_equal(plain[2]["static_probs"], ref[2]["static_probs"])  # the JPEG round trip was in the comparison


# ---------------------------------------------------------------------------------------------------- 7: the fp32 repeat
def test_overflow_repeats_the_streamed_set_in_fp32(eng, paths, sd_static):
    """The overflow input of tests/test_gpu_stream.py: a static model whose fc1 is scaled by 1e6 leaves fp16's range, engine.guarded
    repeats the set in fp32 -- every job is opened a second time, and the records are the first sweep's."""
    opened = []

    def counting(job):
        def open(per):
            opened.append(job.name)
            return job.open(per)
        return dataclasses.replace(job, open=open)

    jobs = [counting(j) for j in jobs_of(eng, paths, script())]
    armed = dict(sd_static)
    armed["fc1.weight"], armed["fc1.bias"] = sd_static["fc1.weight"] * 1.0e6, sd_static["fc1.bias"] * 1.0e6
    try:
        eng.load_static(armed)
        before = eng.x3_fallbacks
        ref = run_dataset(eng, jobs, mode=MODE_F16X3, max_frames_per_pass=32)
        assert eng.x3_fallbacks == before + 1 and opened == [], "the armed model must overflow fp16 in the in-memory call"
        got = run_dataset(eng, jobs, mode=MODE_F16X3, max_frames_per_pass=32, stream_frames=16)
        assert eng.x3_fallbacks == before + 2 and opened == list(NAMES) * 2
        assert_same_sets(got, ref, "armed")
        assert_same_sets(got, run_dataset(eng, jobs, mode=MODE_FP32, max_frames_per_pass=32), "fp32")
    finally:
        eng.load_static(sd_static)
    # with a detector the second sweep takes the first sweep's records: the detector is not asked again
    dets = script()
    seen = Scripted(dets)
    try:
        eng.load_static(armed)
        got2 = run_dataset(eng, jobs_of(eng, paths, [None] * 3), seen, mode=MODE_F16X3, max_frames_per_pass=32, stream_frames=16)
    finally:
        eng.load_static(sd_static)
    assert seen.at == 5 + 37 + 70
    assert_same_sets(got2, ref, "armed, detector")


# ---------------------------------------------------------------------------------------------------- 8: distributed, world size 1
def test_distributed_at_world_size_1(eng, paths):
    import socket

    import torch.distributed as dist

    jobs = jobs_of(eng, paths, script())
    ref = run_dataset(eng, jobs, mode=MODE_F16X3, max_frames_per_pass=32, stream_frames=16)
    mine = not dist.is_initialized()
    if mine:  # set up as tests/test_gpu_rccl.py sets it up
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        assert dist.get_world_size() == 1
        got = run_dataset(eng, jobs, mode=MODE_F16X3, max_frames_per_pass=32, stream_frames=16, distributed=True)
    finally:
        if mine:
            dist.destroy_process_group()
    assert_same_sets(got, ref, "distributed")


# ---------------------------------------------------------------------------------------------------- 9: memory
def test_the_streamed_call_holds_one_frame_pass_not_the_clip(eng, tmp_path):
    """96 frames of 256 x 256 (Motion-JPEG), one face per frame, stream_frames=8.  Peak device memory, measured as tools/stream_bench.py
    measures it (torch.cuda.max_memory_allocated around the call; the frames, tiles and tables are torch allocations, so the figure
    sees them -- the networks' workspace is the library's own and the same in both calls): the streamed call's peak is at most the
    in-memory call's minus the decoded clip, plus two frame passes."""
    n, h, w, per = 96, 256, 256, 8
    path = str(avi.write_avi(tmp_path / "wide.avi", [jpeg_file(w, h, 500 + i % 8, 2, quality=92) for i in range(n)], 25, 1,
                             pcm_of(44100 * n // 25, 2, seed=9)))
    jobs = [video_job_from_avi(path, detections=faces(n, w, h), engine=eng)]

    def peak(**kw):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = run_dataset(eng, jobs, mode=MODE_F16X3, **kw)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(), out

    peak(), peak(stream_frames=per)                                           # every cache of the engine is filled
    p_mem, ref = peak()
    p_stream, got = peak(stream_frames=per)
    assert_same_sets(got, ref)
    clip, one_pass = n * h * w * 3, per * h * w * 3
    print(f"peak bytes: in memory {p_mem}, streamed {p_stream}; clip {clip}, frame pass {one_pass}; allowed {p_mem - (clip - 2 * one_pass)}")
    assert p_stream <= p_mem - (clip - 2 * one_pass)


# ---------------------------------------------------------------------------------------------------- 10: refusals
def test_refusals_come_before_any_work(eng, paths):
    touched = []

    def never(*a):
        touched.append(a)
        raise AssertionError("a job was touched")

    dets = script()
    jobs = [dataclasses.replace(j, load=never, open=never) for j in jobs_of(eng, paths, dets)]
    eng.profile_enable(True)
    try:
        eng.profile_read_launches()
        for bad in (0, -3, 2.5, True, "64"):
            with pytest.raises(ValueError, match="stream_frames"):
                run_dataset(eng, jobs, mode=MODE_F16X3, stream_frames=bad)
        only_load = VideoJob("only_load", 5, 96, 96, 25, 8820, 44100, never, dets[0])
        with pytest.raises(ValueError, match="only_load"):
            run_dataset(eng, jobs + [only_load], mode=MODE_F16X3, stream_frames=8)
        assert eng.profile_read_launches() == [] and touched == []
    finally:
        eng.profile_enable(False)


def test_what_open_hands_out_is_held_to_the_metadata(eng, paths):
    dets = script()
    good = jobs_of(eng, paths, dets)
    ref = run_dataset(eng, good, mode=MODE_F16X3, stream_frames=8)

    def wrong(job, cut):
        def open(per):
            batches, wav = job.open(per * 2 if cut is None else per)
            return (b if cut is None else b[:cut] for b in batches), wav
        return dataclasses.replace(job, open=open)

    for cut, what in ((None, "a batch larger than asked"), (7, "fewer frames than the job says")):
        with pytest.raises(ValueError, match="dib"):
            run_dataset(eng, [good[0], wrong(good[1], cut), good[2]], mode=MODE_F16X3, stream_frames=8)
    assert eng.x3_overflow_count(reset=False) == 0
    assert_same_sets(run_dataset(eng, good, mode=MODE_F16X3, stream_frames=8), ref, "after the refusals")  # nothing was left queued
    # host arrays are taken as load() may return them
    def on_host(job):
        def open(per):
            batches, wav = job.open(per)
            return (b.cpu().numpy() for b in batches), wav
        return dataclasses.replace(job, open=open)

    host = [on_host(j) for j in good]
    assert_same_sets(run_dataset(eng, host, mode=MODE_F16X3, stream_frames=8), ref, "host arrays")
