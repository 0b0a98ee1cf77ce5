"""A set of unequal videos in packed passes (avcer_amd/dataset.py) against the per-video path, bit for bit: the segmented fusion
launch against `audio_frame_mean` + `fuse` per video, `run_dataset` against `run_inference` per video, and the failure paths."""
import os

import numpy as np
import pytest
import torch

from avcer_amd import run as arun
from avcer_amd import synth
from avcer_amd.dataset import VideoJob, run_dataset
from avcer_amd.engine import MODE_F16X3, MODE_FP32
from avcer_amd.fusion import WEIGHTS_AV_1, covered_frames
from test_face_cpu import golden_frames, golden_script

pytestmark = pytest.mark.gpu

# frames, (frame_lo, frame_hi) per window: spans do not decrease within a video, as chunk_spans yields them
VIDEOS = (
    (1, [(0, 2)]),                                                            # the span ends behind the video
    (2, [(0, 1), (0, 2), (1, 3)]),
    (9, [(0, 5), (2, 7), (4, 7)]),                                            # frames 7, 8 uncovered: the tail rule (n_aud = 7 < 9)
    (16, [(0, 8), (3, 11), (6, 14), (9, 17), (12, 17), (15, 17)]),            # window 2 is NaN; hi exceeds the frame count
    (40, [(a, min(a + 10, 41)) for a in range(0, 40, 4)]),                    # 68 frames in all: a second block of 64 threads
)
NAN_WINDOW = (3, 2)


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


def tables(c):
    n = sum(t for t, _ in VIDEOS)
    w = sum(len(s) for _, s in VIDEOS)
    e = np.exp(synth.centered(5, "ds_stat", (n, 7), 1.5))
    stat = (e / e.sum(1, keepdims=True)).astype(np.float32)
    dyn = synth.centered(5, "ds_dyn", (n, 7), 2.0).astype(np.float32)
    win = synth.centered(5, f"ds_win{c}", (w, c), 2.0).astype(np.float32)
    at = sum(len(s) for _, s in VIDEOS[:NAN_WINDOW[0]]) + NAN_WINDOW[1]
    win[at] = np.nan
    return torch.from_numpy(stat), torch.from_numpy(dyn), torch.from_numpy(win)


def same(a, b):
    """NaN positions by mask, everything else by equality."""
    a, b = a.cpu(), b.cpu()
    if a.is_floating_point():
        return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    return torch.equal(a, b)


@pytest.mark.parametrize("c", [7, 8])
@pytest.mark.parametrize("w1", [WEIGHTS_AV_1, None])
def test_fuse_videos_equals_the_per_video_pair(engine, c, w1):
    stat, dyn, win = tables(c)
    lo = np.array([a for _, s in VIDEOS for a, _ in s])
    hi = np.array([b for _, s in VIDEOS for _, b in s])
    fc, wc = [t for t, _ in VIDEOS], [len(s) for _, s in VIDEOS]
    w2 = (0.5, 1.25, 2.0)
    for cwt in (False, True):
        for cmask in (False, True):
            prob, am, mean, cnt = engine.fuse_videos(stat, dyn, win, lo, hi, fc, wc, w1, w2, cwt, cmask)
            assert tuple(prob.shape) == (4, sum(fc), 7) and tuple(am.shape) == (4, sum(fc)) and tuple(mean.shape) == (sum(fc), c)
            f = w = 0
            for t, spans in VIDEOS:
                l, h = lo[w:w + len(spans)], hi[w:w + len(spans)]
                m1, c1 = engine.audio_frame_mean(win[w:w + len(spans)], l, h, t)
                p1, a1 = engine.fuse(stat[f:f + t], dyn[f:f + t], m1, covered_frames(l, h, t), w1, w2, cwt, cmask)
                assert same(mean[f:f + t], m1) and same(cnt[f:f + t], c1), (t, cwt, cmask)
                assert same(prob[:, f:f + t], p1) and same(am[:, f:f + t], a1), (t, cwt, cmask)
                f, w = f + t, w + len(spans)
            if not cmask:  # (the Rule-1 mask turns a NaN probability into 0: NaN > 1/7 is false)
                assert torch.isnan(prob[:, 12 + 6:12 + 14]).any()  # the NaN window reached the frames it covers (video 3, frames 6..13)
    # without the optional outputs
    p2, a2, m2, c2 = engine.fuse_videos(stat, dyn, win, lo, hi, fc, wc, w1, w2, True, True, with_mean=False)
    assert m2 is None and c2 is None and same(p2, prob) and same(a2, am)


def test_fuse_videos_refuses_on_the_host(engine):
    stat, dyn, win = tables(8)
    lo = np.array([a for _, s in VIDEOS for a, _ in s])
    hi = np.array([b for _, s in VIDEOS for _, b in s])
    fc, wc = [t for t, _ in VIDEOS], [len(s) for _, s in VIDEOS]
    engine.x3_overflow_clear()
    good = engine.fuse_videos(stat, dyn, win, lo, hi, fc, wc, WEIGHTS_AV_1)
    bad_lo, bad_hi = lo.copy(), hi.copy()
    bad_lo[1:4], bad_hi[1:4] = 5, 7                                           # video 1 (2 frames): no window covers a frame
    with pytest.raises(IndexError, match="video 1"):
        engine.fuse_videos(stat, dyn, win, bad_lo, bad_hi, fc, wc, WEIGHTS_AV_1)
    with pytest.raises(IndexError, match="video b"):
        engine.fuse_videos(stat, dyn, win, bad_lo, bad_hi, fc, wc, WEIGHTS_AV_1, names=list("abcde"))
    gap_lo = lo.copy()
    gap_lo[4] = 1                                                             # video 2: frame 0 uncovered, 1..6 covered
    with pytest.raises(ValueError, match="video 2"):
        engine.fuse_videos(stat, dyn, win, gap_lo, hi, fc, wc, WEIGHTS_AV_1)
    with pytest.raises(ValueError):
        engine.fuse_videos(stat, dyn, win[:, :6], lo, hi, fc, wc, WEIGHTS_AV_1)
    assert engine.x3_overflow_count(reset=False) == 0
    again = engine.fuse_videos(stat, dyn, win, lo, hi, fc, wc, WEIGHTS_AV_1)
    assert all(same(a, b) for a, b in zip(again, good))


# ------------------------------------------------------------------------------------------------ run_dataset
def make_jobs():
    frames, script = golden_frames(), golden_script()
    total, sr = len(frames), 16000
    h, w = frames.shape[1:3]
    specs = (("full25", total, 25), ("short30", total - 5, 30), ("nine25", 9, 25))
    wavs = {
        "full25": synth.waveforms(99, 1, 8000 * 2)[0],                        # a multiple of 8000 samples: the empty NaN tail window
        "nine25": synth.waveforms(98, 1, int(9 / 25 * sr))[0],
    }
    pcm = synth.waveforms(97, 2, int((total - 5) / 30 * 44100))               # 44.1 kHz stereo int16, as it lies in the WAV file
    wavs["short30"] = np.ascontiguousarray(np.clip(np.round(pcm * 32768), -32768, 32767).astype(np.int16).T)
    jobs = []
    for name, t, fps in specs:
        wav_sr = 44100 if name == "short30" else None
        jobs.append(VideoJob(name, t, h, w, fps, len(wavs[name]), wav_sr=wav_sr, detections=script[:t],
                             load=lambda name=name, t=t: (frames[:t], wavs[name])))
    return jobs


KEYS = ("av", "vs", "vd", "a", "compound_prob", "static_probs", "dynamic_logits", "audio_rows", "audio_frames", "records")


def reference(engine, jobs, mode, path="", **kw):
    out = []
    for j in jobs:
        fr, wav = j.load()
        out.append(arun.run_inference(engine, fr, wav, j.fps, detections=j.detections, mode=mode, wav_sr=j.wav_sr,
                                      path_save_results=path, name_video=j.name, flag_save_prob=bool(path), **kw))
    return out


def assert_same_results(got, ref):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


@pytest.mark.parametrize("mode", [MODE_F16X3, MODE_FP32])
def test_run_dataset_equals_run_inference(engine_all, tmp_path, mode):
    jobs = make_jobs()
    ref = reference(engine_all, jobs, mode, str(tmp_path / "ref"))
    assert np.isnan(ref[0]["audio_rows"]).any()                               # the empty tail window is in the set
    cut = run_dataset(engine_all, jobs, mode=mode, max_frames_per_pass=7, max_windows_per_pass=3,
                      path_save_results=str(tmp_path / "cut"), flag_save_prob=True)
    assert max(cut.passes["static"]) <= 7 and len(cut.passes["static"]) > 1 and max(cut.passes["audio"]) <= 3
    assert cut.passes["static"][0] == 7                                       # 6 + 6 + 6 present tiles: the first pass ends inside video 2
    whole = run_dataset(engine_all, jobs, mode=mode)
    assert len(whole.passes["static"]) == 1 and len(whole.passes["audio"]) == 1
    for res in (cut, whole):
        assert [r["name"] for r in res] == [j.name for j in jobs] and res.real_time_factor > 0
        for got, want in zip(res, ref):
            assert_same_results(got, want)
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "ref") for d, _, fs in os.walk(tmp_path / "ref") for f in fs)
    assert len(files) == 9                                                    # static, dynamic and audio CSV per video
    for f in files:
        assert (tmp_path / "cut" / f).read_bytes() == (tmp_path / "ref" / f).read_bytes(), f
    # fusion settings reach the packed launch
    kw = dict(weights_prob_model=WEIGHTS_AV_1, weights_model=(0.5, 1, 2), ce_weights_type=False, ce_mask=True)
    for got, want in zip(run_dataset(engine_all, jobs, mode=mode, max_frames_per_pass=5, **kw), reference(engine_all, jobs, mode, **kw)):
        assert_same_results(got, want)


def test_run_dataset_failure_paths(engine_all):
    jobs = make_jobs()
    ref = run_dataset(engine_all, jobs, mode=MODE_F16X3)
    bad = list(jobs)
    j = jobs[1]
    bad[1] = VideoJob(j.name, j.n_frames, j.height, j.width, j.fps, j.n_samples, j.wav_sr, j.load,
                      [np.zeros((0, 15), np.float32)] * j.n_frames)
    with pytest.raises(FileNotFoundError, match="short30"):
        run_dataset(engine_all, bad, mode=MODE_F16X3)
    part = run_dataset(engine_all, bad, mode=MODE_F16X3, skip_failed=True)
    assert set(part[1]) == {"name", "error"} and isinstance(part[1]["error"], FileNotFoundError)
    for k in (0, 2):
        assert_same_results(part[k], ref[k])
    assert engine_all.x3_overflow_count(reset=False) == 0
    again = run_dataset(engine_all, jobs, mode=MODE_F16X3)
    for got, want in zip(again, ref):
        assert_same_results(got, want)
