"""GPU parity of the audio resampler (csrc/resample.hip through Engine.resample) and of the entries built on it against the
restatement of torchaudio's resampler in tests/test_resample_cpu.py.

Tolerance of the kernel tests: nothing is fixed here.  The oracle is the restatement's float32 taps summed in float64; e_ref is
the error of the restatement run in float32 (F.conv1d, what the reference executes) against that oracle ON THE SAME INPUT, and
the GPU's error must stay within 4 * e_ref (a different summation order over <= 37 terms).  Every figure is printed before it
is asserted."""
import os
import wave

import numpy as np
import pytest
import torch

from avcer_amd import audio_pipeline as ap
from avcer_amd import io_formats
from avcer_amd import run as arun
from avcer_amd.engine import MODE_F16X3, MODE_FP32
from avcer_amd.fusion import WEIGHTS_AV_1
from test_face_cpu import golden_frames, golden_script
from test_resample_cpu import RATE_PAIRS, reference_mono, reference_resample

pytestmark = pytest.mark.gpu

LENGTHS = (0, 5, 300, 44100 * 7 + 123)
SIGNALS = ("noise", "sine1k", "sine7k9")


def make_source(signal, rate, length, channels, dtype, seed=0):
    """int16 [L] / [L, C] (WAV frame order) or float32 [L] / [C, L]; the channels differ (phase and level, or independent noise)."""
    rng = np.random.default_rng([seed, rate, length, channels])
    if signal == "noise":                                          # white, full scale
        x = rng.integers(-32768, 32768, size=(channels, length)).astype(np.float64) / 32768
    elif signal == "zeros":
        x = np.zeros((channels, length))
    else:
        f = {"sine1k": 1000.0, "sine7k9": 7900.0}[signal]          # 7.9 kHz: just under the 16 kHz output's cut-off
        t = np.arange(length) / rate
        x = np.stack([np.sin(2 * np.pi * f * t + 0.7 * c) * (0.999 - 0.1 * c) for c in range(channels)]).reshape(channels, length)
    if dtype == "int16":
        pcm = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16).T
        return np.ascontiguousarray(pcm[:, 0] if channels == 1 and seed % 2 else pcm)
    x = x.astype(np.float32)
    return np.ascontiguousarray(x[0] if channels == 1 else x)


def check_against_oracle(engine, src, orig, new, tag):
    mono = reference_mono(src)
    ref32, oracle = reference_resample(mono, orig, new)
    got = engine.resample(src, orig, new)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == tuple(oracle.shape), (tag, got.shape, oracle.shape)
    if oracle.numel() == 0:
        return 0.0, 0.0
    e_ref = (ref32.double() - oracle).abs().max().item()
    e_gpu = (got.cpu().double() - oracle).abs().max().item()
    print(f"{tag}: n_out {oracle.numel()} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} max|y| {oracle.abs().max().item():.3g}")
    assert e_gpu <= 4 * e_ref, (tag, e_gpu, e_ref)
    return e_gpu, e_ref


@pytest.mark.parametrize("orig,new", RATE_PAIRS)
def test_kernel_matches_the_oracle(engine, orig, new):
    worst = (0.0, 0.0)
    for channels in (1, 2):
        for dtype in ("int16", "float32"):
            for length in LENGTHS:
                for i, signal in enumerate(SIGNALS):
                    src = make_source(signal, orig, length, channels, dtype, seed=i)
                    tag = f"{orig}->{new} C{channels} {dtype} L{length} {signal}"
                    worst = max(worst, check_against_oracle(engine, src, orig, new, tag))
    print(f"{orig}->{new}: worst e_gpu {worst[0]:.3e} (its e_ref {worst[1]:.3e})")


@pytest.mark.parametrize("orig,new", RATE_PAIRS)
def test_zero_input_and_empty_input_are_exact(engine, orig, new):
    plan = ap.resample_plan(orig, new)
    for channels, dtype in ((1, "int16"), (2, "int16"), (1, "float32"), (2, "float32")):
        src = make_source("zeros", orig, 300, channels, dtype)
        got = engine.resample(src, orig, new).cpu()
        assert got.numel() == ap.resample_out_len(300, plan.o, plan.n) and torch.equal(got, torch.zeros_like(got))
        empty = engine.resample(make_source("zeros", orig, 0, channels, dtype), orig, new)
        assert tuple(empty.shape) == (0,) and empty.dtype == torch.float32 and empty.is_cuda


def test_short_and_boundary_lengths(engine):
    """L < width, L = o, L = o + 1 and a length whose last block is partial, at the reference's own rate pair."""
    plan = ap.resample_plan(44100, 16000)
    for length in (1, plan.width - 1, plan.o, plan.o + 1, plan.o * 16, plan.o * 16 + 1, plan.o * 33 - 7):
        src = make_source("noise", 44100, length, 2, "int16", seed=length)
        check_against_oracle(engine, src, 44100, 16000, f"44100->16000 L{length}")


def test_equal_rates_convert_and_downmix_bit_exactly(engine):
    for channels, dtype in ((1, "int16"), (2, "int16"), (2, "float32"), (1, "float32")):
        for seed in (0, 1):                                        # seed 1: int16 mono as [L] instead of [L, 1]
            src = make_source("noise", 16000, 12345, channels, dtype, seed=seed)
            got = engine.resample(src, 16000, 16000).cpu()
            assert torch.equal(got, reference_mono(src)), (channels, dtype)
    src = make_source("noise", 16000, 4097, 6, "int16")            # int16 sums are exact in f32, the division rounds once
    np.testing.assert_allclose(engine.resample(src, 16000, 16000).cpu().numpy(), reference_mono(src).numpy(), rtol=0, atol=2.0 ** -24)


def test_six_channel_float_input(engine):
    for orig, new in ((44100, 16000), (48000, 16000)):
        src = make_source("noise", orig, 44100 * 2 + 11, 6, "float32", seed=6)
        check_against_oracle(engine, src, orig, new, f"{orig}->{new} C6 float32")


def test_determinism_and_table_cache(engine):
    src = make_source("noise", 44100, 44100 * 3 + 17, 2, "int16", seed=3)
    a = engine.resample(src, 44100, 16000).cpu()
    b = engine.resample(src, 44100, 16000).cpu()
    assert torch.equal(a, b)
    other = make_source("noise", 22050, 22050, 1, "float32", seed=4)
    engine.resample(other, 22050, 16000)
    engine.resample(other, 48000, 16000)
    c = engine.resample(src, 44100, 16000).cpu()
    assert torch.equal(a, c)
    assert {(44100, 16000), (22050, 16000), (48000, 16000)} <= set(engine._resample_cache)
    fresh = type(engine)(0)
    try:
        assert torch.equal(fresh.resample(src, 44100, 16000).cpu(), a)   # alone on a new engine: same bits
    finally:
        fresh.close()


def test_bad_sources_and_rates_raise_before_any_launch(engine):
    good = make_source("noise", 44100, 1000, 2, "int16")
    with pytest.raises(ValueError):
        engine.resample(good, 44100, 16001)                        # coprime rates: outside the kernel's limits
    with pytest.raises(ValueError):
        engine.resample(good.astype(np.int32), 44100, 16000)
    with pytest.raises(ValueError):
        engine.resample(np.zeros((1000, 9), np.int16), 44100, 16000)
    with pytest.raises(ValueError):
        engine.resample(np.zeros((2, 3, 4), np.float32), 44100, 16000)
    with pytest.raises(ValueError):
        engine.resample(good, 0, 16000)
    assert (44100, 16001) not in engine._resample_cache


@pytest.mark.parametrize("mode", [MODE_FP32, MODE_F16X3])
def test_audio_forward_from_source_audio(engine_audio, mode):
    """audio_forward(wav_sr=44100) on stereo int16 against audio_forward on the restatement's 16 kHz waveform: same windows, same
    frame spans, logits within 1e-4 (what tests/test_gpu_audio.py asks of the logits in both modes).  88200 source samples give
    32000 at 16 kHz = 4 steps of 0.5 s exactly: the empty tail window and its NaN row survive the new front end."""
    for length in (88200, 100000):
        src = make_source("noise", 44100, length, 2, "int16", seed=length)
        src[:] = (src.astype(np.float64) * 0.3).astype(np.int16)
        ref16 = reference_resample(reference_mono(src), 44100, 16000)[0]
        got, lo, hi = ap.audio_forward(engine_audio, torch.from_numpy(src), 16000, 25, window=2, step=0.5, padding="mean", mode=mode,
                                       wav_sr=44100)
        ref, rlo, rhi = ap.audio_forward(engine_audio, ref16, 16000, 25, window=2, step=0.5, padding="mean", mode=mode)
        assert got.shape == ref.shape
        np.testing.assert_array_equal(lo, rlo)
        np.testing.assert_array_equal(hi, rhi)
        got, ref = got.cpu(), ref.cpu()
        nan = torch.isnan(ref).any(dim=1)
        assert torch.equal(nan, torch.isnan(got).any(dim=1))
        if length == 88200:
            assert len(ref16) % 8000 == 0 and nan[-1] and not nan[:-1].any()
        d = (got[~nan] - ref[~nan]).abs().max().item()
        print(f"mode {mode} L{length}: {len(ref)} windows, max|dlogit| {d:.3e}")
        assert d < 1e-4


@pytest.fixture(scope="module")
def engine_all(engine, sd_static, sd_dynamic, sd_audio):
    engine.load_static(sd_static)
    engine.load_dynamic(sd_dynamic)
    engine.load_audio(sd_audio)
    return engine


@pytest.mark.parametrize("mode,tol", [(MODE_FP32, 1e-4), (MODE_F16X3, 1e-4)])
def test_run_inference_from_source_audio(engine_all, mode, tol):
    """run_inference(wav=<stereo int16>, wav_sr=44100) against run_inference with the restatement's 16 kHz mono waveform, with the
    assertions of tests/test_gpu_run.py::test_run_inference_matches_oracle_chain."""
    from oracle import fusion as ofu

    frames, script = golden_frames(), golden_script()
    total, fps = len(frames), 25
    src = make_source("noise", 44100, int(total / fps * 44100), 2, "int16", seed=99)
    src[:] = (src.astype(np.float64) * 0.3).astype(np.int16)
    ref16 = reference_resample(reference_mono(src), 44100, 16000)[0].numpy()
    kw = dict(detections=script, weights_prob_model=WEIGHTS_AV_1, ce_weights_type=False, ce_mask=True, mode=mode)
    out = arun.run_inference(engine_all, frames, src, fps, wav_sr=44100, **kw)
    ref = arun.run_inference(engine_all, frames, ref16, fps, **kw)
    np.testing.assert_array_equal(out["records"], ref["records"])
    assert np.abs(out["static_probs"] - ref["static_probs"]).max() < tol
    assert np.abs(ofu.softmax(out["dynamic_logits"]) - ofu.softmax(ref["dynamic_logits"])).max() < tol
    np.testing.assert_array_equal(out["audio_frames"], ref["audio_frames"])
    ok = ~np.isnan(ref["audio_rows"]).any(axis=1)
    assert np.array_equal(ok, ~np.isnan(out["audio_rows"]).any(axis=1))
    d_a = np.abs(ofu.softmax(out["audio_rows"][ok][:, :7]) - ofu.softmax(ref["audio_rows"][ok][:, :7])).max()
    d_c = np.abs(out["compound_prob"] - ref["compound_prob"]).max()
    print(f"mode {mode}: audio max|dprob| {d_a:.3e}, compound max|dprob| {d_c:.3e}")
    assert d_a < tol and d_c < tol
    for name in ("av", "vs", "vd", "a"):
        np.testing.assert_array_equal(out[name], ref[name])
    with pytest.raises(ValueError):
        arun.run_inference(engine_all, frames, src, fps, wav_sr=44101, **kw)


def test_file_level_mirror(engine_audio, tmp_path):
    src = make_source("sine1k", 44100, 3 * 44100, 2, "int16")
    src[:] = src // 2 + make_source("noise", 44100, 3 * 44100, 2, "int16") // 8
    video = str(tmp_path / "clip_y.mp4")
    with pytest.raises(FileNotFoundError, match="ffmpeg"):
        ap.preprocess_audio_and_predict(engine_audio, video, fps=25)
    with wave.open(video[:-3] + "wav", "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(44100)
        f.writeframes(src.astype("<i2").tobytes())
    rows, frames = ap.preprocess_audio_and_predict(engine_audio, video, fps=25, step=0.5, padding="mean", save_path=str(tmp_path),
                                                   flag_save_prob=True, window=2, sr=16000)
    logits, lo, hi = ap.audio_forward(engine_audio, torch.from_numpy(src), 16000, 25, window=2, step=0.5, padding="mean", wav_sr=44100)
    ref_rows, ref_frames = ap.replicate_per_frame(logits.cpu().numpy(), lo, hi)
    np.testing.assert_array_equal(frames, ref_frames)
    np.testing.assert_array_equal(rows, ref_rows)                  # same samples, same launches: same bits (NaN tail included)
    assert np.isnan(rows[-1]).all()                                # 3 s = 6 steps exactly: the empty tail window
    wav16 = ap.convert_mp4_to_mp3(engine_audio, video, 16000)
    assert torch.equal(wav16, engine_audio.resample(src, 44100, 16000)) and wav16.numel() == 48000
    csv = os.path.join(str(tmp_path), ap.MODEL_NAME, "clip_y.csv")
    assert os.path.exists(csv)
    c_rows, c_frames = io_formats.read_audio_csv(csv)              # drops the NaN rows, as get_pred_av.py does
    ok = ~np.isnan(rows).any(axis=1)
    np.testing.assert_array_equal(c_frames, frames[ok])
    np.testing.assert_allclose(c_rows, rows[ok], rtol=1e-6, atol=0)
    # a WAV at a rate the kernel does not cover: refused before anything is launched
    other = str(tmp_path / "odd.mp4")
    with wave.open(other[:-3] + "wav", "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(44101)
        f.writeframes(src[:1000, 0].astype("<i2").tobytes())
    with pytest.raises(ValueError):
        ap.preprocess_audio_and_predict(engine_audio, other, fps=25)
