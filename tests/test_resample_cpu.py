"""Host side of the audio resampler (avcer_amd/audio_pipeline.py: resample_plan, resample_out_len, load_wav) against a
restatement of torchaudio's sinc resampler.  No GPU.

`sinc_resample_kernel` / `apply_sinc_resample_kernel` below restate `_get_sinc_resample_kernel` and
`_apply_sinc_resample_kernel` of torchaudio 2.1.2 (torchaudio/functional/functional.py; BSD 2-Clause License, Copyright (c) 2017
Facebook Inc. (Soumith Chintala)) for the settings data/utils.py:55 uses: "sinc_interp_hann", lowpass_filter_width 6, rolloff
0.99.  torchaudio is not installed beside torch for ROCm: the restatement rests on its published source.  tests/test_gpu_resample.py
imports these helpers as its oracle."""
import math
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from avcer_amd import audio_pipeline as ap

RATE_PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (44100, 48000)]


def sinc_resample_kernel(orig_freq, new_freq, dtype=None, lowpass_filter_width=6, rolloff=0.99):
    """-> (kernel [n, 1, 2 * width + o], width, o, n).  dtype None: float32 taps out of a float64 sample term and a float32 phase
    term (what Resample builds by default); torch.float64: everything in float64."""
    gcd = math.gcd(int(orig_freq), int(new_freq))
    orig_freq, new_freq = int(orig_freq) // gcd, int(new_freq) // gcd
    base_freq = min(orig_freq, new_freq) * rolloff
    width = math.ceil(lowpass_filter_width * orig_freq / base_freq)
    idx_dtype = dtype if dtype is not None else torch.float64
    idx = torch.arange(-width, width + orig_freq, dtype=idx_dtype)[None, None] / orig_freq
    t = torch.arange(0, -new_freq, -1, dtype=dtype)[:, None, None] / new_freq + idx
    t *= base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base_freq / orig_freq
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    if dtype is None:
        kernels = kernels.to(dtype=torch.float32)
    return kernels, width, orig_freq, new_freq


def apply_sinc_resample_kernel(waveform, kernel, width, o, n):
    """waveform [L] in the kernel's dtype -> [ceil(n * L / o)]: pad, strided conv1d, interleave the phases, cut."""
    length = waveform.shape[-1]
    padded = F.pad(waveform.reshape(1, -1), (width, width + o))
    resampled = F.conv1d(padded[:, None], kernel, stride=o).transpose(1, 2).reshape(1, -1)
    return resampled[0, :math.ceil(n * length / o)]


def reference_mono(src):
    """What data/utils.py:50-52 holds in front of the transform: torchaudio.load's float32 [C, L] (int16 / 32768) and the
    channel mean when there is more than one.  src: int16 [L] / [L, C] or float32 [L] / [C, L] (numpy)."""
    src = np.asarray(src)
    if src.dtype == np.int16:
        wav = torch.from_numpy((src[:, None] if src.ndim == 1 else src).T.astype(np.float32)) / 32768
    else:
        wav = torch.from_numpy(src if src.ndim == 2 else src[None])
    return wav.mean(dim=0) if wav.size(0) > 1 else wav[0]


def reference_resample(mono, orig_freq, new_freq):
    """mono float32 [L] -> (what the reference computes: float32 conv1d; the oracle: the same float32 taps, float64 sums)."""
    if orig_freq == new_freq:
        return mono, mono.double()
    k, width, o, n = sinc_resample_kernel(orig_freq, new_freq)
    return apply_sinc_resample_kernel(mono, k, width, o, n), apply_sinc_resample_kernel(mono.double(), k.double(), width, o, n)


@pytest.mark.parametrize("orig,new", RATE_PAIRS)
def test_plan_scatters_back_to_the_dense_table_bit_for_bit(orig, new):
    k, width, o, n = sinc_resample_kernel(orig, new)
    dense = k[:, 0].numpy()
    plan = ap.resample_plan(orig, new)
    assert (plan.width, plan.o, plan.n) == (width, o, n)
    assert plan.taps.dtype == np.float32 and plan.taps.shape == (n, plan.span) and plan.first.shape == (n,)
    assert plan.first.min() >= 0 and (plan.first + plan.span).max() <= dense.shape[1]
    back = np.zeros_like(dense)
    cols = plan.first[:, None] + np.arange(plan.span)[None]
    back[np.arange(n)[:, None], cols] = plan.taps
    # bit for bit: every tap inside the span carries the dense table's bits (signed zeros too), and outside it the dense table
    # holds nothing but zeros -- of either sign: at the clamp the window is cos(pi / 2)^2 ~ 4e-33 and the float32 cast
    # underflows the product to +-0, which adds nothing to a sum
    assert plan.taps.tobytes() == np.ascontiguousarray(dense[np.arange(n)[:, None], cols]).tobytes()
    assert np.array_equal(back, dense) and back.view(np.uint32)[dense != 0].tobytes() == dense.view(np.uint32)[dense != 0].tobytes()
    outside = np.ones_like(dense, dtype=bool)
    outside[np.arange(n)[:, None], cols] = False
    assert (dense[outside] == 0).all()
    assert 1 <= plan.span <= ap.RESAMPLE_MAX_SPAN and o <= ap.RESAMPLE_MAX_O and n <= ap.RESAMPLE_MAX_N
    print(orig, new, "o", o, "n", n, "width", width, "dense taps", dense.shape[1], "span", plan.span)


def test_plan_spans_are_the_surveyed_ones():
    spans = {pair: ap.resample_plan(*pair).span for pair in RATE_PAIRS}
    assert spans[(44100, 16000)] == 34 and spans[(48000, 16000)] == 37 and spans[(22050, 16000)] == 17
    assert spans[(11025, 16000)] == 13 and spans[(8000, 16000)] == 13
    assert ap.resample_plan(11025, 16000).n == 640


def test_float32_phase_term_matters():
    """The detail resample_plan's docstring names: a float64 phase term gives other float32 taps.  The float32 phase p / n is off
    by up to 2^-24 relative, t = phase * base by up to 158 * 2^-24 = 9.4e-6, and |dk/dt| < 1 * base / o < 0.4: the taps differ by
    less than 4e-6.  resample_plan follows the float32 form (the bit-for-bit test above)."""
    k32 = sinc_resample_kernel(44100, 16000)[0]
    k64 = sinc_resample_kernel(44100, 16000, dtype=torch.float64)[0]
    assert (k32 != k64.float()).any() and (k32.double() - k64).abs().max() < 4e-6


@pytest.mark.parametrize("orig,new", RATE_PAIRS)
def test_compact_form_equals_dense_form(orig, new):
    """The kernel's index arithmetic in numpy: y[q n + p] = sum_j taps[p][j] * xpad[q o + first[p] + j] over the compact table
    equals the dense conv1d form (float64 both, summation order aside)."""
    plan = ap.resample_plan(orig, new)
    g = torch.Generator().manual_seed(orig + new)
    for length in (1, 5, plan.width - 1, plan.o, plan.o + 1, 3001):
        x = torch.rand(length, generator=g, dtype=torch.float64) * 2 - 1
        k, width, o, n = sinc_resample_kernel(orig, new)
        ref = apply_sinc_resample_kernel(x, k.double(), width, o, n).numpy()
        n_out = ap.resample_out_len(length, o, n)
        assert n_out == len(ref)
        xpad = np.pad(x.numpy(), (width, width + o + plan.span))
        m = np.arange(n_out)
        q, p = m // n, m % n
        got = np.zeros(n_out)
        for j in range(plan.span):
            got += plan.taps[p, j].astype(np.float64) * xpad[q * o + plan.first[p] + j]
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13)


def test_output_length_rule():
    plan = ap.resample_plan(44100, 16000)
    o, n, width = plan.o, plan.n, plan.width
    for length in (0, 1, width - 1, o, o + 1, 441000):
        assert ap.resample_out_len(length, o, n) == math.ceil(n * length / o)
        if length:
            assert ap.resample_out_len(length, o, n) == len(reference_resample(torch.zeros(length), 44100, 16000)[0])
    assert ap.resample_out_len(0, o, n) == 0 and ap.resample_out_len(1, o, n) == 1 and ap.resample_out_len(o, o, n) == n
    assert ap.resample_out_len(o + 1, o, n) == n + 1 and ap.resample_out_len(441000, o, n) == 160000
    hour = 3600 * 44100
    assert n * hour > 2 ** 31 and ap.resample_out_len(hour, o, n) == 3600 * 16000   # length only: 64-bit arithmetic
    assert ap.resample_out_len(hour + 1, o, n) == 3600 * 16000 + 1


def test_plan_refuses_what_the_kernel_does_not_cover():
    with pytest.raises(ValueError):
        ap.resample_plan(44100, 16001)      # coprime: o = 44100
    with pytest.raises(ValueError):
        ap.resample_plan(16000, 44101)      # n = 44101
    with pytest.raises(ValueError):
        ap.resample_plan(0, 16000)
    with pytest.raises(ValueError):
        ap.resample_plan(44100.0, 16000)
    with pytest.raises(ValueError):
        ap.resample_plan(1024000, 1000)     # o = 1024, but 12289 taps per phase


def _write_wav(path, pcm, rate, sampwidth=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(pcm.shape[1])
        f.setsampwidth(sampwidth)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


@pytest.mark.parametrize("channels", [1, 2])
def test_load_wav_round_trip(tmp_path, channels):
    rng = np.random.default_rng(channels)
    pcm = rng.integers(-32768, 32768, size=(1234, channels)).astype("<i2")
    pcm[0], pcm[1] = -32768, 32767
    _write_wav(tmp_path / "a.wav", pcm, 44100)
    got, rate = ap.load_wav(str(tmp_path / "a.wav"))
    assert rate == 44100 and got.dtype == np.int16 and got.shape == (1234, channels)
    np.testing.assert_array_equal(got, pcm)


def test_load_wav_refuses_other_sample_widths(tmp_path):
    _write_wav(tmp_path / "u8.wav", np.full((100, 1), 128, np.uint8), 16000, sampwidth=1)
    _write_wav(tmp_path / "s24.wav", np.zeros((100, 3), np.uint8), 16000, sampwidth=3)
    for name in ("u8.wav", "s24.wav"):
        with pytest.raises(ValueError):
            ap.load_wav(str(tmp_path / name))
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    with pytest.raises(ValueError):
        ap.load_wav(str(tmp_path / "junk.wav"))


def test_missing_wav_names_the_ffmpeg_command(tmp_path):
    with pytest.raises(FileNotFoundError, match="ffmpeg -i .*clip.mp4 -vn -acodec pcm_s16le -ar 44100 -ac 2"):
        ap.convert_mp4_to_mp3(None, str(tmp_path / "clip.mp4"))
    with pytest.raises(FileNotFoundError):
        ap.preprocess_audio_and_predict(None, str(tmp_path / "clip.mp4"))


@pytest.mark.parametrize("orig,new", RATE_PAIRS)
def test_restatement_agrees_with_upfirdn(orig, new):
    """Guards the oracle, not the product: the same taps laid out as ONE prototype filter and applied by
    scipy.signal.upfirdn (zero-stuff by n, filter, keep every o-th sample) give the conv1d form's output to float64 rounding.
    Tap k[p][j] sits at prototype index c + p * o - j * n (distinct for distinct (p, j): o and n are coprime), c a multiple of o."""
    from scipy.signal import upfirdn

    k, width, o, n = sinc_resample_kernel(orig, new)
    dense = k[:, 0].double().numpy()
    taps = dense.shape[1]
    c = o * math.ceil((taps - 1) * n / o)
    h = np.zeros(c + (n - 1) * o + 1)
    pos = c + np.arange(n)[:, None] * o - np.arange(taps)[None] * n
    assert len(np.unique(pos)) == pos.size
    h[pos] = dense
    x = torch.rand(2000 + o, generator=torch.Generator().manual_seed(7), dtype=torch.float64) * 2 - 1
    ref = apply_sinc_resample_kernel(x, k.double(), width, o, n).numpy()
    xpad = np.pad(x.numpy(), (width, width + o))
    out = upfirdn(h, xpad, up=n, down=o)
    got = out[c // o: c // o + len(ref)]
    assert len(got) == len(ref)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13)
