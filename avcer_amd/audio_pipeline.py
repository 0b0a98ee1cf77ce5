"""Batched counterpart of EmotionRecognition.load_audio_features (get_prob_audio_8_cl.py:68-138).

Index arithmetic (window starts, frame spans, Python banker's rounding) is restated on the host; sample conversion, downmix and
resampling of the source audio (data/utils.py:42-60), slicing, padding, normalisation and the model run on the GPU, the model in
one batch over all windows of a waveform.
"""
from __future__ import annotations

import functools
import math
import os
import wave
from typing import NamedTuple

import numpy as np
import torch

from .engine import Engine, MODE_DEFAULT

EMO_AUDIO_8 = ("Neutral", "Anger", "Disgust", "Fear", "Happiness", "Sadness", "Surprise", "Other")  # :114-123
MODEL_NAME = "FLW-ExprModelV3-2024.03.02-11.42.11"  # get_prob_audio_8_cl.py:155: the directory the audio CSV goes to

# limits of the resampling kernel (include/avcer_hip.h AVCER_RESAMPLE_MAX_*): reduced input / output period and taps per phase
RESAMPLE_MAX_O, RESAMPLE_MAX_N, RESAMPLE_MAX_SPAN = 2048, 1024, 128
LOWPASS_FILTER_WIDTH, ROLLOFF = 6, 0.99  # torchaudio.transforms.Resample's defaults, which data/utils.py:55 takes


class ResamplePlan(NamedTuple):
    """The compact tap table of one rate pair: dense tap k[p][first[p] + j] = taps[p][j], every other dense tap is exactly 0."""
    taps: np.ndarray   # float32 [n, span]
    first: np.ndarray  # int32 [n], first[p] + span <= 2 * width + o
    width: int
    o: int             # orig_freq / gcd: input samples per period
    n: int             # new_freq / gcd: output samples per period (= phases)

    @property
    def span(self) -> int:
        return int(self.taps.shape[1])


def resample_out_len(n_samples: int, o: int, n: int) -> int:
    """ceil(n * L / o) in Python integers (n * L passes 2^31 for an hour of audio)."""
    return (int(n) * int(n_samples) + int(o) - 1) // int(o)


@functools.lru_cache(maxsize=None, typed=True)
def resample_plan(orig_freq: int, new_freq: int) -> ResamplePlan:
    """The filter of torchaudio.transforms.Resample(orig_freq, new_freq) (Hann-windowed sinc, lowpass_filter_width 6, rolloff
    0.99), as include/avcer_hip.h avcer_resample defines it, reduced to its non-zero taps.  Pure host code.

    The table is computed with the torch operations and dtypes torchaudio 2.1.2's `_get_sinc_resample_kernel` uses when its
    `dtype` is None, because the float32 result depends on them: the sample term is float64, but the phase term
    `torch.arange(0, -n, -1) / n` is an int64 tensor divided by an int, i.e. float32.  With a float64 phase the output moves by
    5.9e-6 (44100 -> 16000) and 1.5e-5 (22050 -> 16000) at full-scale input.  torchaudio is not installed beside torch for ROCm,
    so this detail rests on reading its published source, not on running it.
    Raises ValueError for rates that are not positive integers or whose reduced pair is outside the kernel's limits."""
    for f in (orig_freq, new_freq):
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f <= 0:
            raise ValueError(f"resample: sample rates must be positive integers, got {orig_freq!r} -> {new_freq!r}")
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    if o > RESAMPLE_MAX_O or n > RESAMPLE_MAX_N:
        raise ValueError(f"resample {orig_freq} -> {new_freq}: the reduced pair {o} -> {n} is outside the kernel's range "
                         f"(<= {RESAMPLE_MAX_O} -> <= {RESAMPLE_MAX_N})")
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None] / o
    t = torch.arange(0, -n, -1)[:, None] / n + idx
    t *= base
    t = t.clamp_(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t *= math.pi
    k = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    k *= window * (base / o)
    dense = k.to(torch.float32).numpy()                      # [n, 2 * width + o]
    nz = dense != 0
    lo = nz.argmax(axis=1)                                   # every phase has a non-zero tap (its centre)
    hi = dense.shape[1] - nz[:, ::-1].argmax(axis=1)
    span = int((hi - lo).max())
    if span > RESAMPLE_MAX_SPAN:
        raise ValueError(f"resample {orig_freq} -> {new_freq}: {span} taps per phase, the kernel takes {RESAMPLE_MAX_SPAN}")
    first = np.minimum(lo, dense.shape[1] - span).astype(np.int32)
    taps = np.ascontiguousarray(dense[np.arange(n)[:, None], first[:, None] + np.arange(span)[None]])
    taps.setflags(write=False)
    first.setflags(write=False)
    return ResamplePlan(taps, first, int(width), o, n)


def load_wav(path: str):
    """A PCM s16 WAV file (what `ffmpeg -acodec pcm_s16le` writes, data/utils.py:46) -> (int16 [L, C] in frame order, sample
    rate), with the standard library's `wave`.  Any other sample format raises ValueError."""
    try:
        with wave.open(path, "rb") as f:
            if f.getsampwidth() != 2 or f.getcomptype() != "NONE":
                raise ValueError(f"{path}: {8 * f.getsampwidth()}-bit samples ({f.getcomptype()}); only PCM s16 is read")
            channels, rate, raw = f.getnchannels(), f.getframerate(), f.readframes(f.getnframes())
    except wave.Error as e:
        raise ValueError(f"{path}: not a PCM s16 WAV file ({e})") from None
    pcm = np.frombuffer(raw, dtype="<i2").astype(np.int16).reshape(-1, channels)
    return pcm, int(rate)


def _wav_path(path: str) -> str:
    path_save = path[:-3] + "wav"                            # data/utils.py:44
    if not os.path.exists(path_save):
        raise FileNotFoundError(f"{path_save} is missing; the reference writes it with "
                                f"`ffmpeg -i {path} -vn -acodec pcm_s16le -ar 44100 -ac 2 {path_save}` (data/utils.py:46)")
    return path_save


def convert_mp4_to_mp3(engine: Engine, path: str, sampling_rate: int = 16000) -> torch.Tensor:
    """data/utils.py:42-60 on its "the .wav already exists" branch: reads `path[:-3] + "wav"` and returns the mono waveform at
    `sampling_rate`, float32 [n] on the device (conversion, downmix and resampling in one launch, Engine.resample).  Running
    ffmpeg is not part of this build: a missing WAV raises FileNotFoundError naming the command."""
    pcm, sr = load_wav(_wav_path(path))
    return engine.resample(pcm, sr, sampling_rate)


def chunk_spans(n_samples: int, sr: int, fps: float, window: float, step: float):
    """get_prob_audio_8_cl.py:70-99.  Returns int arrays (start, end, frame_lo, frame_hi), one row per window;
    window i reports its logits for frames range(frame_lo[i], frame_hi[i])."""
    window_a = int(window * sr)
    step_a = int(step * sr)
    rows = []
    for start in range(0, n_samples + 1, step_a):
        end = min(start + window_a, n_samples)
        rows.append((start, end, round(start / sr * fps), round(end / sr * fps + 1)))
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def window_tokens(n_samples: int) -> int:
    """wav2vec2 tokens of a window of `n_samples` samples: the seven convolutions of its feature extractor (kernels 10, 3, 3, 3, 3,
    2, 2; strides 5, 2, 2, 2, 2, 2, 2; no padding), i.e. (n - 400) // 320 + 1 from 400 samples on.  0 below the receptive field."""
    n = int(n_samples)
    for k, s in ((10, 5), (3, 2), (3, 2), (3, 2), (3, 2), (2, 2), (2, 2)):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


def check_window(engine: Engine, window: float, sr: int) -> int:
    """The token count of a `window`-second window at `sr`, settled before any work: ValueError when it is more than the engine's
    loaded audio model accepts (Engine.load_audio(sd, max_tokens=...))."""
    tokens = window_tokens(int(window * sr))
    limit = engine.audio_max_tokens
    if tokens > limit:
        raise ValueError(f"window={window} s at {sr} Hz is {tokens} tokens, more than the loaded audio model's max_tokens={limit}: "
                         f"load it with Engine.load_audio(state_dict, max_tokens={tokens}) or more (at most 5000)")
    return tokens


def audio_forward(engine: Engine, wav: torch.Tensor, sr: int = 16000, fps: float = 25, window: float = 4,
                  step: float = 0.5, padding: str = "mean", mode: int = MODE_DEFAULT, wav_sr: int | None = None,
                  windows_per_pass: int | None = None):
    """wav f32 [L] (mono, already at `sr`); or, with `wav_sr` given, source audio at `wav_sr` as Engine.resample takes it (int16
    [L] / [L, C] or float32 [L] / [C, L]), brought to mono at `sr` on the device first (data/utils.py:50-57).
    Returns (window_logits [n_win, C], frame_lo [n_win], frame_hi [n_win]).
    An empty tail window (len(wav) % (step*sr) == 0) yields NaN logits, as in the reference ('mean' padding of an
    empty chunk is NaN, data/utils.py:76-82).
    `windows_per_pass`: the windows go through Engine.audio_chunks / Engine.audio_forward in groups of that many and the logits are
    concatenated -- the same logits, with the chunk buffer and the model's workspace those of a group (None: one call for all)."""
    if padding not in ("mean", "constant", "repeat"):
        raise ValueError(f"padding={padding!r}")
    if windows_per_pass is not None and (isinstance(windows_per_pass, bool) or not isinstance(windows_per_pass, (int, np.integer))
                                         or windows_per_pass < 1):
        raise ValueError(f"audio_windows_per_pass must be an integer >= 1, not {windows_per_pass!r}")
    check_window(engine, window, sr)
    wav = wav.reshape(-1) if wav_sr is None else engine.resample(wav, wav_sr, sr)
    starts, ends, lo, hi = chunk_spans(int(wav.numel()), sr, fps, window, step)
    if windows_per_pass is None or len(starts) <= windows_per_pass:
        chunks = engine.audio_chunks(wav, starts, ends, int(window * sr), padding)
        logits = engine.audio_forward(chunks, normalize=True, mode=mode)
        return logits, lo, hi
    parts = []
    for a in range(0, len(starts), int(windows_per_pass)):
        b = a + int(windows_per_pass)
        chunks = engine.audio_chunks(wav, starts[a:b], ends[a:b], int(window * sr), padding)
        parts.append(engine.audio_forward(chunks, normalize=True, mode=mode))
    return torch.cat(parts), lo, hi


def replicate_per_frame(logits: np.ndarray, lo, hi):
    """get_prob_audio_8_cl.py:94-101: the reference's DataFrame content (rows, frame index per row)."""
    rows, frames = [], []
    for lg, a, b in zip(logits, lo, hi):
        for f in range(int(a), int(b)):
            rows.append(lg)
            frames.append(f)
    if not rows:
        return np.zeros((0, logits.shape[1]), logits.dtype), np.zeros((0,), np.int64)
    return np.stack(rows), np.asarray(frames, dtype=np.int64)


def preprocess_audio_and_predict(engine: Engine, path_video: str = "", fps: float = 25, step: float = 0.5, padding: str = "mean",
                                 save_path: str = "src/pred_results/C-EXPR-DB", flag_save_prob: bool = False, window: float = 4,
                                 sr: int = 16000, mode: int = MODE_DEFAULT):
    """`get_prob_audio_8_cl.preprocess_audio_and_predict` (get_prob_audio_8_cl.py:141-172) with the reference's argument meaning,
    on the HIP path (the engine holds the audio weights): the WAV beside `path_video` in, the per-frame table out -- (rows float32
    [m, C], frame index int64 [m]), one row per (window, frame) pair as the reference's DataFrame holds them -- and
    `<save_path>/<MODEL_NAME>/<video>.csv` when `flag_save_prob`.  A missing WAV raises FileNotFoundError, a sample-rate pair the
    resampling kernel does not cover ValueError, a `window` of more tokens than the loaded model's max_tokens ValueError, all
    before anything is launched."""
    from . import io_formats

    path_wav = _wav_path(path_video)
    check_window(engine, window, sr)
    pcm, wav_sr = load_wav(path_wav)
    resample_plan(wav_sr, sr)
    src = torch.from_numpy(pcm)
    logits, lo, hi = engine.guarded(mode, lambda m: audio_forward(engine, src, sr, fps, window, step, padding, m, wav_sr=wav_sr))
    rows, frames = replicate_per_frame(logits.cpu().numpy(), lo, hi)
    if flag_save_prob:
        io_formats.write_audio_csv(rows, frames, save_path, MODEL_NAME, os.path.basename(path_video[:-4]))
    return rows, frames
