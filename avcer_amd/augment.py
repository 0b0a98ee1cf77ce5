"""The waveform augmentations of the reference's training windows on the device: the `AUGMENTATION=True` half of
src/audio/train_c_audio.py:112-119, RandomChoice([PolarityInversion(), WhiteNoise(), Gain()]) of
src/audio/augmentation/wave_augmentation.py, applied to the padded window in front of the processor's normalisation.

    philox4x32 / normal_stream   the generator of the noise and its Box-Muller values: the CPU statement of what the kernel draws
    AugmentSpec                  the recipe: which transforms, their ranges, the seed
    draw_plan                    per window which transform and its numbers, drawn on the host from (seed, the window's global index)
    augment_numpy                the statement of avcer_wave_augment (include/avcer_hip.h) in numpy
    augment                      the device call (Engine.wave_augment, csrc/augment.hip), in place

Where this departs from the reference, on purpose: the reference draws from Python's `random` and `np.random` afresh every time a
sample is dealt, so no two epochs and no two runs see the same noise.  Here the draws are a function of (seed, window index): a
view of the corpus can be named, repeated and extracted once (head_fit.augmented_views).  The random draws of the plan are numpy's
(Generator(PCG64)), the noise samples are Philox4x32-10's -- neither is the stream `random.choice`, `random.uniform` and
`np.random.normal` would give under some seed.  The reference's own noise can be fed through (`noise=`) and compared at tolerance
zero (tests/test_augment_cpu.py).

Not covered, by name: SoxEffect (wave_augmentation.py:56-81) needs libsox; ResampleAudio (:135-161) is Engine.resample -- a file
given to audio_corpus.run_corpus as (name, wav, wav_sr) goes through it."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

KIND_NONE, KIND_POLARITY, KIND_NOISE, KIND_GAIN = 0, 1, 2, 3    # include/avcer_hip.h AVCER_AUGMENT_*
CHOICES = {"polarity": KIND_POLARITY, "noise": KIND_NOISE, "gain": KIND_GAIN}
REC = np.dtype([("kind", "<i4"), ("ratio", "<f4"), ("u", "<f8"), ("key", "<u8")])   # struct avcer_augment_rec
MAX_WIN = 2 ** 31 - 1    # AVCER_AUGMENT_MAX_WIN

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the generator
def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter [..., 4] and key
    [..., 2] 32-bit words (broadcast against each other) -> uint32 [..., 4].  Integers throughout: exact."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    if c.shape[-1] != 4 or k.shape[-1] != 2:
        raise ValueError(f"philox4x32: counter [..., 4] and key [..., 2] expected, got {c.shape} and {k.shape}")
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], lead).copy() for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], lead).copy() for j in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2    # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def normal_stream(key: int, count: int, first: int = 0) -> np.ndarray:
    """The normal values z[first : first + count] of the window whose 64-bit Philox key is `key`, float32: z[i] is lane i % 4 of
    philox4x32 at counter (i // 4, 0) -- low word, high word, 0, 0 -- under (key & 0xffffffff, key >> 32); lanes (0, 1) and (2, 3)
    are Box-Muller pairs: with words a, b  u1 = ((a >> 8) + 1) * 2^-24, u2 = (b >> 8) * 2^-24, r = sqrt(-2 log u1),
    z = r cos(2 pi u2), r sin(2 pi u2).  The integers are exact; log, sqrt, cos and sin are float64 here and the result is rounded
    to float32 once, where the kernel uses logf, sqrtf, cospif and sinpif."""
    key, count, first = int(key), int(count), int(first)
    if not 0 <= key < 2 ** 64 or count < 0 or first < 0:
        raise ValueError(f"normal_stream: a key in [0, 2^64), count >= 0 and first >= 0 expected, got {key}, {count}, {first}")
    q0, q1 = first // 4, -(-(first + count) // 4)
    q = np.arange(q0, q1, dtype=np.uint64)
    ctr = np.stack([q & _MASK, q >> np.uint64(32), np.zeros_like(q), np.zeros_like(q)], axis=-1)
    words = philox4x32(ctr, np.asarray([key & 0xFFFFFFFF, key >> 32], dtype=np.uint64)).reshape(-1, 2, 2)
    u1 = ((words[..., 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    t = (words[..., 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -23     # 2 * u2
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(np.pi * t), r * np.sin(np.pi * t)], axis=-1).reshape(-1)
    return z[first - 4 * q0:first - 4 * q0 + count].astype(np.float32)


# ------------------------------------------------------------------------------------------------ the recipe and its draws
def _finite(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(float(v))


@dataclass(frozen=True)
class AugmentSpec:
    """RandomChoice over `choices` ("polarity", "noise", "gain") with WhiteNoise(min_snr, max_snr) and Gain(min_gain, max_gain) of
    the reference, and the seed of the draws.  ValueError at construction: a choice that is not one of the three ("sox" and
    "resample" are refused by name), no choice, a bound that is not finite, min > max, a seed that is no integer >= 0."""
    seed: int
    choices: tuple = ("polarity", "noise", "gain")
    min_snr: float = 1e-4
    max_snr: float = 5e-3
    min_gain: float = -20.0
    max_gain: float = -1.0

    def __post_init__(self):
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or self.seed < 0:
            raise ValueError(f"AugmentSpec: seed must be an integer >= 0, got {self.seed!r}")
        if isinstance(self.choices, str) or not len(tuple(self.choices)):
            raise ValueError(f"AugmentSpec: choices is a non-empty sequence of {sorted(CHOICES)}, got {self.choices!r}")
        object.__setattr__(self, "choices", tuple(self.choices))
        for name in self.choices:
            low = name.lower() if isinstance(name, str) else name
            if low in ("sox", "soxeffect"):
                raise ValueError("AugmentSpec: SoxEffect needs libsox, which this project does not have")
            if low in ("resample", "resampleaudio"):
                raise ValueError("AugmentSpec: ResampleAudio is Engine.resample: give the file as (name, wav, wav_sr)")
            if name not in CHOICES:
                raise ValueError(f"AugmentSpec: choice {name!r}: one of {sorted(CHOICES)}")
        for lo, hi in (("min_snr", "max_snr"), ("min_gain", "max_gain")):
            a, b = getattr(self, lo), getattr(self, hi)
            if not _finite(a) or not _finite(b):
                raise ValueError(f"AugmentSpec: {lo} and {hi} must be finite numbers, got {a!r} and {b!r}")
            if a > b:
                raise ValueError(f"AugmentSpec: {lo}={a!r} is above {hi}={b!r}")


class Plan(NamedTuple):
    """Per window: kind int32 [n] (0 none, 1 polarity, 2 noise, 3 gain), u f64 [n] (WhiteNoise's uniform draw in [0, 1)), gain_db
    f64 [n], ratio32 f32 [n] (10 ** (gain_db / 20), what F.gain multiplies by), key uint64 [n] (the Philox key of the window's
    noise); min_snr, max_snr: WhiteNoise's range."""
    kind: np.ndarray
    u: np.ndarray
    gain_db: np.ndarray
    ratio32: np.ndarray
    key: np.ndarray
    min_snr: float = 1e-4
    max_snr: float = 5e-3

    def __len__(self) -> int:
        return int(self.kind.shape[0])

    def rows(self, a: int, b: int) -> "Plan":
        return Plan(self.kind[a:b], self.u[a:b], self.gain_db[a:b], self.ratio32[a:b], self.key[a:b], self.min_snr, self.max_snr)

    def records(self) -> np.ndarray:
        """The plan as avcer_augment_rec records."""
        rec = np.zeros(len(self), dtype=REC)
        rec["kind"], rec["ratio"], rec["u"], rec["key"] = self.kind, self.ratio32, self.u, self.key
        return rec


def make_plan(kind, u=None, gain_db=None, key=None, min_snr: float = 1e-4, max_snr: float = 5e-3) -> Plan:
    """A plan from given numbers (whoever has the reference's draws can pass them): kind [n] in 0 .. 3, u [n] in [0, 1), gain_db
    [n], key [n] in [0, 2^64); what is left out is 0.  ValueError: lengths that differ, a value out of range, min_snr > max_snr."""
    kind = np.asarray(kind).reshape(-1)
    n = kind.shape[0]
    if n and (not np.issubdtype(kind.dtype, np.integer) or kind.min() < KIND_NONE or kind.max() > KIND_GAIN):
        raise ValueError("make_plan: kind holds integers in 0 .. 3 (none, polarity, noise, gain)")
    u = np.zeros(n) if u is None else np.asarray(u, dtype=np.float64).reshape(-1)
    gain_db = np.zeros(n) if gain_db is None else np.asarray(gain_db, dtype=np.float64).reshape(-1)
    key = np.zeros(n, np.uint64) if key is None else np.asarray(key, dtype=np.uint64).reshape(-1)
    if u.shape[0] != n or gain_db.shape[0] != n or key.shape[0] != n:
        raise ValueError(f"make_plan: {n} kinds, {u.shape[0]} u, {gain_db.shape[0]} gains and {key.shape[0]} keys")
    if not ((u >= 0.0) & (u < 1.0)).all() or not np.isfinite(gain_db).all():
        raise ValueError("make_plan: u lies in [0, 1) and gain_db is finite")
    if not _finite(min_snr) or not _finite(max_snr) or min_snr > max_snr:
        raise ValueError(f"make_plan: min_snr <= max_snr, both finite, expected, got {min_snr!r} and {max_snr!r}")
    ratio = np.asarray([np.float32(10 ** (g / 20)) for g in gain_db.tolist()], dtype=np.float32)   # F.gain's Python arithmetic
    return Plan(kind.astype(np.int32), u, gain_db, ratio, key, float(min_snr), float(max_snr))


def draw_plan(spec: AugmentSpec, n: int, first: int = 0) -> Plan:
    """The records of the windows first .. first + n - 1 of a corpus under `spec`.  Window g draws from its own numpy
    Generator(PCG64(SeedSequence([spec.seed, g]))), in this order whatever its kind: the choice (integers(len(choices))), WhiteNoise's
    uniform, Gain's uniform (gain_db = min_gain + (max_gain - min_gain) * it, random.uniform spelled out) and the 64-bit Philox key.
    So window g has the same record in every call that covers it."""
    if not isinstance(spec, AugmentSpec):
        raise ValueError(f"draw_plan: an AugmentSpec expected, got {type(spec).__name__}")
    for name, v in (("n", n), ("first", first)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"draw_plan: {name} must be an integer >= 0, got {v!r}")
    codes = [CHOICES[c] for c in spec.choices]
    kind, u, gain, key = np.zeros(n, np.int32), np.zeros(n), np.zeros(n), np.zeros(n, np.uint64)
    for i in range(int(n)):
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(spec.seed), int(first) + i])))
        kind[i] = codes[int(rng.integers(len(codes)))]
        u[i] = rng.random()
        gain[i] = spec.min_gain + (spec.max_gain - spec.min_gain) * rng.random()
        key[i] = rng.integers(0, 2 ** 64, dtype=np.uint64)
    return make_plan(kind, u, gain, key, spec.min_snr, spec.max_snr)


# ------------------------------------------------------------------------------------------------ the statement
def std32_numpy(x) -> np.float32:
    """torch.std of one window (unbiased, over every sample) as the kernel takes it: float64 sums, one rounding to float32.  The
    kernel adds in its own fixed order (include/avcer_hip.h); in float64 the orders differ far below a float32 ulp."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = x - x.sum() / x.shape[0]
        return np.float32(np.sqrt(np.float64((d * d).sum()) / np.float64(x.shape[0] - 1)))


def noise_std_numpy(std32, u: float, min_snr: float, max_snr: float) -> float:
    """random.uniform(min_snr * std, max_snr * std) with its draw `u`: a + (b - a) * u in float64 (wave_augmentation.py:49-50)."""
    a, b = min_snr * float(std32), max_snr * float(std32)
    return a + (b - a) * float(u)


def _check_chunks(chunks, plan: Plan, noise):
    shape = tuple(chunks.shape)
    if len(shape) != 2 or not 1 <= shape[1] <= MAX_WIN:
        raise ValueError(f"augment: chunks [n, win] with 1 <= win <= {MAX_WIN} expected, got {shape}")
    if not isinstance(plan, Plan) or len(plan) != shape[0]:
        raise ValueError(f"augment: a Plan of {shape[0]} windows expected")
    if noise is not None and tuple(noise.shape) != shape:
        raise ValueError(f"augment: noise {shape} expected, got {tuple(noise.shape)}")


def augment_numpy(chunks, plan: Plan, noise=None) -> np.ndarray:
    """The specification of avcer_wave_augment in numpy: chunks f32 [n, win] -> a new f32 [n, win].
    kind 1: -x.  kind 3: clamp(x * ratio32, -1, 1) in float32, NaN staying NaN.  kind 2: x + float32(noise_std * z) with
    std32_numpy, noise_std_numpy and normal_stream -- or x + noise[w] when `noise` f32 [n, win] is given."""
    x = np.array(chunks, dtype=np.float32)
    _check_chunks(x, plan, noise)
    nz = None if noise is None else np.asarray(noise, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for w in range(x.shape[0]):
            k = int(plan.kind[w])
            if k == KIND_POLARITY:
                x[w] = -x[w]
            elif k == KIND_GAIN:
                g = x[w] * np.float32(plan.ratio32[w])
                x[w] = np.where(g < -one, -one, np.where(g > one, one, g))
            elif k == KIND_NOISE and nz is not None:
                x[w] = x[w] + nz[w]
            elif k == KIND_NOISE:
                s = noise_std_numpy(std32_numpy(x[w]), plan.u[w], plan.min_snr, plan.max_snr)
                x[w] = x[w] + (s * normal_stream(int(plan.key[w]), x.shape[1]).astype(np.float64)).astype(np.float32)
    return x


# ------------------------------------------------------------------------------------------------ the device call
def augment(engine, chunks, plan: Plan, noise=None, return_std: bool = False):
    """augment_numpy on the device, IN PLACE: chunks f32 [n, win], the contiguous device tensor Engine.audio_chunks(padding=
    "constant") returned, in front of Engine.audio_forward(normalize=True).  One Engine.wave_augment call; nothing synchronises
    with the host.  Returns chunks (with `return_std` also the kernel's float32 std per kind-2 window)."""
    _check_chunks(chunks, plan, noise)
    return engine.wave_augment(chunks, plan.records(), plan.min_snr, plan.max_snr, noise, return_std)
