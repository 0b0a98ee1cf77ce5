"""The audio model (audio.hip avcer_audio_forward) launch by launch against the float64 oracle (oracle/audio.py
expr_model_v3_forward64): every debug tap of the forward, in the exact-f32 and the x3 mode, at six window lengths from the
shortest to the longest accepted one; local checks of the small kernels from the library's own tapped inputs; a production-size
call (130 windows: the weights-direct contraction form and the 128-window pass boundary).

Taps of avcer_audio_forward and what becomes of each (none is left out):
  norm conv0 extract proj pos_in posconv layer<0..11> w2v tl1 tl2 td0 mp td4 pooled      compared (_tap_list)
  ln:fe<1..6>.ln ln:fp.ln ln:enc<l>.ln1|ln2 ln:tl<l>.ln1|ln2 att:enc<l> att:tl<l> pe:tl<l>     compared
  out:fe<1..6>.w out:enc<l>.qkv.w|o.w|ff1.w out:tl<l>.qkv.w|o.w|ff1.w|ff2.w                  compared
  out:fp.w out:enc<l>.ff2.w out:td0.w out:td4.w     the buffers of proj / layer<l> / td0 / td4 under their second name: compared at
                                                    99 tokens only (ALIASES)
  out:pos.w                                         never written: Net::gemm taps dense single-group outputs, the positional conv is
                                                    one grouped launch into the stream (its sum with proj is "posconv")
The convolution of extractor layer 0 is fused with its LayerNorm and GELU (conv0_ln_gelu_kernel): the library has no tensor for the
oracle's "out:fe0.w"; _check_conv0_local compares the fused kernel with float64 from its own input instead.

The net holds.  With the bounds below, ONE change on the oracle side (99 tokens, both modes; tap, max|err|/max|ref|, bound):
  (a) one encoder layer's ff1 weight rounded to fp16 (an x3 contraction without its lo terms), layers 2, 5 and 10 in turn:
      out:enc<l>.ff1.w 2.2e-4 against 1.2e-5 (f32) / 8e-6 (x3), layer<l> 8.1e-5 / 7.4e-5 / 5.5e-5, and EVERY tap behind it in both
      modes: 88, 67 and 32 of the 126 taps, down to pooled at 4.4e-5 / 3.9e-5 / 1.8e-5; no tap in front of it.
  (b) one LayerNorm's epsilon at 1e-6: extractor layer 0 (the smallest variances of the model): conv0 2.0e-5 against 1.0e-5 / 8e-6,
      out:fe1.w 1.5e-5 and ln:fe1.ln 1.2e-5 in both modes, out:fe2.w and out:fe3.w (8.4e-6) in x3 as well; the feature
      projection's: ln:fp.ln, proj, pos_in, posconv at 1.3e-5 and 95 later taps in x3, in the f32 mode 1.2e-5 under proj's 1.3e-5
      and 34 later taps (the contexts from att:enc1 on, the stream from layer 4 on).  In an encoder layer the rows' variance is
      O(1) and the change moves the oracle by 4e-6 (enc0.ln1) to 2e-7 (enc11): below what float32 resolves, no tap fails, and no
      float32-grade bound could make one.
  (c) tanh GELU in extractor layer 3: ln:fe3.ln 9.8e-5, out:fe4.w 2.2e-4 and every tap behind, 119 of 126 in both modes, down to
      pooled at 6.0e-5 (logits 5.3e-5 against 1.4e-5).
  With no change, 0 of 126 in both modes.
"""
import math
import time

import numpy as np
import pytest
import torch

from avcer_amd import synth
from avcer_amd._lib import AvcerError
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine
from avcer_amd.sp32 import raw_to_f32
from oracle import audio as oa

pytestmark = pytest.mark.gpu

MODES = {MODE_FP32: "fp32", MODE_F16X3: "x3"}
U = 2.0 ** -24                      # unit roundoff of float32
E = 1024
# (samples, windows, seed): 51 tokens (L3 = 1), 99 (today's case), 128 (the 8-key-tile attention with every tile full; odd sample
# count), 129 (first size of the 16-key-tile form), 199 (the reference's window), 256 (the longest, no padded key)
CASES = ((16400, 3, 5701), (32000, 2, 5678), (41041, 2, 5702), (41360, 2, 5703), (64000, 3, 5679), (82000, 2, 5704))
TOKENS = {16400: 51, 32000: 99, 41041: 128, 41360: 129, 64000: 199, 82000: 256}
L3 = {16400: 1, 32000: 4, 41041: 6, 41360: 6, 64000: 10, 82000: 14}
ALIASES = {"out:fp.w": "proj", "out:td0.w": "td0", "out:td4.w": "td4", **{f"out:enc{l}.ff2.w": f"layer{l}" for l in range(12)}}


@pytest.fixture(scope="module")
def sd64(sd_audio):
    return oa.state_dict64(sd_audio)


# ------------------------------------------------------------------------------------------------------------ tap plumbing
def _is_split(name, mode):
    """Operand-typed tensors are sp32 pairs in the x3 mode (audio.hip: extractor activations, LN outputs, contexts, FFN hidden,
    pos_in, x + PE); everything else, and every tap of the f32 mode, is f32."""
    return mode == MODE_F16X3 and (name in ("conv0", "extract", "pos_in") or name.startswith(("ln:", "att:", "pe:"))
                                   or name.endswith(".ff1.w"))


def _tap_list(aliases, middle_out=True):
    """(library tap, oracle tap) for every launch of the forward, in launch order.  middle_out=False leaves out the "out:" taps of
    encoder layers 4-7 (the module's time: done at 199 and 256 tokens; every launch stays tapped at 51, 99, 128 and 129)."""
    t = [("norm", "norm"), ("conv0", "ln:fe0.ln")]
    for i in range(1, 7):
        t += [(f"out:fe{i}.w",) * 2, (f"ln:fe{i}.ln",) * 2]
    t += [("extract", "ln:fe6.ln"), ("ln:fp.ln",) * 2, ("proj",) * 2, ("pos_in",) * 2, ("posconv",) * 2]
    for l in range(12):
        p = f"enc{l}"
        t += [(f"ln:{p}.ln1",) * 2, (f"out:{p}.qkv.w",) * 2, (f"att:{p}",) * 2, (f"out:{p}.o.w",) * 2, (f"ln:{p}.ln2",) * 2,
              (f"out:{p}.ff1.w",) * 2, (f"layer{l}",) * 2]
    t.append(("w2v", "w2v"))
    for p in ("tl1", "tl2"):
        t += [(f"pe:{p}",) * 2, (f"out:{p}.qkv.w",) * 2, (f"att:{p}",) * 2, (f"out:{p}.o.w",) * 2, (f"ln:{p}.ln1",) * 2,
              (f"out:{p}.ff1.w",) * 2, (f"out:{p}.ff2.w",) * 2, (f"ln:{p}.ln2",) * 2, (p, p)]
    t += [("td0",) * 2, ("mp",) * 2, ("td4",) * 2, ("pooled",) * 2]
    if not middle_out:
        t = [x for x in t if not x[0].startswith(("out:enc4.", "out:enc5.", "out:enc6.", "out:enc7."))]
    if aliases:
        t += list(ALIASES.items())
    return t


def _tap(eng, name, wav_dev, mode, shape, normalize=True, rows=None):
    """One forward with `name` armed; the tap as float64 on the host, all of it or the windows `rows` of it."""
    split = _is_split(name, mode)
    numel = math.prod(shape)
    dst = eng.debug_tap(name, numel * (2 if split else 1), dtype=torch.int16 if split else torch.float32)
    out = eng.audio_forward(wav_dev, normalize, mode)
    torch.cuda.synchronize()
    assert eng.debug_tap_copied() == numel * 4, (name, eng.debug_tap_copied(), numel * 4)
    if rows is not None:
        dst = dst.view(shape[0], -1)[rows].contiguous()
        shape = (len(rows),) + tuple(shape[1:])
    got = raw_to_f32(dst.cpu(), tuple(shape)) if split else dst.cpu().view(shape)
    return got.double(), out


def _family(tap):
    if tap == "w2v":
        return "enc8-11.ln"
    if tap.startswith(("layer", "ln:enc", "att:enc", "out:enc")):
        l = int("".join(c for c in tap.split(".")[0] if c.isdigit()))
        kind = ("ln" if tap.startswith("ln:") else "att" if tap.startswith("att:") else "qkv" if tap.endswith("qkv.w")
                else "ffh" if tap.endswith("ff1.w") else "res")
        return ("enc0-3.", "enc4-7.", "enc8-11.")[l // 4] + kind
    for p in ("tl1", "tl2"):
        if p in tap:
            return p
    if tap in ("td0", "mp", "td4", "pooled", "out:td0.w", "out:td4.w"):
        return "head"
    if tap in ("ln:fp.ln", "proj", "pos_in", "posconv", "out:fp.w"):
        return "proj"
    return "extractor"


# max|err| / max|ref| over all elements of the tapped windows; each bound about 4x the worst tap of its family over the six inputs
# (measured on the MI355X; the tap and its token count beside it), none above 5e-5.  The error does not grow along the graph: the
# first MFMA contraction makes it (out:fe1.w, K = 1536: 2.2e-6 in the f32 mode, whose contractions accumulate plain f32 products,
# 1.3e-6 in x3; conv0 in front of it is at 3e-7) and every LayerNorm renormalises what it carries, so each later tap holds about
# one contraction's error.  That is what lifts the f32 mode's families past 1e-5 at 4x; beyond it, "proj" has the positional
# conv (K = 8192 per group), "tl1" the 32-wide heads of attention_kernel at 199 keys, "head" td0 (K = 5120).  The contexts sit
# lower (a softmax-weighted mean of v) and keep bounds of their own.  (The "out:" figures of layers 4-7 at 199 / 256 tokens date
# from the run that still tapped them there, see _tap_list.)
TAP_BOUND = {
    MODE_FP32: {"extractor": 1.0e-5,    # measured 2.60e-6 (extract, 199)
                "proj": 1.3e-5,         # measured 3.19e-6 (posconv, 199)
                "enc0-3.ln": 1.2e-5,    # measured 3.11e-6 (ln:enc0.ln2, 199)
                "enc0-3.qkv": 1.1e-5,   # measured 2.83e-6 (out:enc0.qkv.w, 128)
                "enc0-3.att": 7e-6,     # measured 1.71e-6 (att:enc0, 51)
                "enc0-3.res": 1.2e-5,   # measured 3.05e-6 (out:enc0.o.w, 199)
                "enc0-3.ffh": 1.2e-5,   # measured 2.88e-6 (out:enc1.ff1.w, 99)
                "enc4-7.ln": 1.1e-5,    # measured 2.85e-6 (ln:enc4.ln1, 51)
                "enc4-7.qkv": 1.1e-5,   # measured 2.67e-6 (out:enc6.qkv.w, 199)
                "enc4-7.att": 5e-6,     # measured 1.28e-6 (att:enc7, 256)
                "enc4-7.res": 1.0e-5,   # measured 2.61e-6 (out:enc6.o.w, 129)
                "enc4-7.ffh": 1.2e-5,   # measured 2.96e-6 (out:enc7.ff1.w, 256)
                "enc8-11.ln": 1.0e-5,   # measured 2.57e-6 (ln:enc8.ln2, 99)
                "enc8-11.qkv": 1.1e-5,  # measured 2.74e-6 (out:enc10.qkv.w, 51)
                "enc8-11.att": 4e-6,    # measured 9.92e-7 (att:enc9, 256)
                "enc8-11.res": 1.0e-5,  # measured 2.39e-6 (layer11, 199)
                "enc8-11.ffh": 1.2e-5,  # measured 2.96e-6 (out:enc8.ff1.w, 99)
                "tl1": 1.3e-5,          # measured 3.13e-6 (att:tl1, 199)
                "tl2": 9e-6,            # measured 2.25e-6 (out:tl2.ff1.w, 199)
                "head": 1.5e-5},        # measured 3.83e-6 (td0, 256)
    MODE_F16X3: {"extractor": 8e-6,     # measured 2.04e-6 (extract, 199)
                 "proj": 8e-6,          # measured 2.07e-6 (ln:fp.ln, 199)
                 "enc0-3.ln": 8e-6,     # measured 2.00e-6 (ln:enc0.ln1, 199)
                 "enc0-3.qkv": 7.5e-6,  # measured 1.88e-6 (out:enc3.qkv.w, 256)
                 "enc0-3.att": 5.5e-6,  # measured 1.36e-6 (att:enc0, 51)
                 "enc0-3.res": 8e-6,    # measured 1.95e-6 (out:enc2.o.w, 99)
                 "enc0-3.ffh": 8e-6,    # measured 2.01e-6 (out:enc2.ff1.w, 51)
                 "enc4-7.ln": 7.5e-6,   # measured 1.90e-6 (ln:enc7.ln2, 256)
                 "enc4-7.qkv": 6.5e-6,  # measured 1.63e-6 (out:enc6.qkv.w, 129)
                 "enc4-7.att": 2.5e-6,  # measured 6.25e-7 (att:enc6, 51)
                 "enc4-7.res": 7.5e-6,  # measured 1.88e-6 (out:enc7.o.w, 256)
                 "enc4-7.ffh": 7e-6,    # measured 1.79e-6 (out:enc7.ff1.w, 51)
                 "enc8-11.ln": 8e-6,    # measured 1.97e-6 (ln:enc8.ln1, 256)
                 "enc8-11.qkv": 7.5e-6,  # measured 1.90e-6 (out:enc8.qkv.w, 99)
                 "enc8-11.att": 3e-6,   # measured 7.08e-7 (att:enc9, 51)
                 "enc8-11.res": 6.5e-6,  # measured 1.64e-6 (out:enc8.o.w, 256)
                 "enc8-11.ffh": 7e-6,   # measured 1.82e-6 (out:enc9.ff1.w, 199)
                 "tl1": 5.5e-6,         # measured 1.41e-6 (out:tl1.qkv.w, 199)
                 "tl2": 5.5e-6,         # measured 1.42e-6 (out:tl2.ff1.w, 199)
                 "head": 9.5e-6},       # measured 2.39e-6 (td0, 128)
}
# the logits: max|dlogit| < 1e-4 as everywhere, and max|err| / max|ref|: measured 3.61e-6 (fp32) and 2.12e-6 (x3), both at 51 tokens
# (max|dlogit| 2.7e-5 and 1.6e-5)
LOGIT_BOUND = {MODE_FP32: 1.4e-5, MODE_F16X3: 8.5e-6}


def _oracle(sd64, wav, norm=True):
    ref = {}
    lg = oa.expr_model_v3_forward64(sd64, wav, ref, norm=norm)
    ref["logits"] = lg.reshape(len(wav), -1)
    return ref


def measure_case(eng, ref, wav, mode, taps, normalize=True):
    """{library tap: max|err| / max|ref|} of one input in one mode, and the logits' (max|dlogit|, relative)."""
    wav_dev = torch.from_numpy(wav).to(eng.device)
    rel, out = {}, None
    for lib, orc in taps:
        r = ref[orc]
        got, out = _tap(eng, lib, wav_dev, mode, tuple(r.shape), normalize)
        rel[lib] = ((got - r).abs().max() / r.abs().max()).item()
    if out is None:
        out = eng.audio_forward(wav_dev, normalize, mode)
    d = (out.cpu().double() - ref["logits"]).abs().max().item()
    return rel, (d, d / ref["logits"].abs().max().item())


def test_window_lengths_outside_the_range_are_refused(engine_audio):
    """16399 samples are 50 tokens (the head's max-pool would leave 2 positions for a 3-tap convolution), 82320 are 257 (the
    attention kernels hold at most 256 keys): an error, not a run."""
    for t in (16399, 82320):
        for mode in MODES:
            with pytest.raises(AvcerError):
                engine_audio.audio_forward(torch.from_numpy(synth.waveforms(1, 1, t)), True, mode)


def test_every_tap_against_float64_oracle(engine_audio, sd64):
    t_start = time.time()
    eng = engine_audio
    worst = {m: {} for m in MODES}
    logit = {m: (0.0, 0.0, 0) for m in MODES}
    eng.x3_overflow_count(reset=True)
    for samples, batch, seed in CASES:
        wav = synth.waveforms(seed, batch, samples)
        ref = _oracle(sd64, wav)
        tokens = ref["w2v"].shape[1]
        assert tokens == TOKENS[samples] and ref["td4"].shape[1] == L3[samples], (samples, tokens, ref["td4"].shape)
        assert ref["ln:fe0.ln"].shape[1] == (samples - 10) // 5 + 1
        for mode in MODES:
            rel, lg = measure_case(eng, ref, wav, mode, _tap_list(aliases=tokens == 99, middle_out=tokens < 199))
            for k, v in rel.items():
                if v >= worst[mode].get(k, (-1.0,))[0]:
                    worst[mode][k] = (v, tokens)
            if lg[1] >= logit[mode][1]:
                logit[mode] = (lg[0], lg[1], tokens)
            assert lg[0] < 1e-4, (MODES[mode], tokens, lg)
        del ref
    assert eng.x3_overflow_count(reset=True) == 0
    for mode, taps in worst.items():
        fam = {}
        for k, (v, tok) in taps.items():
            if v >= fam.get(_family(k), (-1.0,))[0]:
                fam[_family(k)] = (v, k, tok)
        print(f"{MODES[mode]} worst tap per family:", {f: f"{v:.2e} {k}@{tok}" for f, (v, k, tok) in fam.items()})
        print(f"{MODES[mode]} per tap:", {k: f"{v:.1e}@{tok}" for k, (v, tok) in taps.items()})
        print(f"{MODES[mode]} logits: max|dlogit| {logit[mode][0]:.2e}, relative {logit[mode][1]:.2e} at {logit[mode][2]} tokens")
    print(f"every tap, six lengths, two modes: {time.time() - t_start:.1f} s")
    for mode, taps in worst.items():
        bad = {k: v for k, v in taps.items() if v[0] >= TAP_BOUND[mode][_family(k)]}
        assert not bad, (MODES[mode], bad)
        assert logit[mode][1] < LOGIT_BOUND[mode], (MODES[mode], logit[mode])


# ------------------------------------------------------------------------------------------------------------ local checks
def _ln_bound(x, g, b, eps, dx=0.0, gelu=False, split=False):
    """Elementwise error bound of a float32 two-pass LayerNorm (+ GELU) of the rows of x (float64, the kernel's own input), and
    its float64 value.  One wave per row: a lane adds C/64 <= 16 elements, six butterfly steps and the 1/C multiply follow, so
    the mean is off by at most 23 u max|x| (+ dx, the error the input itself may carry); with s = sqrt(var + eps) and
    A = (23 u max|x| + dx) / s, the centred value (x - mean) / s is off by A + u |n|, the sum of squares by a relative 2 A + 24 u,
    rsqrt by half of that + 2 u: dn <= A + |n| (A + 16 u).  y = n g + b adds three roundings; GELU has slope <= 1.13 and is
    within 4.7e-7 of exact in both of its forms (gemm_dev.h gelu_fast) + 2 u |y| beyond |y| = 8; an sp32 pair keeps 22 bits, and
    2^-25 absolute below 2^-3."""
    mean = x.mean(-1, keepdim=True)
    s = torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    n = (x - mean) / s
    a = (23 * U * x.abs().amax(-1, keepdim=True) + dx) / s
    dn = a + n.abs() * (a + 16 * U)
    y = n * g + b
    dy = g.abs() * dn + 3 * U * ((n * g).abs() + b.abs())
    if gelu:
        y = torch.nn.functional.gelu(y)
        dy = 1.13 * dy + 4.7e-7 + 2 * U * y.abs()
    if split:
        dy = dy + torch.clamp(y.abs() * 2.0 ** -22, min=2.0 ** -25)
    return y, dy


def _ln_checks():
    """(output tap, input tap, state-dict prefix, GELU behind it) of every LayerNorm launch with a tap on both sides."""
    w = "wav2vec2."
    c = [(f"ln:fe{i}.ln", f"out:fe{i}.w", f"{w}feature_extractor.conv_layers.{i}.layer_norm", True) for i in range(1, 7)]
    c.append(("ln:fp.ln", "extract", w + "feature_projection.layer_norm", False))
    for l in range(12):
        p = f"{w}encoder.layers.{l}."
        c.append((f"ln:enc{l}.ln1", "posconv" if l == 0 else f"layer{l - 1}", p + "layer_norm", False))
        c.append((f"ln:enc{l}.ln2", f"out:enc{l}.o.w", p + "final_layer_norm", False))
    c.append(("w2v", "layer11", w + "encoder.layer_norm", False))
    for p in ("tl1", "tl2"):
        c.append((f"ln:{p}.ln1", f"out:{p}.o.w", p + ".add_norm_after_attention.layer_norm", False))
        c.append((f"ln:{p}.ln2", f"out:{p}.ff2.w", p + ".add_norm_after_ff.layer_norm", False))
    return c


def _row_report(got, ref, bound):
    """Per row: max|err| and the bound, both over the row's own max|ref|.  Returns (worst relative error, worst error / bound)."""
    rows = ref.reshape(-1, ref.shape[-1])
    err = (got - ref).abs().reshape(rows.shape).amax(-1)
    lim = bound.reshape(rows.shape).amax(-1)
    scale = rows.abs().amax(-1).clamp_min(1e-300)
    return (err / scale).max().item(), (err / lim).max().item()


def _check_layernorms(eng, sd64, wav, normalize, shapes, what):
    """Every tapped LayerNorm output from the library's own tap in front of it, row by row, the last row of every window and the
    rows of a 51-token input included."""
    wav_dev = torch.from_numpy(wav).to(eng.device)
    worst = {}
    for mode in MODES:
        for out_tap, in_tap, p, gelu in _ln_checks():
            x, _ = _tap(eng, in_tap, wav_dev, mode, shapes[in_tap], normalize)
            got, _ = _tap(eng, out_tap, wav_dev, mode, shapes[out_tap], normalize)
            ref, bound = _ln_bound(x, sd64[p + ".weight"], sd64[p + ".bias"], oa.LN_EPS, gelu=gelu,
                                   split=_is_split(out_tap, mode))
            rel, frac = _row_report(got, ref, bound)
            worst[(MODES[mode], out_tap)] = (rel, frac)
    top = max(worst.items(), key=lambda kv: kv[1][1])
    print(f"LayerNorm from its own input, {what}: worst row {top[0]} err/max|row| {top[1][0]:.2e} = {top[1][1]:.2f} of its bound;"
          f" largest err/max|row| {max(v[0] for v in worst.values()):.2e}")
    bad = {k: v for k, v in worst.items() if not v[1] <= 1.0}
    assert not bad, bad


def _check_conv0_local(eng, sd64, x_lib, wav_dev, normalize, mode, what):
    """conv0_ln_gelu_kernel from its own input x_lib (float64 copy of the f32 samples it read): Conv1d(1 -> 512, k 10, s 5) in
    float32 is ten products and ten sums per output, dx <= 11 u (sum|w x| + |b|), in front of the LayerNorm bound."""
    p = "wav2vec2.feature_extractor.conv_layers.0"
    w, b = sd64[p + ".conv.weight"], sd64[p + ".conv.bias"]
    h = torch.nn.functional.conv1d(x_lib[:, None, :], w, b, stride=5).transpose(1, 2)
    mag = torch.nn.functional.conv1d(x_lib[:, None, :].abs(), w.abs(), b.abs(), stride=5).transpose(1, 2)
    dx = 11 * U * mag.amax(-1, keepdim=True)
    ref, bound = _ln_bound(h, sd64[p + ".layer_norm.weight"], sd64[p + ".layer_norm.bias"], oa.LN_EPS, dx=dx, gelu=True,
                           split=_is_split("conv0", mode))
    got, _ = _tap(eng, "conv0", wav_dev, mode, tuple(ref.shape), normalize)
    rel, frac = _row_report(got, ref, bound)
    print(f"conv0 from its own input, {what}, {MODES[mode]}: worst row err/max|row| {rel:.2e}, {frac:.2f} of its bound")
    assert frac <= 1.0, (what, MODES[mode], rel, frac)


def _shapes(ref):
    return {k: tuple(v.shape) for k, v in ref.items()}


def _ln_shapes(batch, samples):
    """Shapes of the taps on both sides of every LayerNorm, by avcer_audio_forward's length arithmetic."""
    shapes, n = {}, samples
    for i, (k, st) in enumerate(zip(oa.CONV_KERNEL, oa.CONV_STRIDE)):
        n = (n - k) // st + 1
        shapes[f"out:fe{i}.w"] = shapes[f"ln:fe{i}.ln"] = (batch, n, 512)
    shapes["extract"] = shapes["ln:fp.ln"] = (batch, n, 512)
    for out_tap, in_tap, _, _ in _ln_checks():
        shapes.setdefault(out_tap, (batch, n, E))
        shapes.setdefault(in_tap, (batch, n, E))
    return shapes


def test_small_kernels_from_the_librarys_own_inputs(engine_audio, sd_audio, sd64):
    """What a cumulative tap cannot see: each small kernel's output against float64 of the library's OWN tapped input."""
    t_start = time.time()
    eng = engine_audio
    fd_w, fd_b = sd64["feature_downsample.weight"], sd64["feature_downsample.bias"]
    for samples, batch, seed in CASES:
        wav = synth.waveforms(seed, batch, samples)
        wav_dev = torch.from_numpy(wav).to(eng.device)
        s, l3 = TOKENS[samples], L3[samples]
        l1 = (s - 9) // 3 + 1
        l2 = l1 // 5
        assert l2 - 2 == l3
        for mode in MODES:
            x3 = mode == MODE_F16X3
            # max over 5 and ReLU round nothing: bit-equal
            td0, _ = _tap(eng, "td0", wav_dev, mode, (batch, l1, E))
            mp, _ = _tap(eng, "mp", wav_dev, mode, (batch, l2, E))
            assert torch.equal(mp, torch.relu(td0[:, :l2 * 5].reshape(batch, l2, 5, E).amax(2))), (samples, MODES[mode], "mp")
            # x + PE: one float32 add (bit-equal in the f32 mode); an sp32 pair holds it to 2^-22, or 2^-25 below 2^-3
            for tl, src in (("tl1", "w2v"), ("tl2", "tl1")):
                x, _ = _tap(eng, src, wav_dev, mode, (batch, s, E))
                pe = sd_audio[tl + ".positional_encoding.pe"].reshape(-1, E)[:s]
                want = (x.float() + pe).double()
                got, _ = _tap(eng, "pe:" + tl, wav_dev, mode, (batch, s, E))
                if x3:
                    assert ((got - want).abs() <= torch.clamp(want.abs() * 2.0 ** -22, min=2.0 ** -25)).all(), (samples, tl)
                else:
                    assert torch.equal(got, want), (samples, tl)
            # ReLU(mean over L3): L3 - 1 sums and a division in float32
            td4, _ = _tap(eng, "td4", wav_dev, mode, (batch, l3, E))
            pooled, out = _tap(eng, "pooled", wav_dev, mode, (batch, E))
            err = (pooled - torch.relu(td4.mean(1))).abs()
            assert (err <= (l3 + 1) * U * td4.abs().sum(1) / l3).all(), (samples, MODES[mode], "pooled", err.max().item())
            # the last Linear: a lane adds 16 products, six butterfly steps and the bias follow: 24 roundings on any term
            _check_logits(out, pooled, fd_w, fd_b, (samples, MODES[mode]))
        if samples in (16400, 32000, 82000):
            shapes = _ln_shapes(batch, samples)
            assert shapes["extract"][1] == s
            _check_layernorms(eng, sd64, wav, True, shapes, f"{s} tokens")
            for mode in MODES:
                x_lib, _ = _tap(eng, "norm", wav_dev, mode, (batch, samples))
                _check_conv0_local(eng, sd64, x_lib, wav_dev, True, mode, f"{s} tokens")
    print(f"local checks: {time.time() - t_start:.1f} s")


def _check_logits(out, pooled, w, b, what):
    want = pooled @ w.T + b
    lim = 24 * U * (pooled.abs() @ w.abs().T + b.abs())
    err = (out.cpu().double() - want).abs()
    assert (err <= lim).all(), (what, "logits from pooled", (err / lim).max().item())


def test_last_linear_at_seven_classes():
    """fd.w / fd.b of the 7-class variant: logits from the library's own pooled tap, same bound."""
    eng = Engine(0)
    try:
        sd = synth.to_torch(synth.audio_state_dict(43, num_classes=7))
        eng.load_audio(sd)
        assert eng.audio_classes == 7
        wav_dev = torch.from_numpy(synth.waveforms(777, 2, 32000)).to(eng.device)
        for mode in MODES:
            pooled, out = _tap(eng, "pooled", wav_dev, mode, (2, E))
            assert tuple(out.shape) == (2, 7)
            _check_logits(out, pooled, sd["feature_downsample.weight"].double(), sd["feature_downsample.bias"].double(),
                          (7, MODES[mode]))
    finally:
        eng.close()


def offset_burst_window():
    """One 2 s window: a seeded noise burst (sigma 0.1) on a DC offset of 0.5 for 1 s, then 1 s of exact silence."""
    x = np.zeros((1, 32000), np.float32)
    x[0, :16000] = 0.5 + synth.waveforms(5705, 1, 16000)[0]
    return x


def test_layernorms_under_an_offset_and_on_silence(engine_audio, sd64):
    """Real weights, a waveform run as it is (normalize=False): at conv0's LayerNorm the burst's rows carry the offset's response
    in every channel (max|x| / s up to 3.9) and the silent rows are the bare conv bias (standard deviation 0.028 over the
    channels, the smallest of the model: eps is 1.2 % of their variance).  In float64 the input is well-posed: moving eps by one
    float32 ulp moves no oracle tap by more than 3.8e-10 of its max (out:fe1.w; 5.6e-11 at the logits).  Then the same window
    with normalize=True: wav_normalize_kernel's two-pass mean / variance under the offset.  512 threads add 63 samples each, six
    butterfly steps, eight partial sums: mean and variance carry at most 80 roundings each, so with a = 80 u max|x| / s the
    output y = (x - m) / s is off by a + |y| (a + 40 u + 4 u)."""
    eng = engine_audio
    wav = offset_burst_window()
    wav_dev = torch.from_numpy(wav).to(eng.device)
    ref = _oracle(sd64, wav, norm=False)
    assert all(torch.isfinite(v).all() for v in ref.values())
    _check_layernorms(eng, sd64, wav, False, _shapes(ref), "offset burst + silence, as it is")
    for mode in MODES:
        _check_conv0_local(eng, sd64, torch.from_numpy(wav).double(), wav_dev, False, mode, "offset burst + silence, as it is")
        rel, lg = measure_case(eng, ref, wav, mode, [], normalize=False)
        print(f"offset burst + silence, as it is, {MODES[mode]}: max|dlogit| {lg[0]:.2e}")
        assert lg[0] < 1e-4
        x = torch.from_numpy(wav).double()
        want = oa.normalize64(wav)
        s = torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-7)
        a = 80 * U * x.abs().amax(-1, keepdim=True) / s
        lim = a + want.abs() * (a + 44 * U)
        got, _ = _tap(eng, "norm", wav_dev, mode, (1, 32000), True)
        err = (got - want).abs()
        print(f"norm under the offset, {MODES[mode]}: max|err| {err.max().item():.2e}, {(err / lim).max().item():.2f} of its bound")
        assert (err <= lim).all()
        _check_conv0_local(eng, sd64, got, wav_dev, True, mode, "offset burst + silence, normalised")


# ------------------------------------------------------------------------------------- production size and the pass boundary
SUBSET = ("conv0", "extract", "proj", "posconv", "layer0", "layer11", "att:enc0", "out:enc11.ff1.w", "w2v", "tl2", "td4", "pooled")
ORACLE_TAP = {"conv0": "ln:fe0.ln", "extract": "ln:fe6.ln"}
LINEARS = {(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)}   # (N, K) of qkv, out-proj, ff1, ff2


def test_production_size_call_and_the_pass_boundary(sd_audio, sd64):
    """130 windows of 2 s in one call: a pass of 128 windows (M = 12672 rows: in the x3 mode the encoder's linears run
    conv_gemm_wd_kernel, the form the benchmark runs) and a pass of 2.  A debug tap is one-shot (Net::tap disarms it after its
    first copy), so after such a call it holds the FIRST pass: windows 0 and 127 of it are compared with the float64 oracle under
    the bounds above, as are windows 0, 63 and 127 of a 128-window call.  The second pass is held at the logits: rows 128 and 129
    against the oracle, rows 126 .. 129 of logits and features bit for bit against a call of those four windows."""
    t_start = time.time()
    eng = Engine(0)
    try:
        eng.load_audio(sd_audio)
        wav = synth.waveforms(3, 130, 32000)
        wav_dev = torch.from_numpy(wav).to(eng.device)
        picked = (0, 63, 127, 128, 129)
        ref = _oracle(sd64, wav[list(picked)])
        for mode in MODES:
            x3 = mode == MODE_F16X3
            eng.audio_forward(wav_dev, True, mode)      # weights prepared, workspace sized
            torch.cuda.synchronize()
            eng.profile_enable(True)
            eng.audio_forward(wav_dev, True, mode)
            log = eng.profile_read_launches()
            eng.profile_enable(False)
            big = [l for l in log if l["m"] == 128 * 99 and (l["n"], l["k"]) in LINEARS]
            small = [l for l in log if l["m"] == 2 * 99 and (l["n"], l["k"]) in LINEARS]
            print(f"{MODES[mode]} 130 windows: linears of the first pass", sorted({l["family"] for l in big}),
                  "of the second", sorted({l["family"] for l in small}), f"({len(big)} + {len(small)} launches)")
            assert len(big) == len(small) == 12 * 4 + 2 * 4, (len(big), len(small))
            if x3:
                assert all(l["family"] == "conv_gemm_wd_kernel" for l in big), [l for l in big if l["family"] != "conv_gemm_wd_kernel"]
                assert all(l["family"] != "conv_gemm_wd_kernel" for l in small)
            else:
                assert all(l["family"] == "conv_gemm_kernel" for l in big + small)
            eng.x3_overflow_count(reset=True)
            for n, rows in ((130, (0, 127)), (128, (0, 63, 127))):
                idx = [picked.index(r) for r in rows]
                rels = {}
                for lib in SUBSET:
                    r = ref[ORACLE_TAP.get(lib, lib)][idx]
                    got, out = _tap(eng, lib, wav_dev[:n], mode, (128,) + tuple(r.shape[1:]), rows=list(rows))
                    rels[lib] = ((got - r).abs().max() / r.abs().max()).item()
                print(f"{MODES[mode]} {n} windows, windows {rows} of the first pass:", {k: f"{v:.1e}" for k, v in rels.items()})
                bad = {k: v for k, v in rels.items() if v >= TAP_BOUND[mode][_family(k)]}
                assert not bad, (MODES[mode], n, bad)
            lg, feats = eng.audio_forward(wav_dev, True, mode, return_features=True)
            four, four_feats = eng.audio_forward(wav_dev[126:130], True, mode, return_features=True)
            assert torch.equal(lg[126:130], four), MODES[mode]
            assert torch.equal(feats[126:130], four_feats), MODES[mode]  # the second pass's features land behind the first's
            want = ref["logits"][[0, 2, 3, 4]]
            d = (lg[[0, 127, 128, 129]].cpu().double() - want).abs().max().item()
            print(f"{MODES[mode]} 130 windows: rows 0, 127, 128, 129 max|dlogit| {d:.2e}")
            assert d < 1e-4 and d / want.abs().max().item() < LOGIT_BOUND[mode], (MODES[mode], d)
            assert eng.x3_overflow_count(reset=True) == 0
    finally:
        eng.close()
    print(f"production-size call: {time.time() - t_start:.1f} s")
