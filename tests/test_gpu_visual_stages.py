"""The recognition branch launch by launch against float64: the static ResNet-50 (visual.hip static_forward_lane) against
oracle/video.py resnet50_forward64 and the two-layer LSTM (dynamic_forward_impl) against lstm_forward64, every debug tap of
both forwards; local checks of avgpool_kernel, fc1, small_linear_kernel (fc2 + softmax) and lstm_cell_kernel from the library's
OWN tapped inputs.

Taps of static_forward_lane / run_bneck_stage and what becomes of each (none is left out; _tap_list enumerates them per mode):
  pre stem_conv                         f32 / bf16 modes: compared.  The x3 mode preprocesses inside the fused stem: never written.
  out:stem.w                            f32 / bf16: the buffer of stem_conv under its contraction name: compared in case A (ALIASES)
  stem                                  compared, every mode
  out:l<s>.<b>.c1.w                     f32 / bf16: every block.  x3: the conv1 launches that exist there -- l1.0, l2.0, l2.1, l3.0,
                                        l3.1 and stage 4 (every other conv1 is emitted by the fused launch in front of it): compared
  out:l<s>.<b>.c2.w                     f32 / bf16: every block.  x3: l2.0, l3.0 .. l3.5, stage 4 (the chains of stages 1-2 keep
                                        conv2 in registers): compared; at the last block of stages 1-3 against the oracle's
                                        stride-1 conv2 at [::2, ::2]
  out:l<s>.0.c3d.w out:l<s>.<b>.c3.w    conv3 + shortcut + ReLU = the block output.  f32 / bf16: every block; x3: l2.0, l3.0, l3.5
                                        (the r_sub residual path) and stage 4: compared
  chain_out:l<s>.<b>. chain_t1n:l<s>.<b>.   x3: l1.0-l1.2 and l2.1-l2.3; the strided last block of a chain has no t1n: compared
  out:l3.<b>.c3.wf out:l3.<b+1>.c1.wf   x3, b = 1..4, at most kTailPairRows stage-3 positions (cases A, C, D): compared
  tail_out:l3.<b>. tail_t1n:l3.<b>.     x3, b = 1..4, above kTailPairRows (case B, 85 frames): compared
  l1b0_c1 l1b0                          compared, every mode
  l1b0_c2                               f32 / bf16: compared.  x3: conv2 stays in the chain's registers, never written
  blk<s>_<b>                            every block, every mode: compared
  layer1 .. layer4 avgpool out:fc1.w    compared, every mode
  returned logits / probs / feats       compared (feats is the buffer of out:fc1.w)
Taps of dynamic_forward_impl: out:lstm1.wih.w (xp1), out:lstm1.whh.w (W_hh h_0: the first recurrent launch; a tap disarms after
its copy), lstm_h1, out:lstm2.wih.w, out:lstm2.whh.w, lstm_h2 and the returned logits: all compared.

Oracle-side hook.  _oracle_cnn(sd64, x, hook) passes `hook` to resnet50_forward64 (its docstring names the keys); together with a
changed sd64 it is how the following was produced.  No committed test sets it.

The net holds.  With the bounds below, ONE change on the oracle side, case A (frames 0 and 84; 76 taps in the f32 mode, 67 in x3;
tap, max|err| / max|ref|, bound f32 / x3).  In every run no tap in front of the changed launch fails and every tap behind it does:
  (a) one weight rounded to fp16 (an x3 contraction without its lo term):
      layer1.1.conv3: out:l1.1.c3.w / chain_out:l1.1. 6.8e-5 against 1.9e-6 / 2.0e-6, 64 / 60 taps fail in all, the weakest
        out:fc1.w at 1.9e-5 / 1.8e-5 against 6.4e-6 / 4.4e-6; logits 1.6e-5 against 4.6e-6 / 4.0e-6.
      layer2.0.i_downsample.0: out:l2.0.c3d.w 1.4e-4 against 3.4e-6 / 2.6e-6, 55 / 52 taps, the weakest out:fc1.w at 5.7e-5; logits
        6.6e-5.
      layer3.2.conv2: out:l3.2.c2.w 1.4e-4 against 9.4e-6 / 6.8e-6, 31 / 31 taps (out:l3.2.c3.wf and out:l3.3.c1.wf 9.2e-5 and 1.1e-4
        in x3), the weakest avgpool at 3.9e-5 (f32) and out:l4.1.c1.w at 6.3e-5 (x3); logits 3.2e-5.
      lstm1.weight_hh_l0 (n = 3 and 300, unit scale, both modes alike): out:lstm1.whh.w 2.3e-4 / 2.1e-4 against 5.5e-6 / 4.8e-6,
        lstm_h1 7.8e-5 / 8.6e-5 against 3.8e-5, out:lstm2.wih.w 4.6e-5 / 4.0e-5, lstm_h2 5.4e-5 / 5.1e-5 against 3.5e-6 / 3.3e-6,
        logits 4.0e-5 / 4.5e-5 against 3.0e-6 / 2.8e-6.  out:lstm1.wih.w (in front) passes, and so does out:lstm2.whh.w, rightly:
        the tapped launch is W_hh h_0 of layer 2, and h_0 of either layer has no recurrent term in it.
  (b) BN eps 1e-5 in layer1.1: out:l1.1.c1.w (f32) / chain_t1n:l1.0. (x3, the same conv1) 8.1e-4 against 4.1e-6 / 2.9e-6, 66 / 61
      taps, the weakest out:fc1.w at 2.5e-4 (f32), out:l4.0.c2.w at 3.7e-4 (x3); logits 1.7e-4.
  (c) the stride of layer3.0 on conv2 (torchvision's placement; conv1 at stride 1 holds the strided one at its even positions, so
      out:l3.0.c1.w passes): out:l3.0.c2.w 7.4e-1, 39 / 39 taps, the weakest out:fc1.w at 2.0e-2; logits 2.1e-2.
  (d) layer4's mean over 48 positions: avgpool 9.7e-3 and out:fc1.w 7.4e-3 against 6.4e-6 / 4.4e-6, no other tap; logits 6.5e-3.
  With no change, 0 of 76 and 0 of 67, and 0 of the LSTM's 7.  Every change was detected in both modes.
"""
import math
import time

import numpy as np
import pytest
import torch

from avcer_amd import synth
from avcer_amd.engine import MODE_BF16, MODE_F16X3, MODE_FP32, Engine
from avcer_amd.sp32 import raw_to_f32
from oracle import video as ov

pytestmark = pytest.mark.gpu

MODES = {MODE_FP32: "fp32", MODE_F16X3: "x3", MODE_BF16: "bf16"}
F32_GRADE = (MODE_FP32, MODE_F16X3)
U = 2.0 ** -24                      # unit roundoff of float32
TAIL_PAIR_ROWS = 16384              # net.h kTailPairRows
CEILING = 5e-5
N_B = 85                            # case B: 85 * 14 * 14 = 16660 stage-3 positions
ALIASES = {"out:stem.w": "stem_conv"}


def _gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------------------------------------------------ tap plumbing
def _kind(name, mode):
    """Storage of a tap: operand-typed tensors (everything in front of the average pool) are sp32 pairs in the x3 mode and bf16
    in the bf16 mode; "avgpool", fc1's output and every LSTM tap are f32 in every mode."""
    if mode == MODE_FP32 or name in ("avgpool", "out:fc1.w") or "lstm" in name:
        return "f32"
    return "sp32" if mode == MODE_F16X3 else "bf16"


def _tap_list(mode, n_frames, aliases=False):
    """(library tap, oracle tap, even positions only) for every launch of static_forward_lane in `mode` on `n_frames` frames, in
    launch order: run_bneck_stage restated.  The last block of stages 1-3 is evaluated at even positions (stride_last); in the x3
    mode the stride-1 blocks of stages 1-3 are fused, from block 0 in stage 1 and from block 1 in stages 2-3."""
    x3 = mode == MODE_F16X3
    t = [("stem", "stem", False)]
    if not x3:
        t = [("pre", "pre", False), ("stem_conv", "stem_conv", False)] + t
        if aliases:
            t += [(a, o, False) for a, o in ALIASES.items()]
    for s, (_, blocks, _) in enumerate(ov.RESNET_STAGES, start=1):
        fused_from = 0 if s == 1 else 1
        for b in range(blocks):
            k, kn = f"l{s}.{b}.", f"l{s}.{b + 1}."
            last = s < 4 and b == blocks - 1
            fused = x3 and s < 4 and b >= fused_from
            chain, nxt = fused and s < 3, b + 1 < blocks
            if not fused or b == fused_from:
                t.append((f"out:{k}c1.w", "c1:" + k, False))
            if chain:
                t.append(("chain_out:" + k, "c3:" + k, last))
                if nxt:
                    t.append(("chain_t1n:" + k, "c1:" + kn, False))
            else:
                t.append((f"out:{k}c2.w", "c2:" + k, last))
                if fused and nxt and n_frames * 14 * 14 <= TAIL_PAIR_ROWS:
                    t += [(f"out:{k}c3.wf", "c3:" + k, False), (f"out:{kn}c1.wf", "c1:" + kn, False)]
                elif fused and nxt:
                    t += [("tail_out:" + k, "c3:" + k, False), ("tail_t1n:" + k, "c1:" + kn, False)]
                else:
                    t.append((f"out:{k}{'c3d' if b == 0 else 'c3'}.w", "c3:" + k, last))
            if s == 1 and b == 0:
                t.append(("l1b0_c1", "c1:l1.0.", False))
                if not chain:
                    t.append(("l1b0_c2", "c2:l1.0.", False))
                t.append(("l1b0", "c3:l1.0.", False))
            t.append((f"blk{s}_{b}", f"blk{s}_{b}", last))
        t.append((f"layer{s}", f"layer{s}", s < 4))
    return t + [("avgpool", "avgpool", False), ("out:fc1.w", "feats", False)]


def _tap(eng, name, call, mode, shape, keep=None):
    """One forward (`call`) with `name` armed; the tap as float64 on the host: all of the [n, ...] tensor `shape`, or the frames
    `keep` of it (sliced on the device, the full buffer freed before the copy).  Returns (tap, what the call returned)."""
    kind = _kind(name, mode)
    numel = math.prod(shape)
    dst = eng.debug_tap(name, numel * (2 if kind == "sp32" else 1), dtype=torch.float32 if kind == "f32" else torch.int16)
    out = call()
    torch.cuda.synchronize()
    assert eng.debug_tap_copied() == numel * (2 if kind == "bf16" else 4), (name, MODES[mode], eng.debug_tap_copied(), shape)
    if keep is not None:
        dst = dst.view(shape[0], -1)[list(keep)].contiguous()
        eng._tap_keepalive = None
        shape = (len(keep),) + tuple(shape[1:])
    raw = dst.cpu()
    del dst
    if kind == "sp32":
        got = raw_to_f32(raw, tuple(shape))
    elif kind == "bf16":
        got = (raw.to(torch.int32) << 16).view(torch.float32).view(shape)       # bf16 widened (exact)
    else:
        got = raw.view(shape)
    return got.double(), out


def _family(tap):
    """stem | s<stage>.c (conv1 / conv2 outputs) | s<stage>.blk (block outputs) | head."""
    if tap in ("pre", "stem_conv", "stem", "out:stem.w"):
        return "stem"
    if tap in ("avgpool", "out:fc1.w"):
        return "head"
    if tap.startswith("l1b0"):
        return "s1.blk" if tap == "l1b0" else "s1.c"
    if tap.startswith("layer"):
        return f"s{tap[5]}.blk"
    if tap.startswith("blk"):
        return f"s{tap[3]}.blk"
    stage = tap.split(":l")[1][0]
    if tap.endswith((".c1.w", ".c2.w", ".c1.wf")) or tap.startswith(("chain_t1n:", "tail_t1n:")):
        return f"s{stage}.c"          # a t1n / c1.wf tap is the NEXT block's conv1, of the same stage
    return f"s{stage}.blk"


# max|err| / max|ref| per tap over the compared frames; each bound about 4x the worst tap of its family over cases A-D (measured on
# the MI355X; the tap and the case beside it), no f32-grade bound above 5e-5.
TAP_BOUND = {
    MODE_FP32: {"stem": 2.0e-6,      # measured 4.87e-7 (stem_conv = out:stem.w, A)
                "s1.c": 4.1e-6,      # measured 1.02e-6 (out:l1.2.c1.w, A)
                "s1.blk": 1.9e-6,    # measured 4.62e-7 (blk1_0, A and B)
                "s2.c": 5.6e-6,      # measured 1.40e-6 (out:l2.2.c2.w, A)
                "s2.blk": 3.4e-6,    # measured 8.30e-7 (blk2_0, A and B)
                "s3.c": 9.4e-6,      # measured 2.33e-6 (out:l3.0.c2.w, A)
                "s3.blk": 5.4e-6,    # measured 1.33e-6 (layer3, A and B)
                "s4.c": 9.3e-6,      # measured 2.32e-6 (out:l4.1.c2.w, A)
                "s4.blk": 5.8e-6,    # measured 1.44e-6 (blk4_0, A and B)
                "head": 6.4e-6},     # measured 1.59e-6 (out:fc1.w, A and B)
    MODE_F16X3: {"stem": 1.5e-6,     # measured 3.66e-7 (stem, A and B; 3.60e-7 in C)
                 "s1.c": 2.9e-6,     # measured 7.15e-7 (chain_t1n:l1.0., A and B)
                 "s1.blk": 2.0e-6,   # measured 5.00e-7 (blk1_1 = chain_out:l1.1., A and B)
                 "s2.c": 4.2e-6,     # measured 1.03e-6 (out:l2.0.c2.w, A and B)
                 "s2.blk": 2.6e-6,   # measured 6.37e-7 (blk2_0, A and B)
                 "s3.c": 6.8e-6,     # measured 1.70e-6 (out:l3.3.c2.w, A and B)
                 "s3.blk": 4.6e-6,   # measured 1.15e-6 (blk3_3 = out:l3.3.c3.wf in A, tail_out:l3.3. in B)
                 "s4.c": 8.2e-6,     # measured 2.03e-6 (out:l4.1.c2.w, A and B)
                 "s4.blk": 5.6e-6,   # measured 1.39e-6 (layer4, A and B)
                 "head": 4.4e-6},    # measured 1.10e-6 (out:fc1.w, A and B)
    # bf16 storage and bf16 MFMA operands: 4x measured, no ceiling to cite (case A, the only one this mode runs)
    MODE_BF16: {"stem": 1.4e-2,      # measured 3.35e-3 (stem_conv = out:stem.w; "pre", one bf16 rounding, is at 3.0e-3)
                "s1.c": 3.7e-2,      # measured 9.18e-3 (out:l1.2.c2.w)
                "s1.blk": 2.6e-2,    # measured 6.45e-3 (layer1)
                "s2.c": 4.5e-2,      # measured 1.12e-2 (out:l2.3.c2.w)
                "s2.blk": 3.6e-2,    # measured 8.97e-3 (blk2_2)
                "s3.c": 5.8e-2,      # measured 1.44e-2 (out:l3.0.c2.w)
                "s3.blk": 4.4e-2,    # measured 1.10e-2 (blk3_4)
                "s4.c": 4.5e-2,      # measured 1.11e-2 (out:l4.0.c2.w)
                "s4.blk": 3.7e-2,    # measured 9.25e-3 (blk4_1)
                "head": 1.1e-2},     # measured 2.64e-3 (avgpool)
}
# Frames 0 and 84 come out of the 85-frame call (case B) with the figures of the 2-frame call (case A) to every printed digit, in
# both modes, the fused stage-3 tail against the pair of contractions included: a frame's values do not depend on the batch around
# it.  "pre" is exact in the f32 mode (0.0 in A and C).
# The logits: max|dlogit| < 1e-4 and max|dprob| < 1e-4 in the f32-grade modes as everywhere (measured: f32 1.19e-5 / 2.42e-6 in D,
# x3 1.02e-5 / 6.34e-7 in A), and max|dlogit| / max|logit|: measured 1.15e-6 (f32, D), 9.87e-7 (x3, A and B), 2.81e-3 (bf16, A;
# max|dlogit| 2.89e-2, max|dprob| 6.05e-3)
LOGIT_BOUND = {MODE_FP32: 4.6e-6, MODE_F16X3: 4.0e-6, MODE_BF16: 1.2e-2}
# The LSTM (f32 and x3 modes; n = 3 and 300, two input scales): "proj" = the four contraction outputs, "h1" = lstm_h1, "h2" =
# lstm_h2.  lstm_h1 stands out at the saturating scale only: a gate pre-activation of magnitude 54 carries its contraction's 8e-7
# as 4e-5 absolute, and a gate that is not saturated passes a quarter of that on to h, whose maximum is 1.
LSTM_BOUND = {MODE_FP32: {"proj": 5.5e-6,     # measured 1.36e-6 (out:lstm1.whh.w, n = 300, unit scale)
                          "h1": 3.8e-5,       # measured 9.35e-6 (n = 300, saturating)
                          "h2": 3.5e-6,       # measured 8.72e-7 (n = 300, saturating)
                          "logits": 3.0e-6},  # measured 7.27e-7 (n = 3, saturating)
              MODE_F16X3: {"proj": 4.8e-6,    # measured 1.19e-6 (out:lstm2.whh.w, n = 300, saturating)
                           "h1": 3.8e-5,      # measured 9.54e-6 (n = 300, saturating)
                           "h2": 3.3e-6,      # measured 8.11e-7 (n = 300, saturating)
                           "logits": 2.8e-6}}  # measured 6.87e-7 (n = 3, saturating)
assert max(max(TAP_BOUND[m].values()) for m in F32_GRADE) <= CEILING and max(max(v.values()) for v in LSTM_BOUND.values()) <= CEILING


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _oracle_cnn(sd64, x, hook=None, stem_only=False):
    """{oracle tap: float64, NHWC} of resnet50_forward64 on the preprocessed x [n,3,224,224]; "pre" in the library's 230 x 230 x 4
    layout (oracle/video.py stem64)."""
    taps = {}
    with torch.no_grad():
        if stem_only:
            ov.stem64(sd64, x.double(), taps)
        else:
            ov.resnet50_forward64(sd64, x.double(), taps, hook=hook)
    ref = {k: _nhwc(v) if v.dim() == 4 else v for k, v in taps.items()}
    ref["pre"] = torch.nn.functional.pad(ref["pre"], (0, 1, 0, 1, 0, 1))
    return ref


def _ref_of(ref, orc, sub, rows=None):
    r = ref[orc]
    if rows is not None:
        r = r[list(rows)]
    return r[:, ::2, ::2].contiguous() if sub else r


def measure_cnn(eng, call, ref, mode, taps, n, keep=None, ref_rows=None):
    """{library tap: max|err| / max|ref|} of one input in one mode; `call` runs the forward on all n frames, `keep` are the frames
    compared (with the oracle rows `ref_rows`).  Also the call's last return value."""
    rel, out = {}, None
    for lib, orc, sub in taps:
        r = _ref_of(ref, orc, sub, ref_rows)
        got, out = _tap(eng, lib, call, mode, (n,) + tuple(r.shape[1:]), keep)
        rel[lib] = ((got - r).abs().max() / r.abs().max()).item()
    return rel, out


def _final(out, ref, rows=None, ref_rows=None):
    """(max|dlogit|, max|dlogit| / max|logit|, max|dprob|) of a call's (logits, probs, feats)."""
    lg, pr = out[0].cpu().double(), out[1].cpu().double()
    rl, rp = ref["logits"], ref["probs"]
    if rows is not None:
        lg, pr = lg[list(rows)], pr[list(rows)]
    if ref_rows is not None:
        rl, rp = rl[list(ref_rows)], rp[list(ref_rows)]
    d = (lg - rl).abs().max().item()
    return d, d / rl.abs().max().item(), (pr - rp).abs().max().item()


class _Worst:
    """Worst figure per (mode, tap) with the case that made it; the family report and the assertion."""

    def __init__(self):
        self.tap = {m: {} for m in MODES}
        self.logit = {m: (0.0, 0.0, 0.0, "") for m in MODES}

    def add(self, mode, case, rel, final=None):
        for k, v in rel.items():
            if not v < self.tap[mode].get(k, (-1.0,))[0]:
                self.tap[mode][k] = (v, case)
        if final is not None and not final[1] < self.logit[mode][1]:
            self.logit[mode] = (*final, case)

    def report(self):
        for mode, taps in self.tap.items():
            if not taps:
                continue
            fam = {}
            for k, (v, case) in taps.items():
                if not v < fam.get(_family(k), (-1.0,))[0]:
                    fam[_family(k)] = (v, k, case)
            print(f"{MODES[mode]} worst tap per family:", {f: f"{v:.2e} {k}@{c}" for f, (v, k, c) in sorted(fam.items())})
            print(f"{MODES[mode]} per tap:", {k: f"{v:.1e}@{c}" for k, (v, c) in taps.items()})
            lg = self.logit[mode]
            print(f"{MODES[mode]} final: max|dlogit| {lg[0]:.2e}, relative {lg[1]:.2e}, max|dprob| {lg[2]:.2e} at {lg[3]}")

    def failures(self):
        bad = {}
        for mode, taps in self.tap.items():
            for k, (v, case) in taps.items():
                if not v < TAP_BOUND[mode][_family(k)]:
                    bad[(MODES[mode], k)] = (v, case, TAP_BOUND[mode][_family(k)])
            lg = self.logit[mode]
            if lg[3] and not lg[1] < LOGIT_BOUND[mode]:
                bad[(MODES[mode], "logits")] = lg
            if lg[3] and mode in F32_GRADE and not (lg[0] < 1e-4 and lg[2] < 1e-4):
                bad[(MODES[mode], "final")] = lg
        return bad


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def eng(sd_static, sd_dynamic):
    e = Engine(0)
    e.load_static(sd_static)
    e.load_dynamic(sd_dynamic)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sd64(sd_static):
    return ov.state_dict64(sd_static)


@pytest.fixture(scope="module")
def frames():
    return synth.face_frames(8501, N_B)


def nchw_input(frames2):
    """Case D's input: the preprocessed frames plus a fixed fractional offset pattern in (-0.47, 0.47) (a period of 97 over the
    flattened tensor, float32): |x| < 165, well inside fp16's range, and no value is the difference of an integer and a channel
    mean any more, so the lo halves of the planar fp16 pair image carry bits in every position."""
    x = ov.pth_processing(frames2)
    off = ((torch.arange(x.numel(), dtype=torch.float32) % 97) / 97 - 0.5) * 0.94
    return (x + off.view(x.shape)).contiguous()


@pytest.fixture(scope="module")
def ref_a(sd64, frames):
    """The float64 oracle on frames 0 and 84: the reference of cases A and B, computed once, never modified."""
    t0 = time.time()
    ref = _oracle_cnn(sd64, ov.pth_processing(frames[[0, N_B - 1]]))
    print(f"float64 ResNet-50 on two frames: {time.time() - t0:.1f} s")
    return ref


# ------------------------------------------------------------------------------------------------------------ the CNN
def test_every_tap_two_frames(eng, ref_a, frames):
    """Case A: frames 0 and 84 as a 2-frame call, all three modes, every tap, both frames.  6050 stage-1 positions (47 blocks of
    128 and 34 rows); the stage-3 tails as the pair of contractions; the deep layers on the skinny form."""
    t0 = time.time()
    two = torch.from_numpy(frames[[0, N_B - 1]]).to(eng.device)
    assert 2 * 55 * 55 % 128 == 34 and 2 * 14 * 14 <= TAIL_PAIR_ROWS
    w = _Worst()
    eng.x3_overflow_count(reset=True)
    for mode in MODES:
        rel, out = measure_cnn(eng, lambda: eng.static_forward(two, mode), ref_a, mode, _tap_list(mode, 2, aliases=True), 2)
        w.add(mode, "A", rel, _final(out, ref_a))
        df = (out[2].cpu().double() - ref_a["feats"]).abs().max().item() / ref_a["feats"].abs().max().item()
        assert df < TAP_BOUND[mode]["head"], (MODES[mode], "returned feats", df)
    assert eng.x3_overflow_count(reset=True) == 0
    w.report()
    print(f"case A: {time.time() - t0:.1f} s")
    assert not w.failures(), w.failures()


def test_every_tap_85_frames(eng, ref_a, frames):
    """Case B: all 85 frames in one call, x3 (every tap) and f32 (the block taps): 16660 stage-3 positions, above kTailPairRows,
    so bneck_tail2_kernel runs, with a ragged last tile of 20 rows that lies inside frame 84.  Frames 0 and 84 of each tap are
    compared."""
    t0 = time.time()
    assert N_B * 14 * 14 > TAIL_PAIR_ROWS and N_B * 14 * 14 % 128 == 20 and 20 < 14 * 14
    dev = torch.from_numpy(frames).to(eng.device)
    w = _Worst()
    eng.x3_overflow_count(reset=True)
    for mode in F32_GRADE:
        taps = _tap_list(mode, N_B)
        if mode == MODE_F16X3:
            assert sum(t[0].startswith("tail_out:") for t in taps) == 4 and not any(t[0].endswith(".wf") for t in taps)
        else:
            taps = [t for t in taps if t[0].startswith(("blk", "layer", "stem", "avgpool", "out:fc1"))]
        rel, out = measure_cnn(eng, lambda: eng.static_forward(dev, mode), ref_a, mode, taps, N_B, keep=(0, N_B - 1))
        w.add(mode, "B", rel, _final(out, ref_a, rows=(0, N_B - 1)))
    assert eng.x3_overflow_count(reset=True) == 0
    w.report()
    print(f"case B: {time.time() - t0:.1f} s")
    assert not w.failures(), w.failures()


def test_resize_inside_the_stem_and_the_nchw_entry(eng, sd64, frames):
    """Case C: two 150 x 131 frames: the nearest-neighbour resize inside the stem (k_preprocess in the f32 mode, the fused u8 stem
    in x3) against the oracle's stem on nearest_resize_u8.  Case D: static_forward_nchw on an input whose fp16 lo halves are dense
    (nchw_input): the planar hi / lo image and launch_stem_pool in x3, k_pack_nchw in f32; "stem", logits and probabilities."""
    w = _Worst()
    odd = synth.u8(8502, "odd", (2, 150, 131, 3))
    ref_c = _oracle_cnn(sd64, ov.pth_processing(np.stack([ov.nearest_resize_u8(f) for f in odd])), stem_only=True)
    odd_dev = torch.from_numpy(odd).to(eng.device)
    x = nchw_input(frames[[0, N_B - 1]])
    hi = x.half().float()
    assert ((x - hi) != 0).float().mean().item() > 0.9 and x.abs().max().item() < 200
    ref_d = _oracle_cnn(sd64, x)
    x_dev = x.to(eng.device)
    eng.x3_overflow_count(reset=True)
    for mode in F32_GRADE:
        stem_taps = [t for t in _tap_list(mode, 2) if _family(t[0]) == "stem"]
        assert len(stem_taps) == (1 if mode == MODE_F16X3 else 3)
        rel, _ = measure_cnn(eng, lambda: eng.static_forward(odd_dev, mode), ref_c, mode, stem_taps, 2)
        w.add(mode, "C", rel)
        rel, out = measure_cnn(eng, lambda: eng.static_forward_nchw(x_dev, mode), ref_d, mode, [("stem", "stem", False)], 2)
        w.add(mode, "D", rel, _final(out, ref_d))
    assert eng.x3_overflow_count(reset=True) == 0
    w.report()
    assert not w.failures(), w.failures()


# ------------------------------------------------------------------------------------------------------------ local checks
def test_avgpool_fc1_fc2_from_the_librarys_own_inputs(eng, sd64, frames):
    """What a cumulative tap cannot see: each small launch against float64 of the library's OWN tapped input.
    avgpool_kernel: 48 additions in position order and a division in float32, plus the rounding of the result read back: with
    S = sum|x| every partial sum is at most S, so |err| <= (49 + 2) u S / 49 = 51 u mean|x|.
    fc1 (K = 2048, f32 mode and the bf16 mode, which runs fc1 on the f32 kernel): any summation order of 2048 products and the
    bias is within gamma_2050 (sum|w_i x_i| + |b|).  x3: the sp32 contraction's budget of test_gpu_kernels.py
    test_x3_small_magnitude_activations_keep_the_absolute_bound -- sum_k |w_k| d_k + 2e-6 max|ref| + 2^-25 with d_k the pair error
    of operand k, 2^-25 below 2^-3 and 2^-22 |x_k| above it.
    small_linear_kernel (fc2 + softmax) from the returned feats: gamma_514 (sum|w_i relu(x_i)| + |b|) on the logits,
    probabilities within 1e-6 of the float64 softmax, rows summing to 1 within 1e-6."""
    two = torch.from_numpy(frames[[0, N_B - 1]]).to(eng.device)
    w1, b1, w2, b2 = (sd64[k] for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))
    for mode in MODES:
        call = lambda: eng.static_forward(two, mode)     # noqa: E731
        l4, _ = _tap(eng, "layer4", call, mode, (2, 7, 7, 2048))
        pooled, _ = _tap(eng, "avgpool", call, mode, (2, 2048))
        x = l4.reshape(2, 49, 2048)
        err = (pooled - x.mean(1)).abs()
        lim = 51 * U * x.abs().mean(1)
        print(f"avgpool from layer4, {MODES[mode]}: worst err / bound {(err / lim.clamp_min(1e-300)).max().item():.2f}")
        assert (err <= lim).all(), (MODES[mode], "avgpool", (err / lim).max().item())
        feats, out = _tap(eng, "out:fc1.w", call, mode, (2, 512))
        assert torch.equal(feats, out[2].cpu().double())
        want = pooled @ w1.T + b1
        if mode == MODE_F16X3:
            d = torch.clamp(pooled.abs() * 2.0 ** -22, min=2.0 ** -25)
            lim = d @ w1.abs().T + 2e-6 * want.abs().max() + 2.0 ** -25
        else:
            lim = _gamma(2050) * (pooled.abs() @ w1.abs().T + b1.abs())
        err = (feats - want).abs()
        print(f"fc1 from avgpool, {MODES[mode]}: worst err / bound {(err / lim).max().item():.3f}")
        assert (err <= lim).all(), (MODES[mode], "fc1", (err / lim).max().item())
        _check_fc2(out, (MODES[mode], "case A"), w2, b2)


def _check_fc2(out, what, w2, b2):
    logits, probs, feats = (t.cpu().double() for t in out)
    r = torch.relu(feats)
    want = r @ w2.T + b2
    lim = _gamma(514) * (r @ w2.abs().T + b2.abs())
    err = (logits - want).abs()
    assert (err <= lim).all(), (what, "fc2", (err / lim).max().item())
    assert (probs - torch.softmax(want, dim=1)).abs().max().item() <= 1e-6, what
    assert (probs.sum(1) - 1).abs().max().item() <= 1e-6, what


def test_nan_frame_stays_in_its_row(eng, sd64, frames):
    """static_forward_nchw, f32 mode, three frames, one NaN pixel in frame 1: that frame's feats row is NaN, its probabilities are
    all NaN (small_linear_kernel's ReLU passes NaN on), and frames 0 and 2 are bit-identical to a call without the NaN."""
    x = ov.pth_processing(frames[[0, 1, N_B - 1]])
    bad = x.clone()
    bad[1, 1, 100, 117] = float("nan")
    clean = [t.cpu() for t in eng.static_forward_nchw(x.to(eng.device), MODE_FP32)]
    got = [t.cpu() for t in eng.static_forward_nchw(bad.to(eng.device), MODE_FP32)]
    assert torch.isnan(got[2][1]).any(), "the NaN pixel did not reach feats"
    assert torch.isnan(got[1][1]).all() and torch.isnan(got[0][1]).all()
    for a, b in zip(clean, got):
        assert torch.equal(a[[0, 2]], b[[0, 2]])
    _check_fc2([t[[0, 2]] for t in got], "beside a NaN row", sd64["fc2.weight"], sd64["fc2.bias"])


# ------------------------------------------------------------------------------------------------------------ the LSTM
LSTM_TAPS = (("out:lstm1.wih.w", "xp1"), ("out:lstm1.whh.w", "hp1_t1"), ("lstm_h1", "h1"), ("out:lstm2.wih.w", "xp2"),
             ("out:lstm2.whh.w", "hp2_t1"), ("lstm_h2", "h2"))
LSTM_SCALES = {"unit": 1.5, "saturating": 24.0}       # 1.5: test_gpu_visual.py test_lstm_matches_golden_and_oracle


def lstm_windows(n, scale):
    return np.maximum(synth.centered(8503 + n, "lstm_in", (n, 10, 512), scale), 0).astype(np.float32)


def _lstm_family(tap):
    return {"lstm_h1": "h1", "lstm_h2": "h2"}.get(tap, "proj")


def measure_lstm(eng, ref, win_dev, mode):
    rel, out = {}, None
    n = win_dev.shape[0]
    for lib, orc in LSTM_TAPS:
        r = ref[orc]
        got, out = _tap(eng, lib, lambda: eng.dynamic_forward(win_dev, mode), mode, (n,) + tuple(r.shape[1:]))
        rel[lib] = ((got - r).abs().max() / r.abs().max()).item()
    d = (out.cpu().double() - ref["logits"]).abs().max().item()
    return rel, (d, d / ref["logits"].abs().max().item())


@pytest.fixture(scope="module")
def sd64_dyn(sd_dynamic):
    return ov.state_dict64(sd_dynamic)


def test_lstm_every_tap_against_float64_oracle(eng, sd64_dyn):
    """n = 3 (the skinny recurrent contractions in x3) and n = 300 (tiled, 2 tiles of 128 and 44 rows; 3000 rows in the input
    projections), at the scale the golden test uses and at one where the gates saturate.  In x3 out:lstm2.wih.w reads the sp32 copy
    of h1 the cell kernel writes: it meets the same "proj" bound the f32 mode is held to (asserted below)."""
    t0 = time.time()
    worst = {m: {} for m in F32_GRADE}
    for n in (3, 300):
        for what, scale in LSTM_SCALES.items():
            win = lstm_windows(n, scale)
            ref = {}
            with torch.no_grad():
                ov.lstm_forward64(sd64_dyn, torch.from_numpy(win).double(), ref)
            assert all(torch.isfinite(v).all() for v in ref.values())
            if what == "saturating":
                g = ref["xp1"].clone()
                g[:, 1:] += ref["h1"][:, :-1] @ sd64_dyn["lstm1.weight_hh_l0"].T
                frac = (g.abs() > 20).double().mean().item()
                print(f"n = {n}: {frac:.1%} of layer 1's gate pre-activations beyond +-20, max {g.abs().max().item():.1f}")
                assert frac >= 0.01
            win_dev = torch.from_numpy(win).to(eng.device)
            for mode in F32_GRADE:
                eng.x3_overflow_count(reset=True)
                rel, lg = measure_lstm(eng, ref, win_dev, mode)
                assert eng.x3_overflow_count(reset=True) == 0
                rel["logits"] = lg[1]
                assert lg[0] < 1e-4, (MODES[mode], n, what, lg)
                for k, v in rel.items():
                    if not v < worst[mode].get(k, (-1.0,))[0]:
                        worst[mode][k] = (v, f"n={n},{what}")
    for mode, taps in worst.items():
        print(f"{MODES[mode]} LSTM per tap:", {k: f"{v:.2e}@{c}" for k, (v, c) in taps.items()})
    print(f"LSTM taps: {time.time() - t0:.1f} s")
    for mode, taps in worst.items():
        bad = {k: v for k, v in taps.items() if not v[0] < LSTM_BOUND[mode]["logits" if k == "logits" else _lstm_family(k)]}
        assert not bad, (MODES[mode], bad)
        assert taps["out:lstm2.wih.w"][0] < LSTM_BOUND[MODE_FP32]["proj"], (MODES[mode], taps["out:lstm2.wih.w"])


def test_lstm_cell_from_the_librarys_own_inputs(eng, sd64_dyn):
    """lstm_cell_kernel, one launch isolated: h of step 0 from the tapped xp1[:, 0] (no recurrent term, c_0 = 0), h of step 1 from
    xp1[:, 1], the tapped W_hh h_0 and c recomputed in float64 from step 0.  |h| < 1 and the expression is a handful of roundings
    and two or three library transcendentals per factor: 8 u absolute."""
    for what, scale in LSTM_SCALES.items():
        for n in (3, 300):
            win_dev = torch.from_numpy(lstm_windows(n, scale)).to(eng.device)
            for mode in F32_GRADE:
                call = lambda: eng.dynamic_forward(win_dev, mode)     # noqa: E731
                xp, _ = _tap(eng, "out:lstm1.wih.w", call, mode, (n, 10, 2048))
                hp, _ = _tap(eng, "out:lstm1.whh.w", call, mode, (n, 2048))
                h, _ = _tap(eng, "lstm_h1", call, mode, (n, 10, 512))
                i, f, g, o = xp[:, 0].chunk(4, dim=1)
                c0 = torch.sigmoid(i) * torch.tanh(g)
                e0 = (h[:, 0] - torch.sigmoid(o) * torch.tanh(c0)).abs().max().item()
                i, f, g, o = (xp[:, 1].float() + hp.float()).double().chunk(4, dim=1)      # the kernel's own float32 sum
                c1 = torch.sigmoid(f) * c0 + torch.sigmoid(i) * torch.tanh(g)
                e1 = (h[:, 1] - torch.sigmoid(o) * torch.tanh(c1)).abs().max().item()
                print(f"lstm cell, {MODES[mode]}, n = {n}, {what}: step 0 {e0 / U:.2f} u, step 1 {e1 / U:.2f} u")
                assert e0 <= 8 * U and e1 <= 8 * U, (MODES[mode], n, what, e0 / U, e1 / U)
