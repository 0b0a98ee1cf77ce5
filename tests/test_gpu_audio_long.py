"""Audio windows longer than 256 tokens on the GPU (Engine.load_audio(sd, max_tokens=1024)): ExprModelV3 and ExprModelV1 at 257
and 400 tokens against the float64 oracle, tap by tap with the bounds of tests/test_gpu_audio_stages.py; batch and pass-boundary
invariance; the unchanged bits of windows up to 256 tokens; the limits; run_inference(window=8).

Bounds of the taps: TAP_BOUND / LOGIT_BOUND of test_gpu_audio_stages.py (measured there up to 256 tokens).  Past 256 tokens the
reference's own float32 arithmetic (oracle/audio.py in float32 on the CPU) is measured against float64 at the same tap and length,
and a tap's bound is max(the table's, 2 x that error): the rule of tests/test_gpu_attention_long.py.  V1 runs the same trunk
launches as V3 (checked per launch in the V3 cases): its case compares the trunk's output, both GRU layers and the head, with
test_gpu_expr_v1.test_stage_taps_against_float64's bound (5e-5 of max(|ref|, 1)) under the same rule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_v1_oracle as v1  # noqa: E402
import test_gpu_audio_stages as stages  # noqa: E402
from avcer_amd import run as arun  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd._lib import AvcerError  # noqa: E402
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine  # noqa: E402
from avcer_amd.fusion import WEIGHTS_AV_1  # noqa: E402
from avcer_amd.models import AudioModel  # noqa: E402
from oracle import audio as oa  # noqa: E402
from oracle import fusion as ofu  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = stages.MODES
LENGTHS = {257: 82320, 400: 128080}  # tokens: samples
MAX_TOKENS = 1024
PASS_400 = 128 * 256 // 400          # windows per pass at 400 tokens (include/avcer_hip.h): 81


@pytest.fixture(scope="module")
def eng_long(sd_audio):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    eng = Engine(0)
    eng.load_audio(sd_audio, max_tokens=MAX_TOKENS)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def sd_v1():
    return synth.to_torch(synth.audio_v1_state_dict(44))


@pytest.fixture(scope="module")
def eng_v1_long(sd_v1):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    eng = Engine(0)
    eng.load_audio(sd_v1, max_tokens=MAX_TOKENS)
    yield eng
    eng.close()


def _own_error(ref64, ref32, name):
    """max|err| / max|ref| of the float32 oracle against the float64 one at a tap"""
    return ((ref32[name].double() - ref64[name]).abs().max() / ref64[name].abs().max()).item()


_V3_REF = {}


def _v3_reference(sd_audio, tokens):
    """(wav, float64 taps, float32 taps) of the V3 case at `tokens`, computed once for both modes"""
    if tokens not in _V3_REF:
        wav = synth.waveforms(7701 + tokens, 2, LENGTHS[tokens])
        ref64 = stages._oracle(oa.state_dict64(sd_audio), wav)
        ref32 = {}
        with torch.no_grad():
            lg = oa.expr_model_v3_forward(sd_audio, torch.from_numpy(oa.normalize(wav)), ref32)
        ref32["logits"] = lg.reshape(2, -1)
        _V3_REF[tokens] = (wav, ref64, ref32)
    return _V3_REF[tokens]


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
@pytest.mark.parametrize("tokens", list(LENGTHS))
def test_v3_every_tap_against_float64(eng_long, sd_audio, tokens, mode):
    wav, ref64, ref32 = _v3_reference(sd_audio, tokens)
    taps = stages._tap_list(False, middle_out=False)
    rel, (dlogit, rlogit) = stages.measure_case(eng_long, ref64, wav, mode, taps)
    worst, bad = {}, []
    for lib, orc in taps:
        fam = stages._family(lib)
        own = _own_error(ref64, ref32, orc) if orc != "norm" else 0.0
        bound = max(stages.TAP_BOUND[mode][fam], 2 * own)
        if rel[lib] > worst.get(fam, (0.0,))[0]:
            worst[fam] = (rel[lib], lib, bound, own)
        if not rel[lib] < bound:
            bad.append((lib, rel[lib], bound))
    print(f"V3 {tokens} tokens {MODES[mode]}: worst tap per family (max|err|/max|ref|, tap, bound, float32 oracle's own):")
    for fam, w in worst.items():
        print(f"   {fam:12s} {w[0]:.2e} {w[1]} bound {w[2]:.2e} own {w[3]:.2e}")
    own_l = _own_error(ref64, ref32, "logits")
    print(f"   logits max|d| {dlogit:.2e} rel {rlogit:.2e} (float32 oracle's own rel {own_l:.2e})")
    assert not bad, bad
    assert dlogit < 1e-4 and rlogit < max(stages.LOGIT_BOUND[mode], 2 * own_l)
    out = eng_long.audio_forward(torch.from_numpy(wav), True, mode).cpu().double()
    assert torch.equal(out.argmax(1), ref64["logits"].argmax(1))
    assert (torch.softmax(out, 1) - torch.softmax(ref64["logits"], 1)).abs().max().item() < 1e-4


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
@pytest.mark.parametrize("tokens", list(LENGTHS))
def test_v1_stage_taps_against_float64(eng_v1_long, sd_v1, tokens, mode):
    wav = synth.waveforms(7801 + tokens, 2, LENGTHS[tokens])
    ref64, ref32 = {}, {}
    lg64 = v1.expr_model_v1_forward64(oa.state_dict64(sd_v1), wav, ref64).reshape(2, -1)
    with torch.no_grad():
        v1.expr_model_v1_forward(sd_v1, torch.from_numpy(oa.normalize(wav)), ref32)
    report = []
    for name in ("w2v", "gru1", "gru2", "td0", "mp", "td4", "pooled"):
        ref = ref64[name]
        dst = eng_v1_long.debug_tap(name, ref.numel())
        out = eng_v1_long.audio_forward(torch.from_numpy(wav), True, mode)
        torch.cuda.synchronize()
        assert eng_v1_long.debug_tap_copied() == ref.numel() * 4, name
        err = (dst.cpu().view(ref.shape).double() - ref).abs().max().item()
        own = (ref32[name].double() - ref).abs().max().item()
        report.append((name, err, max(5e-5 * max(ref.abs().max().item(), 1.0), 2 * own), own))
    print(f"V1 {tokens} tokens {MODES[mode]} (tap, max|err|, bound, float32 oracle's own):", report)
    for name, err, bound, _ in report:
        assert err < bound, report
    out = out.cpu().double()
    assert (out - lg64).abs().max().item() < 1e-4 and torch.equal(out.argmax(1), lg64.argmax(1))
    assert (torch.softmax(out, 1) - torch.softmax(lg64, 1)).abs().max().item() < 1e-4


@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
def test_a_window_does_not_depend_on_its_batch(eng_long, eng_v1_long, mode):
    """Alone, among three, and on both sides of the pass boundary at 400 tokens (82 windows = one pass of 81 and one window)."""
    t = LENGTHS[400]
    few = torch.from_numpy(synth.waveforms(31, 3, t))
    wav = few[torch.arange(PASS_400 + 1) % 3].contiguous()
    for eng in (eng_long, eng_v1_long):
        big = eng.audio_forward(wav, True, mode).cpu()
        assert torch.isfinite(big).all()
        three = eng.audio_forward(few, True, mode).cpu()
        assert torch.equal(three, big[:3])
        for i in range(3):
            assert torch.equal(eng.audio_forward(few[i:i + 1], True, mode).cpu()[0], three[i])
        for i in (PASS_400 - 1, PASS_400):
            assert torch.equal(big[i], three[i % 3]), i


@pytest.mark.parametrize("t", [32000, 64000])
def test_short_windows_keep_their_bits(eng_long, engine_audio, t):
    """99 and 199 tokens: a model loaded for long windows returns what a default-loaded one does, bit for bit."""
    wav = torch.from_numpy(synth.waveforms(32, 3, t))
    for mode in MODES:
        assert torch.equal(eng_long.audio_forward(wav, True, mode).cpu(), engine_audio.audio_forward(wav, True, mode).cpu())


def test_limits(eng_long, engine_audio, sd_audio):
    assert eng_long.audio_max_tokens == MAX_TOKENS and engine_audio.audio_max_tokens == 256
    with pytest.raises(AvcerError, match="1025 tokens"):
        eng_long.audio_forward(torch.zeros(1, 1025 * 320 + 80), True, MODE_FP32)
    with pytest.raises(AvcerError):
        engine_audio.audio_forward(torch.from_numpy(synth.waveforms(1, 1, 82320)), True, MODE_FP32)  # 257 tokens, default engine
    # the setter itself: range, and the rows of the loaded pe
    for bad in (255, 5001, MAX_TOKENS + 1):
        assert eng_long.lib.avcer_set_audio_max_tokens(eng_long.ctx, bad) != 0
    assert eng_long.audio_max_tokens == MAX_TOKENS
    with pytest.raises(ValueError, match="max_tokens"):
        arun.run_inference(engine_audio, np.zeros((2, 8, 8, 3), np.uint8), np.zeros(16000, np.float32), 25,
                           detections=[np.zeros((0, 5))] * 2, window=8)


def test_audio_model_takes_long_windows(sd_audio):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    eng = Engine(0)
    try:
        model = AudioModel(eng, sd_audio, mode=MODE_FP32, max_tokens=MAX_TOKENS)
        x = torch.from_numpy(oa.normalize(synth.waveforms(33, 2, LENGTHS[257])))
        one, two = model(x[0]), model(x)
        assert tuple(one.shape) == (8,) and tuple(two.shape) == (2, 8) and torch.equal(one.cpu(), two.cpu()[0])
    finally:
        eng.close()


def test_run_inference_with_an_8_s_window(sd_static, sd_dynamic, sd_audio):
    """window=8 (399 tokens): the audio table and the fusion against the oracle's audio model and fusion on the same windows
    (the visual probabilities are the run's own: tests/test_gpu_run.py holds them to the visual oracle)."""
    from test_face_cpu import golden_frames, golden_script

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    eng = Engine(0)
    try:
        eng.load_static(sd_static)
        eng.load_dynamic(sd_dynamic)
        eng.load_audio(sd_audio, max_tokens=400)
        frames, script = golden_frames(), golden_script()
        total, fps, sr = len(frames), 25, 16000
        wav = synth.waveforms(98, 1, int(total / fps * sr))[0]
        out = arun.run_inference(eng, frames, wav, fps, detections=script, weights_prob_model=WEIGHTS_AV_1, ce_weights_type=False,
                                 ce_mask=True, window=8, step=1, mode=MODE_F16X3)
        a_rows, a_frames = oa.audio_forward(sd_audio, torch.from_numpy(wav), sr, fps, 8, 1, "mean")
        np.testing.assert_array_equal(out["audio_frames"], a_frames)
        assert np.abs(ofu.softmax(out["audio_rows"][:, :7]) - ofu.softmax(a_rows[:, :7])).max() < 1e-4
        prob, am = ofu.fuse(out["static_probs"].astype(np.float32), out["dynamic_logits"].astype(np.float32), a_rows, a_frames,
                            WEIGHTS_AV_1, (1, 1, 1), False, True)
        assert np.abs(out["compound_prob"] - prob).max() < 1e-4
        for i, name in enumerate(("av", "vs", "vd", "a")):
            np.testing.assert_array_equal(out[name], am[i])
    finally:
        eng.close()
