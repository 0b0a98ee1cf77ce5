"""The GRU-head audio model ExprModelV1 on the GPU: the recurrence kernel alone (avcer_gru_layer, csrc/gru.hip) against a
float64 restatement, the whole model against the reference's golden logits and the float64 oracle (tests/expr_v1_oracle.py),
its stage taps, batch invariance, launch counts, the features entry point, head switching on one context and the pipelines."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_v1_oracle as v1  # noqa: E402
from avcer_amd import audio_pipeline, synth  # noqa: E402
from avcer_amd import run as arun  # noqa: E402
from avcer_amd._lib import AvcerError  # noqa: E402
from avcer_amd.engine import MODE_BF16, MODE_F16X3, MODE_FP32, Engine  # noqa: E402
from avcer_amd.fusion import WEIGHTS_AV7_1, WEIGHTS_AV7_2  # noqa: E402
from avcer_amd.models import AudioModel  # noqa: E402
from oracle import audio as oa  # noqa: E402

pytestmark = pytest.mark.gpu
F32_GRADE = ((MODE_FP32, "fp32"), (MODE_F16X3, "x3"))


@pytest.fixture(scope="module")
def sd8():
    return synth.audio_v1_state_dict(44)


@pytest.fixture(scope="module")
def eng_v1(sd8):
    eng = Engine(0)
    eng.load_audio(sd8)
    assert eng.audio_head_kind == 1 and eng.audio_classes == 8
    yield eng
    eng.close()


# ---- the recurrence kernel alone
@pytest.mark.parametrize("mode,mname", F32_GRADE)
@pytest.mark.parametrize("n,s", [(1, 1), (1, 99), (5, 2), (5, 199), (16, 99), (33, 1), (33, 2), (33, 199), (16, 199), (1, 199),
                                 (5, 99), (33, 99), (16, 1), (16, 2), (1, 2), (5, 1)])
def test_gru_layer_against_float64(eng_v1, n, s, mode, mname):
    """avcer_gru_layer on random input projections, W_hh and biases at the synthetic scale (+-1/16).  The yardstick is the
    reference arithmetic's own rounding: the float32 restatement's error against float64 on the same inputs; the device's
    error over the whole [n, S, 256] sequence has to stay within 8 x that (another summation order over K = 256 and the
    device's exp / tanh, compounding over the steps as the CPU's do).  n = 5 and 33: partial tiles; S = 1: the step with h_0 = 0."""
    seed = 1000 * n + s
    xp = synth.centered(seed, "gru.xp", (n, s, 768), 0.6)
    w = synth.uniform(seed, "gru.whh", (768, 256), -1 / 16, 1 / 16)
    b = synth.uniform(seed, "gru.bhh", (768,), -1 / 16, 1 / 16)
    txp, tw, tb = torch.from_numpy(xp), torch.from_numpy(w), torch.from_numpy(b)
    with torch.no_grad():
        ref64 = v1.gru_layer(txp.double(), tw.double(), tb.double())
        ref32 = v1.gru_layer(txp, tw, tb)
    own = (ref32.double() - ref64).abs().max().item()
    got = eng_v1.gru_layer(txp, tw, tb, mode=mode).cpu()
    assert tuple(got.shape) == (n, s, 256) and torch.isfinite(got).all()
    err = (got.double() - ref64).abs().max().item()
    msg = f"gru_layer {mname} n={n} S={s}: device error {err:.3e}, float32 restatement's own error {own:.3e}, ratio {err / own:.2f}"
    print(msg)
    assert err <= 8 * own, msg


def test_gru_layer_refuses_other_hidden_sizes(eng_v1):
    x = torch.zeros(1, 2, 768, device="cuda")
    rc = eng_v1.lib.avcer_gru_layer(eng_v1.ctx, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 2, 128, MODE_FP32, x.data_ptr(), None)
    assert rc != 0 and b"256" in eng_v1.lib.avcer_last_error(eng_v1.ctx)


# ---- whole model
def _probs(lg):
    return torch.softmax(torch.from_numpy(np.asarray(lg, np.float32).reshape(-1, lg.shape[-1])), 1).numpy()


@pytest.mark.parametrize("classes,seed,case", [(8, 44, "t32000"), (8, 44, "t64000"), (7, 45, "c7_t32000"), (7, 45, "c7_t64000")])
def test_whole_model_against_golden_and_oracle(golden, classes, seed, case):
    """2 s and 4 s windows, 8- and 7-class models: the reference's golden logits where the fixture holds them (8 classes at both
    lengths, 7 classes at 2 s) and the float32 oracle everywhere.  One gate for the two f32-grade modes, as for ExprModelV2 / V3."""
    g = golden("audio_model_v1")
    sd = synth.audio_v1_state_dict(seed, classes)
    t = 64000 if case.endswith("64000") else 32000
    wav = {"t32000": synth.waveforms(6678, 2, 32000), "t64000": synth.waveforms(6679, 1, 64000),
           "c7_t32000": synth.waveforms(6680, 2, 32000), "c7_t64000": synth.waveforms(6681, 2, 64000)}[case]
    assert wav.shape[1] == t
    with torch.no_grad():
        ref = v1.expr_model_v1_forward(synth.to_torch(sd), torch.from_numpy(oa.normalize(wav))).numpy().reshape(-1, classes)
    refs = [("oracle", ref)]
    if f"{case}_logits" in g.files:
        refs.append(("golden", g[f"{case}_logits"].reshape(-1, classes)))
    eng = Engine(0)
    try:
        eng.load_audio(sd)
        assert eng.audio_classes == classes and eng.audio_head_kind == 1
        for mode, mname in F32_GRADE:
            out = eng.audio_forward(torch.from_numpy(wav), normalize=True, mode=mode).cpu().numpy()
            assert out.shape == ref.shape
            for rname, r in refs:
                dl, dp = np.abs(out - r).max(), np.abs(_probs(out) - _probs(r)).max()
                print(f"V1 {case} {mname} vs {rname}: max|dlogit| {dl:.3e} max|dprob| {dp:.3e}")
                assert dl < 1e-4 and dp < 1e-4, (case, mname, rname, dl, dp)
        out = eng.audio_forward(torch.from_numpy(wav), normalize=True, mode=MODE_BF16).cpu().numpy()
        dp = np.abs(_probs(out) - _probs(ref)).max()
        print(f"V1 {case} bf16: max|dprob| {dp:.3e}")
        assert np.isfinite(out).all() and dp < 0.1
        assert eng.x3_overflow_count() == 0
    finally:
        eng.close()


@pytest.mark.parametrize("mode,mname", F32_GRADE)
def test_stage_taps_against_float64(eng_v1, sd8, mode, mname):
    wav = synth.waveforms(6678, 2, 32000)
    taps = {}
    v1.expr_model_v1_forward64(oa.state_dict64(synth.to_torch(sd8)), wav, taps)
    report = []
    for name in ("gru1", "gru2", "td0", "mp", "td4", "pooled"):
        ref = taps[name]
        dst = eng_v1.debug_tap(name, ref.numel())
        eng_v1.audio_forward(torch.from_numpy(wav), normalize=True, mode=mode)
        torch.cuda.synchronize()
        assert eng_v1.debug_tap_copied() == ref.numel() * 4, name
        err = (dst.cpu().view(ref.shape).double() - ref).abs().max().item()
        report.append((name, err, ref.abs().max().item()))
    print(f"V1 stage taps {mname} (name, max|err| vs float64, max|ref|):", report)
    for name, err, mx in report:
        assert err < 5e-5 * max(mx, 1.0), report


@pytest.mark.parametrize("mode,mname", F32_GRADE)
def test_batch_invariance(eng_v1, mode, mname):
    """Row i of a 128-window call, the same window alone, and in a batch of 17: the same bits."""
    wav = torch.from_numpy(synth.waveforms(13, 128, 32000))
    big = eng_v1.audio_forward(wav, True, mode).cpu()
    assert torch.isfinite(big).all()
    for i in (0, 77, 127):
        assert torch.equal(eng_v1.audio_forward(wav[i:i + 1], True, mode).cpu()[0], big[i]), (mname, i)
    lo = 70
    mid = eng_v1.audio_forward(wav[lo:lo + 17], True, mode).cpu()
    assert torch.equal(mid, big[lo:lo + 17]), mname


def test_launch_count_does_not_depend_on_the_steps(eng_v1, sd_audio):
    """The profile counts the MFMA launches (contractions and the recurrence): the same NUMBER for 99 and for 199 steps, two of
    them the recurrence's (which FORM of the contraction serves a layer -- skinny, tiled, weights-direct -- follows the row count,
    so the per-family split of the trunk's launches differs between the two lengths, as it does for ExprModelV3); the head is
    what follows the trunk's contractions: at most 12 launches by the source's own count (split, 2 x (projection + recurrence),
    td0, max-pool, td4, mean, linear = 10), 6 of them MFMA launches."""
    counts = {}
    for t in (32000, 64000):
        wav = torch.from_numpy(synth.waveforms(21, 1, t))
        eng_v1.audio_forward(wav, True, MODE_F16X3)
        eng_v1.profile_enable(True)
        eng_v1.audio_forward(wav, True, MODE_F16X3)
        fam = eng_v1.profile_read_families()
        eng_v1.profile_enable(False)
        counts[t] = {k: v[1] for k, v in fam.items()}
        assert counts[t]["gru_layer_kernel"] == 2
    total = sum(counts[32000].values())
    assert total == sum(counts[64000].values()), counts
    eng3 = Engine(0)
    try:
        eng3.load_audio(sd_audio)
        wav = torch.from_numpy(synth.waveforms(21, 1, 32000))
        eng3.audio_forward(wav, True, MODE_F16X3)
        eng3.profile_enable(True)
        eng3.audio_forward(wav, True, MODE_F16X3)
        total3 = sum(v[1] for v in eng3.profile_read_families().values())
    finally:
        eng3.close()
    # ExprModelV3's head: 2 x (qkv, attention is no contraction, o, ff1, ff2) + td0 + td4 = 10 contractions behind the same trunk
    head = total - (total3 - 10)
    print("MFMA launches: V1", total, "V3", total3, "V1 head", head)
    assert head == 6 and head <= 12


def test_features(golden, sd8, sd_audio):
    g = golden("audio_model_v1")
    for sd, width in ((sd8, 256), (sd_audio, 1024)):
        eng = Engine(0)
        try:
            eng.load_audio(sd)
            wav = torch.from_numpy(synth.waveforms(6678, 2, 32000))
            for mode, mname in F32_GRADE:
                plain = eng.audio_forward(wav, True, mode).cpu()
                dst = eng.debug_tap("pooled", 2 * width)
                lg, feats = eng.audio_forward(wav, True, mode, return_features=True)
                torch.cuda.synchronize()
                assert tuple(feats.shape) == (2, width) and eng.debug_tap_copied() == 2 * width * 4
                assert torch.equal(feats.cpu().reshape(-1), dst.cpu()), (width, mname)   # the pooled tap's bytes
                assert torch.equal(lg.cpu(), plain), (width, mname)                       # the same logits, bit for bit
            if width == 256:
                model = AudioModel(eng, sd)
                x = torch.from_numpy(oa.normalize(synth.waveforms(6678, 2, 32000)))
                lg, feats = model.get_features(x)
                ref = g["t32000_features"]
                err = np.abs(feats.cpu().numpy() - ref).max()
                print("get_features max|err| vs the reference's", err)
                assert tuple(feats.shape) == (2, 256) and err < 5e-5 * max(np.abs(ref).max(), 1.0)
                assert np.abs(lg.cpu().numpy() - g["t32000_logits"]).max() < 1e-4
                lg1, f1 = model.get_features(x[0])
                assert tuple(lg1.shape) == (8,) and tuple(f1.shape) == (256,)
                assert tuple(model(x[0]).shape) == (8,)
        finally:
            eng.close()


def test_head_switch_on_one_context(sd8, sd_audio):
    eng = Engine(0)
    try:
        assert eng.audio_head_kind == 0
        wav = torch.from_numpy(synth.waveforms(6678, 2, 32000))
        kinds, v3 = [], []
        eng.load_audio(sd_audio)
        kinds.append(eng.audio_head_kind)
        v3.append([eng.audio_forward(wav, True, m).cpu() for m, _ in F32_GRADE])
        eng.load_audio(sd8)
        kinds.append(eng.audio_head_kind)
        a = [eng.audio_forward(wav, True, m).cpu() for m, _ in F32_GRADE]
        assert all(torch.isfinite(t).all() for t in a)
        eng.load_audio(sd_audio)
        kinds.append(eng.audio_head_kind)
        v3.append([eng.audio_forward(wav, True, m).cpu() for m, _ in F32_GRADE])
        assert kinds == [3, 1, 3]
        for x, y in zip(*v3):
            assert torch.equal(x, y)
        # a blob with neither head is refused with a message
        from avcer_amd import packing
        p = packing.pack_audio(sd8)
        blob = packing.to_blob({k: v for k, v in p.items() if not k.startswith("gru")})
        import ctypes as C
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        rc = eng.lib.avcer_load_audio(eng.ctx, C.cast(buf, C.c_void_p), len(blob))
        assert rc != 0 and b"neither" in eng.lib.avcer_last_error(eng.ctx) and eng.audio_head_kind == 0
        with pytest.raises(AvcerError):
            eng.audio_forward(wav, True, MODE_FP32)
    finally:
        eng.close()


def test_audio_pipeline_with_v1(eng_v1, sd8):
    """9.3 s of audio through the chunker and ExprModelV1, against the oracle chain; the empty tail window is NaN on both sides."""
    wav = torch.from_numpy(synth.waveforms(78, 1, 148800)[0])
    eng_v1.x3_overflow_clear()
    logits, lo, hi = audio_pipeline.audio_forward(eng_v1, wav, 16000, 25, window=4, step=0.5, padding="mean")
    rows, frames = audio_pipeline.replicate_per_frame(logits.cpu().numpy(), lo, hi)
    ref_rows, ref_frames = v1.audio_forward_v1(synth.to_torch(sd8), wav, 16000, 25, 4, 0.5, "mean")
    np.testing.assert_array_equal(frames, ref_frames)
    ok = ~np.isnan(ref_rows).any(axis=1)
    assert np.array_equal(ok, ~np.isnan(rows).any(axis=1)) and ok.sum() > 0
    err = np.abs(rows[ok] - ref_rows[ok]).max()
    print("V1 chunked audio max|dlogit|", err, "rows", len(rows), "NaN rows", int((~ok).sum()))
    assert err < 2e-4
    assert eng_v1.x3_overflow_count() == 0


def test_run_inference_with_seven_class_v1(sd_static, sd_dynamic):
    """run.run_inference in the 7-class audio configuration (ExprModelV2's place taken by a 7-column ExprModelV1; padding
    "repeat", step 1, the Acl7 weights: get_pred_av.py:362-365)."""
    from test_face_cpu import golden_frames, golden_script

    eng = Engine(0)
    try:
        eng.load_static(sd_static)
        eng.load_dynamic(sd_dynamic)
        eng.load_audio(synth.audio_v1_state_dict(45, 7))
        frames, script = golden_frames(), golden_script()
        total, fps = len(frames), 25
        wav = synth.waveforms(99, 1, int(total / fps * 16000) + 37)[0]
        eng.x3_overflow_clear()
        out = arun.run_inference(eng, frames, wav, fps, detections=script, weights_prob_model=WEIGHTS_AV7_1,
                                 weights_model=WEIGHTS_AV7_2, padding="repeat", step=1, mode=MODE_F16X3)
        assert out["audio_rows"].shape[1] == 7 and np.isfinite(out["audio_rows"]).all()
        assert out["compound_prob"].shape == (4, total, 7) and np.isfinite(out["compound_prob"]).all()
        assert out["av"].shape == (total,)
        assert eng.x3_overflow_count() == 0
    finally:
        eng.close()
