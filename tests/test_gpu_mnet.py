"""The MobileNet-0.25 RetinaFace detector on the GPU (csrc/mnet.hip): the network against the reference's golden outputs and the
float64 restatement, the conv_dw kernel block by block, batching, lanes, the predictor chain and switching between the detectors."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mnet_ref
from avcer_amd import face_tiles as ft
from avcer_amd import run as arun
from avcer_amd import synth
from avcer_amd.engine import MODE_BF16, MODE_F16X3, MODE_FP32, Engine
from oracle import face as of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "face_net_mnet.npz"))
MODES = [(MODE_FP32, "fp32"), (MODE_F16X3, "x3")]
SHAPES = [(8, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1)]


@pytest.fixture(scope="module")
def sd_mnet():
    return synth.to_torch(synth.retina_mnet_state_dict(42))


@pytest.fixture(scope="module")
def eng(sd_mnet):
    """An engine of this module's own: the session's shared engine keeps whatever detector the other modules loaded."""
    e = Engine(0)
    try:
        e.load_face(sd_mnet)
        yield e
    finally:
        e.close()


def _gates(got, want, what):
    (loc, conf, lm), (rl, rc, rm) = got, want
    d = [float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) for a, b in ((conf, rc), (loc, rl), (lm, rm))]
    print(f"{what}: max|d conf| {d[0]:.2e}  max|d loc| {d[1]:.2e}  max|d landms| {d[2]:.2e}")
    assert d[0] < 1e-4 and d[1] < 1e-3 and d[2] < 1e-3, (what, d)


def _np(ts):
    return [t.cpu().numpy() for t in ts]


# ---- 1
@pytest.mark.parametrize("mode,mname", MODES)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_network_matches_the_reference_golden(eng, name, mode, mname):
    h, w = (int(v) for v in GOLD[f"{name}_size"])
    assert eng.face_kind() == 2
    got = [t[0] for t in _np(eng.face_forward(synth.video_frames(900, 1, h, w), mode))]
    _gates(got, [GOLD[f"{name}_loc"], GOLD[f"{name}_conf"], GOLD[f"{name}_landms"]], f"golden {name} {mname}")
    assert eng.x3_overflow_count() == 0


# ---- 2
def _block(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
    return dict(dw_w=r(9, cin) * (2.0 / 9) ** 0.5, dw_s=u(0.6, 1.4, cin), dw_b=u(-0.1, 0.1, cin), pw_w=r(cout, cin) * (2.0 / cin) ** 0.5,
                pw_s=u(0.6, 1.4, cout), pw_b=u(-0.1, 0.1, cout))


def _block_ref(p, x_nhwc, stride, dtype):
    c = lambda t: t.to(dtype)
    cin = x_nhwc.shape[-1]
    x = c(x_nhwc).permute(0, 3, 1, 2)
    t = F.conv2d(x, c(p["dw_w"]).t().reshape(cin, 1, 3, 3), stride=stride, padding=1, groups=cin)
    t = F.leaky_relu(t * c(p["dw_s"]).view(1, -1, 1, 1) + c(p["dw_b"]).view(1, -1, 1, 1), 0.1)
    y = F.conv2d(t, c(p["pw_w"]).view(*p["pw_w"].shape, 1, 1))
    y = F.leaky_relu(y * c(p["pw_s"]).view(1, -1, 1, 1) + c(p["pw_b"]).view(1, -1, 1, 1), 0.1)
    return y.permute(0, 2, 3, 1).contiguous(), t


@pytest.mark.parametrize("mode,mname", MODES)
@pytest.mark.parametrize("cin,cout,stride", SHAPES)
def test_dwsep_block_against_float64(eng, cin, cout, stride, mode, mname):
    """One conv_dw block per launch against the float64 restatement of the same block, two frames, at 1 x 1, 5 x 7 and the extent
    whose OUTPUT is 9 x 9 -- one row and one column past the kernel's 8 x 8 output tile (input 9 x 9 at stride 1, 17 x 17 at
    stride 2).  Gate: 4 x the error of an f32 CPU torch evaluation of the same block against float64 (max abs / max|ref|): a
    different summation order is the only legitimate difference."""
    p = _block(cin, cout, 1000 * cin + cout + stride)
    for h, w in ((1, 1), (5, 7), (8 * stride + 1, 8 * stride + 1)):
        x = torch.randn(2, h, w, cin, generator=torch.Generator().manual_seed(h * 100 + w))
        ref, _ = _block_ref(p, x, stride, torch.float64)
        cpu32, _ = _block_ref(p, x, stride, torch.float32)
        got = eng.dwsep(x, p["dw_w"], p["dw_s"], p["dw_b"], p["pw_w"], p["pw_s"], p["pw_b"], stride, mode).cpu()
        assert got.shape == ref.shape
        scale = float(ref.abs().max())
        e32 = float((cpu32.double() - ref).abs().max()) / scale
        err = float((got.double() - ref).abs().max()) / scale
        print(f"dwsep {cin}->{cout} s{stride} {h}x{w} {mname}: kernel {err:.2e}  f32 cpu {e32:.2e}")
        assert err <= 4 * e32, (h, w, err, e32)
    assert eng.x3_overflow_count() == 0


@pytest.mark.parametrize("cin,cout,stride", [(32, 64, 2), (256, 256, 1)])
def test_dwsep_x3_small_magnitude_keeps_the_absolute_bound(eng, cin, cout, stride):
    """Depthwise outputs of whole-tensor magnitude 1e-3: the lo half of such a pair is an fp16 subnormal, an element carries an
    absolute error of at most 2^-25, and the pointwise contraction stays within sum_k |w_k| * 2^-25 of the exact result plus the
    f32 accumulation's own error (the bound of test_x3_small_magnitude_activations_keep_the_absolute_bound)."""
    p = _block(cin, cout, 7)
    p["pw_s"], p["pw_b"] = torch.ones(cout), torch.zeros(cout)
    x = torch.randn(2, 9, 9, cin, generator=torch.Generator().manual_seed(3)) * 1e-3
    p["dw_b"] = p["dw_b"] * 1e-3
    ref, t = _block_ref(p, x, stride, torch.float64)
    assert 1e-4 < float(t.abs().max()) < 2e-2
    got = eng.dwsep(x, p["dw_w"], p["dw_s"], p["dw_b"], p["pw_w"], p["pw_s"], p["pw_b"], stride, MODE_F16X3).cpu()
    bound = 2.0 ** -25
    err = float((got.double() - ref).abs().max())
    budget = float(p["pw_w"].abs().sum(1).max()) * bound + 2e-6 * float(ref.abs().max()) + bound
    print(f"dwsep {cin}->{cout} small magnitude: max|err| {err:.2e} (budget {budget:.2e})")
    assert err <= budget


# ---- 3
@pytest.mark.parametrize("h,w,n", [(150, 214, 3), (70, 33, 2)])
def test_x3_against_f32_mode_and_restatement(eng, sd_mnet, h, w, n):
    frames = synth.video_frames(31, n, h, w)
    x3 = _np(eng.face_forward(frames, MODE_F16X3))
    f32 = _np(eng.face_forward(frames, MODE_FP32))
    ref = [t.numpy() for t in mnet_ref.mnet_forward64(sd_mnet, frames)]
    _gates(x3, f32, f"{h}x{w} x3 vs fp32")
    _gates(x3, ref, f"{h}x{w} x3 vs float64")
    _gates(f32, ref, f"{h}x{w} fp32 vs float64")
    for mode, whole in ((MODE_F16X3, x3), (MODE_FP32, f32)):
        alone = _np(eng.face_forward(frames[1:2], mode))
        for a, b in zip(alone, whole):
            np.testing.assert_array_equal(a[0], b[1])  # a frame's result does not depend on the batch around it
        rgb = _np(eng.face_forward(np.ascontiguousarray(frames[..., ::-1]), mode, rgb=True))
        for a, b in zip(rgb, whole):
            np.testing.assert_array_equal(a, b)
    assert eng.x3_overflow_count() == 0


def test_x3_against_f32_mode_at_360x640(eng):
    frames = synth.video_frames(32, 2, 360, 640)
    x3, f32 = _np(eng.face_forward(frames, MODE_F16X3)), _np(eng.face_forward(frames, MODE_FP32))
    assert x3[1].shape == (2, 2 * (45 * 80 + 23 * 40 + 12 * 20), 2) and np.isfinite(x3[1]).all()
    _gates(x3, f32, "360x640 x3 vs fp32")


# ---- 4
@pytest.mark.parametrize("mode,mname", MODES)
def test_two_lanes_are_bit_identical(eng, mode, mname):
    frames = synth.video_frames(21, 21, 96, 128)
    try:
        eng.set_static_lanes(1)
        one = [t.clone() for t in eng.face_forward(frames, mode)]
        eng.set_static_lanes(2)
        for _ in range(2):
            two = eng.face_forward(frames, mode)
            assert all(torch.equal(a, b) for a, b in zip(one, two))
    finally:
        eng.set_static_lanes(2)


# ---- 5
def test_predictor_chain_matches_oracle_chain(eng, sd_mnet):
    frame = synth.video_frames(5, 1, 120, 160)[0]
    rl, rc, rm = mnet_ref.mnet_forward(sd_mnet, mnet_ref.preprocess(frame))
    ref = of.detections(rl[0].numpy(), rc[0].numpy(), rm[0].numpy(), (120, 160), threshold=0.5)
    assert 0 < ref.shape[0] < rl.shape[1]  # holds for the restatement alone: some rows, not all priors
    pred = ft.RetinaFacePredictor(eng, sd_mnet, threshold=0.5, mode=MODE_FP32)
    got = pred(frame, rgb=False)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-2)      # pixels
    frames = synth.video_frames(11, 4, 96, 128)
    together = pred.batch(frames, rgb=False)
    for t in range(4):
        np.testing.assert_array_equal(together[t], pred(frames[t], rgb=False))


# ---- 6
def test_switching_detectors_leaves_nothing_behind(sd_mnet):
    sd_r50 = synth.to_torch(synth.retina_state_dict(42))
    frames = synth.video_frames(77, 2, 64, 96)
    e = Engine(0)
    try:
        assert e.face_kind() == 0
        e.load_face(sd_r50)
        assert e.face_kind() == 1
        first = [t.clone() for t in e.face_forward(frames, MODE_F16X3)]
        try:
            e.load_face(sd_mnet)
            assert e.face_kind() == 2
            m1 = [t.clone() for t in e.face_forward(frames, MODE_F16X3)]
            m2 = [t.clone() for t in e.face_forward(frames, MODE_FP32)]
            assert all(torch.isfinite(t).all() for t in m1 + m2)
        finally:
            e.load_face(sd_r50)
        assert e.face_kind() == 1
        again = e.face_forward(frames, MODE_F16X3)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        e.load_face(sd_mnet)
        assert all(torch.equal(a, b) for a, b in zip(m1, e.face_forward(frames, MODE_F16X3)))
        e.load_face(sd_r50)
    finally:
        e.close()


# ---- 7
def test_errors(eng):
    with pytest.raises(Exception, match="AVCER_MODE_BF16"):
        eng.face_forward(np.zeros((1, 64, 64, 3), np.uint8), MODE_BF16)
    with pytest.raises(Exception):
        eng.face_forward(np.zeros((1, 16, 16, 3), np.uint8), MODE_FP32)
    assert eng.face_kind() == 2


# ---- 8
def test_run_inference_with_the_mnet_detector(sd_mnet, engine, sd_static, sd_dynamic, sd_audio):
    """run_inference(detector=...) with the MobileNet detector equals run_inference(detections=...) fed that detector's own rows."""
    e = Engine(0)
    try:
        e.load_static(sd_static)
        e.load_dynamic(sd_dynamic)
        e.load_audio(sd_audio)
        pred = ft.RetinaFacePredictor(e, sd_mnet, threshold=0.9, mode=MODE_F16X3)
        frames = synth.video_frames(13, 12, 96, 128)
        wav = synth.waveforms(99, 1, int(12 / 25 * 16000))[0]
        dets = pred.batch(frames, rgb=False)
        assert sum(len(d) for d in dets) > 0
        a = arun.run_inference(e, frames, wav, 25, detector=pred, mode=MODE_F16X3)
        b = arun.run_inference(e, frames, wav, 25, detections=dets, mode=MODE_F16X3)
        for key in ("static_probs", "dynamic_logits", "audio_rows", "compound_prob", "av", "records"):
            np.testing.assert_array_equal(a[key], b[key])
    finally:
        e.close()


# ---- 9
NECK_TAPS = ("body1", "body2", "body3", "fpn1", "fpn2", "fpn3", "ssh1")


@pytest.fixture(scope="module")
def neck_ref(sd_mnet):
    """Two 75 x 101 frames and the taps of the restatement in float64 and in f32 on the CPU, NHWC like the library's."""
    frames = synth.video_frames(75, 2, 75, 101)
    t64, t32 = {}, {}
    mnet_ref.mnet_forward64(sd_mnet, frames, t64)
    mnet_ref.mnet_forward(sd_mnet, torch.cat([mnet_ref.preprocess(f) for f in frames]), t32)
    nhwc = lambda taps: {k: taps[k].permute(0, 2, 3, 1).contiguous().double() for k in NECK_TAPS}
    return frames, nhwc(t64), nhwc(t32)


@pytest.mark.parametrize("mode,mname", MODES)
def test_neck_taps_against_float64(eng, neck_ref, mode, mname):
    """The body's three outputs, the pyramid and level 1's SSH output (csrc/detect.hip run_neck), tap by tap against float64,
    both frames in full.  75 x 101 frames: pyramid extents 10 x 13, 5 x 7 and 3 x 4, odd at every level, and nearest-upsample
    ratios 5/10 and 3/5 of which one is no whole number.  Activations are NHWC f32 in both modes.  Gate, as in
    test_dwsep_block_against_float64: max|err| / max|ref| of a tap within 4 x that of the f32 CPU restatement."""
    frames, t64, t32 = neck_ref
    assert [tuple(t64[k].shape[1:3]) for k in ("fpn1", "fpn2", "fpn3")] == [(10, 13), (5, 7), (3, 4)]
    bad = []
    for name in NECK_TAPS:
        ref = t64[name]
        dst = eng.debug_tap("face_" + name, ref.numel())
        eng.face_forward(frames, mode)
        assert eng.debug_tap_copied() == ref.numel() * 4, name
        scale = float(ref.abs().max())
        e32 = float((t32[name] - ref).abs().max()) / scale
        err = float((dst.cpu().view(ref.shape).double() - ref).abs().max()) / scale
        print(f"mnet tap {name} {mname}: library {err:.2e}  f32 cpu {e32:.2e}")
        if not err <= 4 * e32:
            bad.append((name, err, e32))
    assert not bad, bad
    assert eng.x3_overflow_count() == 0
