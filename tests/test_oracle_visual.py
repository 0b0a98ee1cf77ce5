"""Pins oracle/video.py against vectors produced by the imported reference (tests/golden/make_golden.py)."""
import numpy as np
import torch

from avcer_amd import synth
from oracle import video as ov


def _stats(t):
    t = t.detach().float()
    return np.array([t.mean().item(), t.abs().max().item(), t.std().item()])


def test_preprocess_matches_reference(golden):
    g = golden("static")
    x = ov.pth_processing(synth.face_frames(1234, 8))
    np.testing.assert_array_equal(x.reshape(-1)[:16].numpy(), g["pre_head16"])
    np.testing.assert_allclose(_stats(x), g["pre_stats"], rtol=1e-6)


def test_nearest_resize_matches_pil(golden):
    g = golden("static")
    odd = synth.u8(77, "odd", tuple(g["resize_in_shape"]))
    x = ov.pth_processing(ov.nearest_resize_u8(odd)[None])
    np.testing.assert_array_equal(x[0, :, ::16, ::16].numpy(), g["resize_out"])


def test_resnet50_matches_reference(golden, sd_static):
    g = golden("static")
    taps = {}
    with torch.no_grad():
        logits, feats = ov.resnet50_forward(sd_static, ov.pth_processing(synth.face_frames(1234, 8)), taps)
        probs = torch.softmax(logits, dim=1)
    for k in ("stem", "layer1", "layer2", "layer3", "layer4", "avgpool"):
        np.testing.assert_allclose(taps[k].reshape(-1)[:16].numpy(), g[f"{k}_head16"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(_stats(taps[k]), g[f"{k}_stats"], rtol=1e-5)
    np.testing.assert_allclose(feats.numpy(), g["feats"], atol=2e-5)
    np.testing.assert_allclose(logits.numpy(), g["logits"], atol=2e-5)
    assert np.abs(probs.numpy() - g["probs"]).max() < 1e-6
    assert (probs.argmax(1).numpy() == g["probs"].argmax(1)).all()


def test_lstm_matches_reference(golden, sd_dynamic):
    w = np.maximum(synth.centered(5, "lstm_in", (4, 10, 512), 1.0), 0).astype(np.float32)
    w[0] = w[0, 0]
    with torch.no_grad():
        lo = ov.lstm_forward(sd_dynamic, torch.from_numpy(w))
    assert np.abs(lo.numpy() - golden("lstm")["logits"]).max() < 1e-6


def test_visual_harness_matches_reference(golden, sd_static, sd_dynamic):
    g = golden("visual_harness")
    clip = synth.face_frames(4321, 16)
    for name in ("gap25", "gap30", "lead25", "full25"):
        present = g[f"{name}_present"]
        fps = float(g[f"{name}_fps"])
        st, dy = ov.visual_forward(sd_static, sd_dynamic, clip, present, fps)
        assert st.dtype == g[f"{name}_static"].dtype and dy.dtype == g[f"{name}_dynamic"].dtype
        assert np.abs(st - g[f"{name}_static"]).max() < 5e-6
        assert np.abs(dy - g[f"{name}_dynamic"]).max() < 1e-5
        # batched CNN evaluation is the same function up to reduction order
        st_b, dy_b = ov.visual_forward(sd_static, sd_dynamic, clip, present, fps, batched=True)
        assert np.abs(st_b - st).max() < 1e-5 and np.abs(dy_b - dy).max() < 1e-4


def test_lstm_step_rounding():
    assert [ov.lstm_step(f) for f in (24, 25, 29, 30, 60, 12.5)] == [5, 5, 6, 6, 12, 2]


U32 = 2.0 ** -24


def test_float64_resnet_agrees_with_float32_oracle(sd_static):
    """resnet50_forward64 restates resnet50_forward: in float64 it differs from the float32 forward by float32 rounding alone.
    Bound: under the probabilistic rounding model (Higham & Mary 2019) a float32 contraction of K terms is off by about sqrt(K) u
    of its output's magnitude; K <= 4608 (3 x 3 x 512) and at most 53 contractions precede any tap (49 convolutions in the main
    path + 4 shortcut ones + fc1 + fc2 at the logits: 55), their contributions adding at worst linearly (BatchNorm, ReLU and the
    pools have gain <= 1 relative to a tensor's maximum): max|err| <= 55 sqrt(4608) u max|ref| = 2.2e-4 max|ref|.  A wrong
    stride, eps, pad or shortcut shows at 1e-2 or more."""
    frames = synth.face_frames(1234, 2)
    x = ov.pth_processing(frames)
    t32, t64 = {}, {}
    with torch.no_grad():
        lg32, ft32 = ov.resnet50_forward(sd_static, x, t32)
        lg64, ft64 = ov.resnet50_forward64(ov.state_dict64(sd_static), x.double(), t64)
    assert lg64.dtype == torch.float64 and t64["blk3_5"].dtype == torch.float64
    bound = 55 * np.sqrt(4608) * U32
    t32.update(feats=ft32, logits=lg32, probs=torch.softmax(lg32, dim=1))
    for k, r32 in t32.items():
        rel = ((t64[k].float() - r32).abs().max() / r32.abs().max()).item()
        assert rel < bound, (k, rel, bound)
    # the final taps are the return values; a block's "c3:" is its output; the last block's output is the stage's
    assert t64["logits"] is lg64 and t64["feats"] is ft64
    assert torch.equal(t64["probs"], torch.softmax(lg64, dim=1))
    for li, (_, blocks, _) in enumerate(ov.RESNET_STAGES, start=1):
        assert t64[f"layer{li}"] is t64[f"blk{li}_{blocks - 1}"] is t64[f"c3:l{li}.{blocks - 1}."]
    assert tuple(t64["pre"].shape) == (2, 3, 229, 229) and torch.equal(t64["pre"][:, :, 2:226, 2:226], x.double())
    assert tuple(t64["stem_conv"].shape) == (2, 64, 112, 112) and tuple(t64["c2:l3.5."].shape) == (2, 256, 14, 14)
    # a 3x3 / stride-2 / pad-1 convolution is the stride-1 one at even positions: what lets "c2:" serve the strided last blocks
    a = torch.nn.functional.conv2d(t64["c1:l1.2."], ov.state_dict64(sd_static)["layer1.2.conv2.weight"], None, 2, 1)
    b = torch.nn.functional.conv2d(t64["c1:l1.2."], ov.state_dict64(sd_static)["layer1.2.conv2.weight"], None, 1, 1)
    assert (a - b[:, :, ::2, ::2]).abs().max().item() <= 1e-12 * b.abs().max().item()


def test_float64_lstm_agrees_with_float32_oracle(sd_dynamic):
    """lstm_forward64 against lstm_forward on 4 windows.  Same model of the bound: 23 contractions (2 input projections, 18
    recurrent ones, fc; K <= 512) and 20 cells whose gates have slope <= 1: 43 sqrt(512) u max|ref| = 5.8e-5 max|ref|."""
    w = np.maximum(synth.centered(5, "lstm_in", (4, 10, 512), 1.0), 0).astype(np.float32)
    taps = {}
    with torch.no_grad():
        lo32 = ov.lstm_forward(sd_dynamic, torch.from_numpy(w))
        lo64 = ov.lstm_forward64(ov.state_dict64(sd_dynamic), torch.from_numpy(w).double(), taps)
    rel = ((lo64.float() - lo32).abs().max() / lo32.abs().max()).item()
    assert rel < 43 * np.sqrt(512) * U32, rel
    assert taps["logits"] is lo64 and lo64.dtype == torch.float64
    assert {k: tuple(v.shape) for k, v in taps.items()} == {
        "xp1": (4, 10, 2048), "hp1_t1": (4, 2048), "h1": (4, 10, 512), "xp2": (4, 10, 1024), "hp2_t1": (4, 1024), "h2": (4, 256),
        "logits": (4, 7)}
    # step 0 has no recurrent term; step 1's is hp1_t1
    sd64 = ov.state_dict64(sd_dynamic)
    assert torch.allclose(taps["hp1_t1"], taps["h1"][:, 0] @ sd64["lstm1.weight_hh_l0"].T, rtol=0, atol=1e-13)
