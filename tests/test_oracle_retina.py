"""The oracle's RetinaFace-R50 restatement against vectors produced by the reference's own RetinaFace class
(FPN / SSH / heads unmodified; torchvision backbone restated in the harness) -- tests/golden/make_golden.py gen_face_net."""
import numpy as np
import pytest
import torch

from avcer_amd import synth
from oracle import face as of
from oracle import retina as orf


@pytest.fixture(scope="module")
def sd_retina():
    return synth.to_torch(synth.retina_state_dict(42))


@pytest.mark.parametrize("name", ["a", "b"])
def test_network_matches_reference_class(golden, sd_retina, name):
    g = golden("face_net")
    h, w = (int(v) for v in g[f"{name}_size"])
    frame = synth.video_frames(900, 1, h, w)[0]
    loc, conf, lm = orf.retina_forward(sd_retina, orf.preprocess(frame))
    assert loc.shape[1] == len(of.prior_boxes((h, w)))            # one row per anchor of PriorBox
    np.testing.assert_allclose(loc[0].numpy(), g[f"{name}_loc"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(conf[0].numpy(), g[f"{name}_conf"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(lm[0].numpy(), g[f"{name}_landms"], rtol=0, atol=2e-5)


def test_intermediate_statistics(golden, sd_retina):
    g = golden("face_net")
    frame = synth.video_frames(900, 1, 96, 128)[0]
    with torch.no_grad():
        feats = orf.backbone(sd_retina, orf.preprocess(frame))
        pyr = orf.fpn(sd_retina, feats)
    for k, t in (("body1", feats[0]), ("body2", feats[1]), ("body3", feats[2]), ("fpn1", pyr[0]), ("fpn3", pyr[2])):
        st = np.array([t.mean().item(), t.abs().max().item(), t.std().item()])
        np.testing.assert_allclose(st, g[f"a_{k}_stats"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(t.reshape(-1)[:16].numpy(), g[f"a_{k}_head16"], rtol=0, atol=2e-5)


def _tap_names():
    """Every tensor the library can tap on the detector (detect.hip face_forward_lane / visual.hip run_bneck_stage), "face_" prefix dropped."""
    names = {"pool", "l1b0_c2", "layer1", "body1", "body2", "body3", "lat1", "lat2", "lat3", "sum2", "fpn2", "fpn1", "ssh1"}
    for li, (_, blocks, _) in enumerate(orf.STAGES, start=1):
        names |= {f"blk{li}_{b}" for b in range(blocks)} | {f"c1:l{li}.{b}." for b in range(blocks)}
    return names


def test_taps_and_float64_forward_match_reference_class(golden, sd_retina):
    """The tap-filling forward that the detector's stage-tap tests compare against (tests/test_gpu_retina_stages.py): arming
    taps changes no output, the float64 form reproduces the reference class's vectors, and every tap is the tensor its name
    says -- stage outputs are their last block's output, a block's conv1 tap follows from the previous block's output, sum2 is
    merge2's input and the taps agree with the golden statistics of the backbone and the FPN."""
    g = golden("face_net")
    for name in ("a", "b"):
        h, w = (int(v) for v in g[f"{name}_size"])
        frame = synth.video_frames(900, 1, h, w)[0]
        x = orf.preprocess(frame)
        taps = {}
        for plain, tapped in zip(orf.retina_forward(sd_retina, x), orf.retina_forward(sd_retina, x, taps)):
            assert torch.equal(plain, tapped)
        t64 = {}
        loc, conf, lm = orf.retina_forward64(sd_retina, frame, t64)
        assert set(taps) == set(t64) == _tap_names()
        assert all(t.dtype == torch.float64 for t in (loc, conf, lm, *t64.values()))
        # the vectors carry the reference's own f32 rounding: measured 1.2e-5 (loc, landms), 2.9e-6 (conf)
        np.testing.assert_allclose(loc[0].numpy(), g[f"{name}_loc"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(conf[0].numpy(), g[f"{name}_conf"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(lm[0].numpy(), g[f"{name}_landms"], rtol=0, atol=2e-5)
    # the float64 taps of frame "a" (96 x 128): wiring and golden statistics
    frame = synth.video_frames(900, 1, *(int(v) for v in g["a_size"]))[0]
    t = {}
    orf.retina_forward64(sd_retina, frame, t)
    sd = {k: v.double() for k, v in sd_retina.items() if v.is_floating_point()}
    for stage, last in (("layer1", "blk1_2"), ("body1", "blk2_3"), ("body2", "blk3_5"), ("body3", "blk4_2")):
        assert torch.equal(t[stage], t[last])
    with torch.no_grad():
        c1 = torch.relu(orf._bn(torch.nn.functional.conv2d(t["blk3_2"], sd["body.layer3.3.conv1.weight"]), sd, "body.layer3.3.bn1"))
        up = torch.nn.functional.interpolate(t["lat3"], size=t["lat2"].shape[2:], mode="nearest")
    assert torch.equal(t["c1:l3.3."], c1)
    assert torch.equal(t["sum2"], t["lat2"] + up)
    assert t["pool"].shape == (1, 64, 24, 32) and t["ssh1"].shape == t["fpn1"].shape == (1, 256, 12, 16)
    for k, ref in (("body1", "body1"), ("body2", "body2"), ("body3", "body3"), ("fpn1", "fpn1"), ("lat3", "fpn3")):
        st = np.array([t[k].mean().item(), t[k].abs().max().item(), t[k].std().item()])
        np.testing.assert_allclose(st, g[f"a_{ref}_stats"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(t[k].reshape(-1)[:16].numpy(), g[f"a_{ref}_head16"], rtol=0, atol=2e-5)
