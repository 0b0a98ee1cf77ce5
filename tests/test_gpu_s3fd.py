"""The S3FD detector on the GPU (csrc/s3fd.hip): its three kernels against float64, the network against the reference's golden
outputs in both modes, batching, Detect on the device, the predictor, the argument checks, switching detectors and run_inference."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import s3fd_ref
from avcer_amd import face_tiles as ft
from avcer_amd import run as arun
from avcer_amd import synth
from avcer_amd.engine import MODE_BF16, MODE_F16X3, MODE_FP32, Engine
from avcer_amd.sp32 import from_sp32, raw_to_f32, to_sp32

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "s3fd_net.npz"))
DET = np.load(os.path.join(HERE, "golden", "s3fd_detect.npz"))
MODES = [(MODE_FP32, "fp32"), (MODE_F16X3, "x3")]
TAPS = {"conv1": 64, "pool3": 256, "conv3_3": 256, "conv4_3": 512, "conv5_3": 512, "fc7": 1024, "ex1": 512, "ex3": 256}
EPS = 2.0 ** -24  # unit roundoff of f32


@pytest.fixture(scope="module")
def sd_s3fd():
    return synth.to_torch(synth.s3fd_state_dict(42))


@pytest.fixture(scope="module")
def eng(sd_s3fd):
    """An engine of this module's own: the session's shared engine keeps whatever detector the other modules loaded."""
    e = Engine(0)
    try:
        e.load_face(sd_s3fd)
        yield e
    finally:
        e.close()


def _frame(name):
    h, w = (int(v) for v in GOLD[f"{name}_size"])
    return synth.video_frames(900, 1, h, w)


def _tap_shape(name, h, w):
    fm = ft.s3fd_feature_maps(h, w)
    hw = {"conv1": (h, w), "conv3_3": fm[0], "pool3": fm[1], "conv4_3": fm[1], "conv5_3": fm[2], "fc7": fm[3], "ex1": fm[4], "ex3": fm[5]}[name]
    return (1, hw[0], hw[1], TAPS[name])


# ---- 1: the stem kernel
@pytest.mark.parametrize("sp32", [False, True])
def test_stem_kernel_against_float64(eng, sp32):
    """conv1_1 from the u8 frame, both `rgb` values; the second frame's border pixels are 0 / 255 alternately, so a tap read from
    outside the frame (instead of skipped) or a missing mean subtraction at the edge shows.  Bound: 27 products and 28 additions
    in f32 -- (27 + 2) eps * sum |x w| + |b| -- plus, in sp32 storage, the pair's 2^-22 relative representation error."""
    g = torch.Generator().manual_seed(5)
    wt = torch.randn(64, 3, 3, 3, generator=g) * 0.02
    b = torch.randn(64, generator=g) * 0.1
    frames = synth.video_frames(3, 2, 19, 23).copy()
    edge = np.zeros((19, 23), bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    frames[1][edge] = np.where((np.arange(edge.sum()) % 2)[:, None] == 0, 0, 255).astype(np.uint8)
    packed = wt.permute(2, 3, 1, 0).reshape(27, 64).contiguous()
    for rgb in (False, True):
        x = torch.cat([s3fd_ref.preprocess(f, rgb, torch.float64) for f in frames])
        ref = F.relu(F.conv2d(x, wt.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
        mag = (F.conv2d(x.abs(), wt.double().abs(), padding=1) + b.double().abs().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
        got = eng.s3fd_stem(frames, packed, b, rgb=rgb, sp32=sp32).cpu()
        got = from_sp32(got) if sp32 else got
        assert got.shape == ref.shape
        err = (got.double() - ref).abs()
        bound = 29 * EPS * mag + (2.0 ** -22 * ref.abs() + 2.0 ** -25 if sp32 else 0.0)
        print(f"stem rgb={rgb} sp32={sp32}: max err {float(err.max()):.2e}, max err/bound {float((err / bound).max()):.2f}")
        assert bool((err <= bound).all())


# ---- 2: the 2x2 max-pool
@pytest.mark.parametrize("sp32", [False, True])
@pytest.mark.parametrize("h,w", [(19, 25), (8, 6), (5, 1), (1, 7)])
def test_maxpool2_is_exact(eng, h, w, sp32):
    """Odd extents with and without ceil_mode, a 1-wide and a 1-high map: a maximum of stored values is exact in either storage."""
    x = torch.randn(2, h, w, 64, generator=torch.Generator().manual_seed(h * 31 + w))
    xs = to_sp32(x) if sp32 else x
    xv = from_sp32(xs) if sp32 else x
    for ceil_mode in (False, True):
        if not ceil_mode and (h < 2 or w < 2):
            with pytest.raises(Exception, match="no 2 x 2 window"):
                eng.maxpool2(xs, ceil_mode, sp32)
            continue
        ref = F.max_pool2d(xv.permute(0, 3, 1, 2), 2, 2, ceil_mode=ceil_mode).permute(0, 2, 3, 1)
        got = eng.maxpool2(xs, ceil_mode, sp32).cpu()
        got = from_sp32(got) if sp32 else got
        assert torch.equal(got, ref.contiguous())


# ---- 3: the head kernel
def _head_ref64(x, w_loc, b_loc, w_conf, b_conf, l2w):
    """s3fd_net.py:121-157 for one level in float64 on NHWC x: L2Norm (if l2w), loc / conf 3x3, level 0's max-out, softmax."""
    xc = x.double().permute(0, 3, 1, 2)
    if l2w is not None:
        xc = s3fd_ref.l2norm(xc, l2w.double())
    loc = F.conv2d(xc, w_loc.double(), b_loc.double(), padding=1).permute(0, 2, 3, 1)
    conf = F.conv2d(xc, w_conf.double(), b_conf.double(), padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(xc.abs(), torch.cat([w_loc, w_conf]).double().abs(), padding=1).permute(0, 2, 3, 1)  # sum |x w| per output
    if conf.shape[-1] == 4:
        conf = torch.cat((conf[..., 0:3].max(dim=-1, keepdim=True)[0], conf[..., 3:]), dim=-1)
    n = x.shape[0]
    return loc.reshape(n, -1, 4), F.softmax(conf.reshape(n, -1, 2), dim=-1), mag.reshape(n, -1, mag.shape[-1])


@pytest.mark.parametrize("sp32", [False, True])
@pytest.mark.parametrize("case", ["level0", "l2_edge", "plain"])
def test_head_kernel_against_float64(eng, case, sp32):
    """level0: 8 outputs, max-out, L2Norm over 256 channels on a 9 x 13 map (two tiles per row, the second 5 wide);
    l2_edge: an L2Norm level of 512 channels with one all-zero position (contributes 0, no NaN) and one of magnitude 1e-4;
    plain: 1024 channels (four channel groups per lane) on a 1 x 2 map.
    Bound on loc: a lane adds 9 c / 64 products in f32, the butterfly six more sums, the bias one: (9 c / 64 + 8) eps sum |x w|;
    an L2Norm level also carries the inverse norm's error (c / 64 + 6 additions, a square root, a division, the product with x:
    (c / 128 + 6) eps relative) and the packed weight's own rounding (eps).  conf = softmax of two logits with that error d each:
    |d conf| <= d / 2 + 4 eps."""
    c, no, (h, w), l2 = {"level0": (256, 8, (9, 13), True), "l2_edge": (512, 6, (4, 5), True), "plain": (1024, 6, (1, 2), False)}[case]
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(2, h, w, c, generator=g).relu()
    if case == "l2_edge":
        x[0, 1, 2] = 0.0
        x[1, 2, 3] *= 1e-4 / float(x[1, 2, 3].norm())
    xs = to_sp32(x) if sp32 else x
    xv = from_sp32(xs) if sp32 else x
    w_loc, b_loc = torch.randn(4, c, 3, 3, generator=g) / (9 * c) ** 0.5, torch.randn(4, generator=g) * 0.1
    w_conf, b_conf = torch.randn(no - 4, c, 3, 3, generator=g) * 3 / (9 * c) ** 0.5, torch.randn(no - 4, generator=g)
    l2w = (torch.rand(c, generator=g) * 4 + 8) if l2 else None
    wall = torch.cat([w_loc, w_conf])
    if l2:
        wall = wall * l2w.view(1, c, 1, 1)
    packed = wall.permute(2, 3, 1, 0).reshape(9, c, no).contiguous()
    rl, rc, mag = _head_ref64(xv, w_loc, b_loc, w_conf, b_conf, l2w)
    loc, conf = (t.cpu().double() for t in eng.s3fd_head(xs, packed, torch.cat([b_loc, b_conf]), l2, sp32))
    assert torch.isfinite(loc).all() and torch.isfinite(conf).all()
    gamma = (9 * c / 64 + 8 + ((c / 128 + 6) + 1 if l2 else 0)) * EPS
    babs = torch.cat([b_loc, b_conf]).abs().double()
    d = gamma * (mag + babs)                                # per output, [n, hw, no]
    e_loc = (loc - rl).abs()
    e_conf = (conf - rc).abs()
    d_conf = d[..., 4:].max(dim=-1)[0][..., None] / 2 + 4 * EPS  # two logits, each within its d: conf moves by at most (d0 + d1) / 4
    print(f"head {case} sp32={sp32}: loc err {float(e_loc.max()):.2e} (x bound {float((e_loc / d[..., :4]).max()):.2f}), "
          f"conf err {float(e_conf.max()):.2e} (x bound {float((e_conf / d_conf).max()):.2f})")
    assert bool((e_loc <= d[..., :4]).all())
    assert bool((e_conf <= d_conf).all())


# ---- 4: the whole network
@pytest.mark.parametrize("mode,mname", MODES)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_network_matches_the_reference_golden(eng, name, mode, mname):
    """conf within 1e-4 and loc within 1e-3 of the reference's own S3FDNet, the project's detector gates; the eight taps against
    the recorded statistics (1e-4 relative: f32-grade sums of at most 9216 terms, against a wrong layer's O(1))."""
    frame = _frame(name)
    h, w = frame.shape[1:3]
    assert eng.face_kind() == 3
    loc, conf, lm = eng.face_forward(frame, mode)
    assert lm is None and tuple(loc.shape) == (1, len(GOLD[f"{name}_loc"]), 4)
    d_conf = float(np.abs(conf[0].cpu().numpy().astype(np.float64) - GOLD[f"{name}_conf"]).max())
    d_loc = float(np.abs(loc[0].cpu().numpy().astype(np.float64) - GOLD[f"{name}_loc"]).max())
    print(f"golden {name} {mname}: max|d conf| {d_conf:.2e}  max|d loc| {d_loc:.2e}")
    assert d_conf < 1e-4 and d_loc < 1e-3
    for tap in TAPS:
        shape = _tap_shape(tap, h, w)
        numel = int(np.prod(shape))
        raw = eng.debug_tap("s3fd_" + tap, numel * (2 if mode == MODE_F16X3 else 1), torch.int16 if mode == MODE_F16X3 else torch.float32)
        eng.face_forward(frame, mode)
        assert eng.debug_tap_copied() == numel * 4, tap
        t = (raw_to_f32(raw.cpu(), shape) if mode == MODE_F16X3 else raw.cpu().reshape(shape)).permute(0, 3, 1, 2).contiguous()
        mean, amax, std = GOLD[f"{name}_{tap}_stats"]
        np.testing.assert_allclose([float(t.mean()), float(t.abs().max()), float(t.std())], [mean, amax, std], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(t.reshape(-1)[:16].numpy(), GOLD[f"{name}_{tap}_head16"], rtol=0, atol=1e-4 * max(1.0, amax))
    assert eng.x3_overflow_count() == 0


@pytest.mark.parametrize("mode,mname", MODES)
def test_a_frame_does_not_depend_on_its_batch(eng, mode, mname):
    frames = synth.video_frames(41, 3, 77, 101)
    whole = eng.face_forward(frames, mode)
    alone = eng.face_forward(frames[1:2], mode)
    assert torch.equal(alone[0][0], whole[0][1]) and torch.equal(alone[1][0], whole[1][1])
    rgb = eng.face_forward(np.ascontiguousarray(frames[..., ::-1]), mode, rgb=True)
    assert torch.equal(rgb[0], whole[0]) and torch.equal(rgb[1], whole[1])


# ---- 5: Detect and the predictor
@pytest.mark.parametrize("which", ["full", "trunc"])
def test_s3fd_detect_reproduces_the_reference(eng, which):
    """Same count, same rows in the same order; boxes within rtol 3e-6 / atol 3e-5 (expf is at most 2 ulp apart: the tolerance
    tests/test_gpu_face.py applies to decode rows), scores equal.  The fixture's generator asserted the margins that make every
    keep decision safe under that difference, so no row is excluded."""
    h, w = (int(v) for v in DET["size"])
    rows, cnt = eng.s3fd_detect(DET["loc"], DET["conf"], DET["priors"], (h, w), nms_top_k=int(DET[f"{which}_nms_top_k"]),
                                threshold=float(DET["threshold"]))
    cnt = cnt.cpu().numpy()
    np.testing.assert_array_equal(cnt, DET[f"{which}_counts"])
    for t in range(4):
        want = DET[f"{which}_dets{t}"]
        got = rows[t, :int(cnt[t])].cpu().numpy()
        np.testing.assert_array_equal(got[:, 4], want[:, 4])
        np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=3e-6, atol=3e-5)
    one, c1 = eng.s3fd_detect(DET["loc"][3], DET["conf"][3], DET["priors"], (h, w), nms_top_k=int(DET[f"{which}_nms_top_k"]),
                              threshold=float(DET["threshold"]))
    assert int(c1[0]) == cnt[3] and torch.equal(one[0, :cnt[3]], rows[3, :cnt[3]])  # a frame alone and in the batch


def test_s3fd_detect_top_k_cut_and_limits(eng):
    """Detect keeps min(count, top_k) before the threshold loop; the limits of avcer_face_nms hold here too."""
    h, w = (int(v) for v in DET["size"])
    full, cf = eng.s3fd_detect(DET["loc"], DET["conf"], DET["priors"], (h, w), threshold=float(DET["threshold"]))
    cut, cc = eng.s3fd_detect(DET["loc"], DET["conf"], DET["priors"], (h, w), threshold=float(DET["threshold"]), top_k=3)
    for t in range(4):
        k = min(int(cf[t]), 3)
        assert int(cc[t]) == k and torch.equal(cut[t, :k], full[t, :k])
    for bad in (dict(nms_top_k=6145), dict(top_k=1025)):
        with pytest.raises(Exception, match="s3fd_detect"):
            eng.s3fd_detect(DET["loc"], DET["conf"], DET["priors"], (h, w), **bad)


@pytest.mark.parametrize("mode,mname", MODES)
def test_predictor_reproduces_the_recorded_detections(eng, sd_s3fd, mode, mname):
    pred = ft.S3FDPredictor(eng, sd_s3fd, threshold=0.5, mode=mode)
    assert pred.kind == 3 and pred.gflop_per_frame == 144.27
    total = 0
    for name in ("a", "b", "c"):
        frame = _frame(name)[0]
        want = GOLD[f"{name}_dets"]
        got = pred(frame, rgb=False)
        assert got.dtype == np.float32 and got.shape == want.shape
        # the network's own error moves a score by < 1e-4 and a box by < 1e-3 of a prior's size: pixels within 2e-2
        np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=0, atol=1e-4)
        np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=1e-4, atol=2e-2)
        np.testing.assert_array_equal(pred(np.ascontiguousarray(frame[..., ::-1]), rgb=True), got)
        total += len(want)
    assert total > 0
    frames = synth.video_frames(11, 3, 65, 97)
    together = pred.batch(frames, rgb=False)
    for t in range(3):
        np.testing.assert_array_equal(together[t], pred(frames[t], rgb=False))


# ---- 6: argument checks and switching
def test_errors(eng):
    frames = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=eng.device)
    loc, conf, lm = eng._new(1, 342, 4), eng._new(1, 342, 2), eng._new(1, 342, 10)
    call = lambda f, h, w, mode, landms: eng.lib.avcer_face_forward(eng.ctx, f.data_ptr(), 1, h, w, 0, mode, loc.data_ptr(), conf.data_ptr(),
                                                                    landms, eng._stream())
    assert eng.lib.avcer_s3fd_num_priors(64, 64) == 342  # 16^2 + 8^2 + 4^2 + 2^2 + 1 + 1
    assert call(frames, 64, 64, MODE_FP32, None) == 0
    assert call(frames, 64, 64, MODE_FP32, lm.data_ptr()) == -1   # AVCER_EINVAL: this kind has no landmarks
    assert call(frames, 64, 64, MODE_BF16, None) == -1
    assert call(frames, 31, 64, MODE_FP32, None) == -1
    with pytest.raises(Exception, match="AVCER_MODE_BF16"):
        eng.face_forward(np.zeros((1, 64, 64, 3), np.uint8), MODE_BF16)
    with pytest.raises(Exception):
        eng.face_forward(np.zeros((1, 31, 40, 3), np.uint8), MODE_FP32)
    assert eng.face_kind() == 3


def test_switching_between_the_three_detectors(sd_s3fd):
    sd_r50, sd_mnet = synth.to_torch(synth.retina_state_dict(42)), synth.to_torch(synth.retina_mnet_state_dict(42))
    frames = synth.video_frames(77, 2, 64, 96)
    e = Engine(0)
    try:
        e.load_face(sd_r50)
        assert e.face_kind() == 1
        first = [t.clone() for t in e.face_forward(frames, MODE_F16X3)]
        e.load_face(sd_s3fd)
        assert e.face_kind() == 3
        s1 = [t.clone() for t in e.face_forward(frames, MODE_F16X3)[:2]]
        assert all(torch.isfinite(t).all() for t in s1)
        e.load_face(sd_mnet)
        assert e.face_kind() == 2
        assert all(torch.isfinite(t).all() for t in e.face_forward(frames, MODE_F16X3))
        e.load_face(sd_r50)
        assert e.face_kind() == 1
        assert all(torch.equal(a, b) for a, b in zip(first, e.face_forward(frames, MODE_F16X3)))
        e.load_face(sd_s3fd)
        assert all(torch.equal(a, b) for a, b in zip(s1, e.face_forward(frames, MODE_F16X3)[:2]))
    finally:
        e.close()


# ---- 7: the pipeline
def test_run_inference_with_the_s3fd_detector(sd_s3fd, sd_static, sd_dynamic, sd_audio):
    """run_inference(detector=...) with the S3FD detector equals run_inference(detections=...) fed that detector's own rows."""
    e = Engine(0)
    try:
        e.load_static(sd_static)
        e.load_dynamic(sd_dynamic)
        e.load_audio(sd_audio)
        pred = ft.S3FDPredictor(e, sd_s3fd, threshold=0.3, mode=MODE_F16X3)
        frames = synth.video_frames(13, 6, 96, 128)
        wav = synth.waveforms(99, 1, int(6 / 25 * 16000))[0]
        dets = pred.batch(frames, rgb=False)
        assert sum(len(d) for d in dets) > 0
        a = arun.run_inference(e, frames, wav, 25, detector=pred, mode=MODE_F16X3)
        b = arun.run_inference(e, frames, wav, 25, detections=dets, mode=MODE_F16X3)
        for key in ("static_probs", "dynamic_logits", "audio_rows", "compound_prob", "av", "records"):
            np.testing.assert_array_equal(a[key], b[key])
    finally:
        e.close()
