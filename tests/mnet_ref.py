"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the RetinaFace-MobileNet-0.25 detector network in functional torch.

Every module of this variant lives in the reference tree, so the whole restatement is pinned by tests/golden/face_net_mnet.npz,
which the reference's own RetinaFace(cfg_mnet, phase="test") produced (tests/golden/make_golden_mnet.py):
  * body: retina_face_net.py:103-125 (MobileNetV1 stage1-3; conv_bn :6-11, conv_dw :29-38, LeakyReLU(0.1)), returned at
    stage1 / stage2 / stage3 (config.py:19, retina_face.py:60);
  * FPN :70-100 and SSH :41-67 at out_channel 64, hence LeakyReLU(0.1) (:46-47, :74-75); the heads and the test-phase softmax
    retina_face.py:9-43,95-115; preprocessing retina_face_predictor.py:59-65.
f32 and float64 entry points; `taps` collects NCHW intermediates named like the library's debug taps without their "face_" prefix.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
MEAN_BGR = (104, 117, 123)   # retina_face_predictor.py:63
BLOCKS = ((8, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2)) + ((128, 128, 1),) * 5 + (
    (128, 256, 2), (256, 256, 1))
BLOCK_NAMES = tuple([f"body.stage1.{i}" for i in range(1, 6)] + [f"body.stage2.{i}" for i in range(6)] +
                    [f"body.stage3.{i}" for i in range(2)])
SLOPE = 0.1


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, BN_EPS)


def preprocess(frame_bgr_u8, dtype=torch.float32) -> torch.Tensor:
    """retina_face_predictor.py:59-65 with rgb=False: int pixels minus the mean, HWC -> 1CHW."""
    x = torch.from_numpy(frame_bgr_u8.astype(int)) - torch.tensor(MEAN_BGR)
    return x.permute(2, 0, 1).unsqueeze(0).to(dtype)


def conv_dw(sd, p, x, stride):
    """retina_face_net.py:29-38: depthwise 3x3 + BN + leaky, pointwise 1x1 + BN + leaky."""
    y = F.leaky_relu(_bn(F.conv2d(x, sd[p + ".0.weight"], stride=stride, padding=1, groups=x.shape[1]), sd, p + ".1"), SLOPE)
    return F.leaky_relu(_bn(F.conv2d(y, sd[p + ".3.weight"]), sd, p + ".4"), SLOPE)


def backbone(sd, x, taps=None):
    x = F.leaky_relu(_bn(F.conv2d(x, sd["body.stage1.0.0.weight"], stride=2, padding=1), sd, "body.stage1.0.1"), SLOPE)
    if taps is not None:
        taps["stem"] = x
    feats = []
    for i, (p, (_, _, s)) in enumerate(zip(BLOCK_NAMES, BLOCKS)):
        x = conv_dw(sd, p, x, s)
        if taps is not None:
            taps[f"blk{i + 1}"] = x
        if i in (4, 10, 12):
            feats.append(x)
    if taps is not None:
        taps.update(body1=feats[0], body2=feats[1], body3=feats[2])
    return feats


def _cba(sd, p, x, k, act):
    y = _bn(F.conv2d(x, sd[p + ".0.weight"], padding=k // 2), sd, p + ".1")
    return F.leaky_relu(y, SLOPE) if act else y


def fpn(sd, feats, taps=None):
    o1, o2, o3 = (_cba(sd, f"fpn.output{i + 1}", f, 1, True) for i, f in enumerate(feats))
    o2 = _cba(sd, "fpn.merge2", o2 + F.interpolate(o3, size=o2.shape[2:], mode="nearest"), 3, True)
    o1 = _cba(sd, "fpn.merge1", o1 + F.interpolate(o2, size=o1.shape[2:], mode="nearest"), 3, True)
    if taps is not None:
        taps.update(fpn1=o1, fpn2=o2, fpn3=o3)
    return [o1, o2, o3]


def ssh(sd, p, x):
    c3 = _cba(sd, p + ".conv3X3", x, 3, False)
    c5_1 = _cba(sd, p + ".conv5X5_1", x, 3, True)
    c5 = _cba(sd, p + ".conv5X5_2", c5_1, 3, False)
    c7 = _cba(sd, p + ".conv7x7_3", _cba(sd, p + ".conv7X7_2", c5_1, 3, True), 3, False)
    return F.relu(torch.cat([c3, c5, c7], dim=1))


def _head(sd, p, x, per_anchor):
    y = F.conv2d(x, sd[p + ".conv1x1.weight"], sd[p + ".conv1x1.bias"])
    return y.permute(0, 2, 3, 1).contiguous().view(y.shape[0], -1, per_anchor)


def mnet_forward(sd, x, taps=None):
    """RetinaFace(cfg_mnet).forward in test phase: (loc [n,P,4], conf [n,P,2] softmaxed, landms [n,P,10])."""
    with torch.no_grad():
        feats = [ssh(sd, f"ssh{i + 1}", f) for i, f in enumerate(fpn(sd, backbone(sd, x, taps), taps))]
        if taps is not None:
            taps["ssh1"] = feats[0]
        loc = torch.cat([_head(sd, f"BboxHead.{i}", f, 4) for i, f in enumerate(feats)], dim=1)
        conf = torch.cat([_head(sd, f"ClassHead.{i}", f, 2) for i, f in enumerate(feats)], dim=1)
        lm = torch.cat([_head(sd, f"LandmarkHead.{i}", f, 10) for i, f in enumerate(feats)], dim=1)
    return loc, F.softmax(conf, dim=-1), lm


def mnet_forward64(sd, frames_bgr_u8, taps=None):
    """mnet_forward of u8 frames [h,w,3] or [n,h,w,3] in float64: a comparison against it measures the library's rounding alone."""
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    fr = frames_bgr_u8 if frames_bgr_u8.ndim == 4 else frames_bgr_u8[None]
    x = torch.cat([preprocess(f, torch.float64) for f in fr])
    return mnet_forward(sd64, x, taps)
