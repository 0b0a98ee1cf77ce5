#!/usr/bin/env python3
"""Generate tests/golden/face_net_mnet.npz by running the REFERENCE's own RetinaFace(cfg_mnet, phase="test") class, unmodified,
on avcer_amd.synth.retina_mnet_state_dict(42).

Run in the build container only (`python tests/golden/make_golden_mnet.py`), like make_golden.py, whose stubs it uses: every
module of this network (MobileNetV1, FPN, SSH, heads) lives in the reference tree; only torchvision's `IntermediateLayerGetter`
(torchvision is absent) is the stand-in make_golden.py already has.  Nothing under tests/ reads the reference at test time: only
the .npz travels."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
from avcer_amd import synth  # noqa: E402

SIZES = (("a", (96, 128)), ("b", (75, 101)), ("c", (33, 47)))  # b: no multiple of the strides; c: level 3 is 2 x 2, stage 1 is 5 x 6


def gen_face_net_mnet():
    from data.face_detection.ibug.face_detection.retina_face.config import cfg_mnet
    from data.face_detection.ibug.face_detection.retina_face import retina_face as rf

    _, rf._utils.IntermediateLayerGetter = mg.torchvision_resnet50_standin()
    net = rf.RetinaFace(cfg=cfg_mnet, phase="test")
    want = net.state_dict()
    mine = synth.retina_mnet_state_dict(42)
    assert list(want.keys()) == list(mine.keys()), set(want) ^ set(mine)
    assert all(tuple(want[k].shape) == tuple(np.shape(mine[k])) for k in want)
    print("state dict:", len(want), "entries,", sum(int(v.numel()) for v in want.values()), "values")
    missing, unexpected = net.load_state_dict(synth.to_torch(mine), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    net.eval()
    out = {}
    for name, (h, w) in SIZES:
        frame = synth.video_frames(900, 1, h, w)[0]
        x = torch.from_numpy((frame.astype(int) - np.array([104, 117, 123])).transpose(2, 0, 1)).unsqueeze(0).float()
        taps = {}
        hooks = [net.body.register_forward_hook(lambda m, i, o: taps.update({f"body{k}": v for k, v in o.items()})),
                 net.fpn.register_forward_hook(lambda m, i, o: taps.update({f"fpn{k + 1}": v for k, v in enumerate(o)})),
                 net.ssh1.register_forward_hook(lambda m, i, o: taps.__setitem__("ssh1", o))]
        with torch.no_grad():
            loc, conf, landms = net(x)
        for hk in hooks:
            hk.remove()
        out[f"{name}_size"] = np.array([h, w])
        out[f"{name}_loc"], out[f"{name}_conf"], out[f"{name}_landms"] = loc[0].numpy(), conf[0].numpy(), landms[0].numpy()
        for k, v in taps.items():
            out[f"{name}_{k}_stats"] = mg.stats(v)
            out[f"{name}_{k}_head16"] = mg.head16(v)
        c1 = conf[0, :, 1]
        print("face net mnet", name, tuple(loc.shape), "conf spread", c1.std().item(), "min", c1.min().item(), "max", c1.max().item(),
              "above 0.5:", int((c1 > 0.5).sum()), {k: tuple(v.shape) for k, v in taps.items()})
    np.savez_compressed(os.path.join(HERE, "face_net_mnet.npz"), **out)


if __name__ == "__main__":
    mg.install_stubs()
    gen_face_net_mnet()
