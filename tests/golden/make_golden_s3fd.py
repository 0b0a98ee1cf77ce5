#!/usr/bin/env python3
"""Generate tests/golden/s3fd_net.npz and tests/golden/s3fd_detect.npz by running the REFERENCE's own S3FDNet, Detect and
S3FDPredictor.__call__, unmodified, on avcer_amd.synth.s3fd_state_dict(42) and on synthetic head outputs.

Run in the build container only (`python tests/golden/make_golden_s3fd.py`), like make_golden.py, whose stubs and paths it uses.
Nothing under tests/ reads the reference at test time: only the two .npz files travel."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
import s3fd_ref  # noqa: E402
from avcer_amd import synth  # noqa: E402

# a: the minimum (pool5 sees 2 x 2, levels 3-5 are 1 x 1); b: 19 x 25 reaches the ceil_mode pool, so both axes have an overhanging
# window, the floor pools drop a row and a column, levels 4-5 are 1 x 2 and 1 x 1; c: odd extents of another kind
SIZES = (("a", (32, 32)), ("b", (77, 101)), ("c", (65, 97)))


def _predictor(threshold, config):
    """The reference's predictor around a given network: everything of __init__ except reading the weight file."""
    from data.face_detection.ibug.face_detection.s3fd.s3fd_predictor import S3FDPredictor

    p = S3FDPredictor.__new__(S3FDPredictor)
    p.threshold, p.device, p.config = threshold, "cpu", config
    return p


def _config(**kw):
    from data.face_detection.ibug.face_detection.s3fd.s3fd_predictor import S3FDPredictor

    return SimpleNamespace(**S3FDPredictor.get_model().config.__dict__, **S3FDPredictor.create_config(**kw).__dict__)


def gen_net():
    from data.face_detection.ibug.face_detection.s3fd.s3fd_net import S3FDNet

    config = _config()
    net = S3FDNet(config=config, device="cpu")
    want, mine = net.state_dict(), synth.s3fd_state_dict(42)
    assert list(want.keys()) == list(mine.keys()), set(want) ^ set(mine)
    assert all(tuple(want[k].shape) == tuple(np.shape(mine[k])) for k in want)
    print("state dict:", len(want), "entries,", sum(int(v.numel()) for v in want.values()), "values")
    net.load_state_dict(synth.to_torch(mine))
    net.eval()
    pred = _predictor(0.5, config)
    pred.net = net
    seen = {}
    inner = net.detect
    net.detect = lambda loc, conf, priors: (seen.update(loc=loc, conf=conf, priors=priors), inner(loc, conf, priors))[1]
    # every tap is what its consumer reads (the ReLUs are in place, so a producer's output changes after its hook has run)
    consumers = {"conv1": net.vgg[2], "pool3": net.vgg[17], "conv3_3": net.L2Norm3_3, "conv4_3": net.L2Norm4_3,
                 "conv5_3": net.L2Norm5_3, "fc7": net.extras[0], "ex1": net.extras[2], "ex3": net.loc[5]}
    out = {}
    for name, (h, w) in SIZES:
        frame = synth.video_frames(900, 1, h, w)[0]
        taps = {}
        hooks = [m.register_forward_pre_hook(lambda mod, inp, k=k: taps.__setitem__(k, inp[0].clone())) for k, m in consumers.items()]
        dets = pred(frame, rgb=False)
        for hk in hooks:
            hk.remove()
        out[f"{name}_size"] = np.array([h, w])
        out[f"{name}_loc"], out[f"{name}_conf"] = seen["loc"][0].numpy(), seen["conf"][0].numpy()
        out[f"{name}_priors"] = seen["priors"].numpy()
        out[f"{name}_dets"] = np.asarray(dets, np.float32).reshape(-1, 5)
        for k, v in taps.items():
            out[f"{name}_{k}_stats"] = mg.stats(v)
            out[f"{name}_{k}_head16"] = mg.head16(v)
        c1 = seen["conf"][0, :, 1]
        print("s3fd net", name, tuple(seen["loc"].shape), "conf min", c1.min().item(), "max", c1.max().item(), "above 0.05:",
              int((c1 > 0.05).sum()), "above 0.5:", int((c1 > 0.5).sum()), "dets", out[f"{name}_dets"].shape,
              {k: (tuple(v.shape), round(float(v.abs().max()), 2)) for k, v in taps.items()})
    np.savez_compressed(os.path.join(HERE, "s3fd_net.npz"), **out)


def _clusters(seed, priors, n_faces, per_face, low_hi):
    """loc / conf a head could emit: `n_faces` clusters of `per_face` priors regress to overlapping boxes with distinct high scores;
    every other prior scores in [0, low_hi)."""
    P = priors.shape[0]
    loc = synth.centered(seed, "loc", (P, 4), 0.5).astype(np.float32)
    score = synth.uniform(seed, "low", (P,), 0.0, low_hi)
    pick = np.argsort(synth.uniform01(seed, "pick", P), kind="stable")[: n_faces * per_face].reshape(n_faces, per_face)
    for f in range(n_faces):
        cx, cy = synth.uniform(seed, f"c{f}", (2,), 0.25, 0.75)
        sw, sh = synth.uniform(seed, f"s{f}", (2,), 0.12, 0.3)
        for j, i in enumerate(pick[f]):
            jit = synth.uniform(seed, f"j{f}_{j}", (4,), -0.12, 0.12)
            tx, ty, tw, th = cx + jit[0] * sw, cy + jit[1] * sh, sw * (1 + jit[2]), sh * (1 + jit[3])
            loc[i] = [(tx - priors[i, 0]) / (0.1 * priors[i, 2]), (ty - priors[i, 1]) / (0.1 * priors[i, 3]),
                      np.log(tw / priors[i, 2]) / 0.2, np.log(th / priors[i, 3]) / 0.2]
            score[i] = 0.3 + 0.69 * synth.uniform01(seed, f"sc{f}_{j}", 1)[0]
    return loc, np.stack([1 - score, score], 1).astype(np.float32)


def gen_detect():
    from data.face_detection.ibug.face_detection.s3fd.utils import Detect

    h, w = 77, 101
    threshold = 0.6
    priors = np.array(__import__("avcer_amd.face_tiles", fromlist=["x"]).s3fd_prior_boxes((h, w)))
    # frame 0: three faces; 1: nothing above the floor; 2: one face among many weak candidates; 3: more than 64 candidates
    frames = [_clusters(11, priors, 3, 9, 0.045), _clusters(12, priors, 0, 0, 0.045), _clusters(13, priors, 1, 14, 0.2),
              _clusters(14, priors, 6, 16, 0.045)]
    out = {"size": np.array([h, w]), "priors": priors, "threshold": np.float32(threshold),
           "loc": np.stack([f[0] for f in frames]), "conf": np.stack([f[1] for f in frames])}
    for name, nms_top_k in (("full", 5000), ("trunc", 64)):
        config = _config(nms_top_k=nms_top_k)
        pred = _predictor(threshold, config)
        counts = []
        for t, (loc, conf) in enumerate(frames):
            pred.net = lambda image, loc=loc, conf=conf: Detect(config)(torch.from_numpy(loc)[None], torch.from_numpy(conf)[None],
                                                                         torch.from_numpy(priors))
            dets = np.asarray(pred(np.zeros((h, w, 3), np.uint8), rgb=True), np.float32).reshape(-1, 5)
            # the margins that let the GPU comparison keep every row: on the restatement, which must first agree with the reference
            ious = []
            mine = s3fd_ref.detect(loc, conf, priors, h, w, threshold, nms_top_k=nms_top_k, ious=ious)
            np.testing.assert_array_equal(mine, dets)
            sc = conf[:, 1]
            assert np.abs(sc - 0.05).min() > 1e-5 and np.abs(sc - threshold).min() > 1e-5
            cand = np.sort(sc[sc > 0.05])
            assert cand.size < 2 or np.diff(cand).min() > 0
            assert all(np.abs(o - 0.3).min() > 1e-4 for o in ious if o.size)
            out[f"{name}_dets{t}"] = dets
            counts.append(len(dets))
            print("s3fd detect", name, "frame", t, "candidates", cand.size, "kept", len(dets), "ious", sum(o.size for o in ious))
        out[f"{name}_counts"] = np.array(counts, np.int32)
        out[f"{name}_nms_top_k"] = np.array(nms_top_k)
    assert out["full_counts"][1] == 0 and (frames[1][1][:, 1] <= 0.05).all()
    assert (frames[3][1][:, 1] > 0.05).sum() > 64
    np.savez_compressed(os.path.join(HERE, "s3fd_detect.npz"), **out)


if __name__ == "__main__":
    mg.install_stubs()
    gen_net()
    gen_detect()
