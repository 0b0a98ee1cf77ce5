"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the S3FD detector in functional torch / numpy.

Pinned by tests/golden/s3fd_net.npz and tests/golden/s3fd_detect.npz, which the reference's own S3FDNet, Detect and
S3FDPredictor.__call__ produced (tests/golden/make_golden_s3fd.py):
  * network: s3fd_net.py:113-171 -- the VGG-16 trunk (:35-76; the pool at index 16 has ceil_mode, fc6 is dilated by 6), L2Norm
    (:8-25) on conv3_3 / conv4_3 / conv5_3, the four extras (:82-87, :139-142), the `loc` / `conf` heads (:89-105), the max-out
    background label of level 0 (:148-149) and the 2-class softmax (:171); preprocessing s3fd_predictor.py:45-52;
  * post-processing: utils.py:6-24 (decode), :94-128 (nms_np), :131-171 (Detect), s3fd_predictor.py:54-68 (the threshold loop).
f32 and float64 entry points; `taps` collects NCHW intermediates named like the library's debug taps without their "s3fd_" prefix,
one per launch (LAUNCHES); `hook` lets a test change one launch's output on the way.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MEAN_RGB = (123, 117, 104)   # s3fd_predictor.py:49
POOLS = {4: False, 9: False, 16: True, 23: False, 30: False}   # vgg index -> ceil_mode
CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28, 31, 33)
TAPS = {0: "conv1", 16: "pool3", 14: "conv3_3", 21: "conv4_3", 28: "conv5_3", 33: "fc7"}
VARIANCE = (0.1, 0.2)


def preprocess(frame_u8, rgb=False, dtype=torch.float32) -> torch.Tensor:
    """s3fd_predictor.py:45-52: a BGR frame is flipped, int pixels minus the RGB mean, HWC -> 1CHW."""
    img = frame_u8 if rgb else frame_u8[..., ::-1]
    x = torch.from_numpy(img.astype(int) - np.array(MEAN_RGB))
    return x.permute(2, 0, 1).unsqueeze(0).to(dtype)


def l2norm(x, weight):
    norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10
    return weight.view(1, -1, 1, 1) * torch.div(x, norm)


LAUNCHES = ("conv1",) + tuple(f"out:vgg{k}.w" for k in CONVS[1:]) + tuple(f"out:ex{k}.w" for k in range(4)) + tuple(f"pool{k}" for k in range(1, 6))
POOL_NAMES = {4: "pool1", 9: "pool2", 16: "pool3", 23: "pool4", 30: "pool5"}
POOL_INPUT = {"pool1": "out:vgg2.w", "pool2": "out:vgg7.w", "pool3": "out:vgg14.w", "pool4": "out:vgg21.w", "pool5": "out:vgg28.w"}
STEM = ("conv1", None, "vgg.0", 1, 1, 1)   # conv1_1 as a row of contractions(): its input is the preprocessed frame


def conv_geometry(k):
    """(stride, padding, dilation) of vgg.k: fc6 (vgg.31) is dilated by 6 with padding 6, fc7 (vgg.33) is 1 x 1."""
    return (1, 6, 6) if k == 31 else (1, 0, 1) if k == 33 else (1, 1, 1)


def trunk(sd, x, taps=None, hook=None):
    """The six head inputs (the first three already normalised).

    taps: every launch's output under the library's tap name without its "s3fd_" prefix -- "conv1", "out:vgg2.w" .. "out:vgg33.w",
    "out:ex0.w" .. "out:ex3.w", "pool1" .. "pool5" (LAUNCHES) -- the eight older names as aliases of the same tensors, and the three
    L2-normalised sources "l2norm0" .. "l2norm2".
    hook(name, tensor) -> tensor: called with each launch's name and output before anything reads it; what it returns goes on.
    tests/test_gpu_s3fd_stages.py plants its deliberate departures through it; None changes nothing."""
    sources = []

    def put(name, t, *aliases):
        if hook is not None:
            t = hook(name, t)
        if taps is not None:
            for n_ in (name,) + aliases:
                taps[n_] = t
        return t

    for k in range(35):
        if k in POOLS:
            x = put(POOL_NAMES[k], F.max_pool2d(x, 2, 2, ceil_mode=POOLS[k]))
        elif k in CONVS:
            _, pad, dil = conv_geometry(k)
            x = F.relu(F.conv2d(x, sd[f"vgg.{k}.weight"], sd[f"vgg.{k}.bias"], padding=pad, dilation=dil))
            x = put("conv1" if k == 0 else f"out:vgg{k}.w", x, *((TAPS[k],) if k in TAPS and k else ()))
        if k in (14, 21, 28):
            sources.append(l2norm(x, sd[{14: "L2Norm3_3", 21: "L2Norm4_3", 28: "L2Norm5_3"}[k] + ".weight"]))
            if taps is not None:
                taps[f"l2norm{len(sources) - 1}"] = sources[-1]
    sources.append(x)
    for k in range(4):
        x = F.relu(F.conv2d(x, sd[f"extras.{k}.weight"], sd[f"extras.{k}.bias"], stride=2 if k % 2 else 1, padding=1 if k % 2 else 0))
        x = put(f"out:ex{k}.w", x, *((f"ex{k}",) if k % 2 else ()))
        if k % 2:
            sources.append(x)
    return sources


def contractions():
    """The 18 contraction launches behind the stem, in launch order: (tap name, input tap name, state-dict prefix, stride, padding,
    dilation).  A launch's input is the launch in front of it (a pool where there is one)."""
    out, prev = [], "conv1"
    for k in range(1, 35):
        if k in POOLS:
            prev = POOL_NAMES[k]
        elif k in CONVS:
            out.append((f"out:vgg{k}.w", prev, f"vgg.{k}") + conv_geometry(k))
            prev = out[-1][0]
    for k in range(4):
        out.append((f"out:ex{k}.w", prev, f"extras.{k}", 2 if k % 2 else 1, 1 if k % 2 else 0, 1))
        prev = out[-1][0]
    return out


def launch64(sd, spec, x, hook=None):
    """One contraction launch (a row of contractions(), or STEM) in float64 on its own input x [n,c,h,w]:
    (ReLU(conv(x) + b), sum |x| |w|, |b| as [1,n,1,1], K).  The second and third are what a rounding bound of the launch scales with,
    K is the number of products per output.  `hook` as in trunk: it sees this launch's name and output."""
    name, _, p, stride, pad, dil = spec
    w, b = sd[p + ".weight"].double(), sd[p + ".bias"].double()
    x = x.double()
    with torch.no_grad():
        ref = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad, dilation=dil))
        sxw = F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=pad, dilation=dil)
    if hook is not None:
        ref = hook(name, ref)
    return ref, sxw, b.abs().view(1, -1, 1, 1), int(w[0].numel())


def pool64(name, x, hook=None):
    """One pool launch on its own input (any dtype: a maximum is exact)."""
    y = F.max_pool2d(x, 2, 2, ceil_mode=name == "pool3")
    return hook(name, y) if hook is not None else y


def heads(sd, sources):
    """Pre-softmax head outputs per level: (loc [n,h,w,4], conf [n,h,w,2]) with level 0's max-out applied."""
    out = []
    for i, s in enumerate(sources):
        loc = F.conv2d(s, sd[f"loc.{i}.weight"], sd[f"loc.{i}.bias"], padding=1)
        conf = F.conv2d(s, sd[f"conf.{i}.weight"], sd[f"conf.{i}.bias"], padding=1)
        if i == 0:
            conf = torch.cat((conf[:, 0:3].max(dim=1, keepdim=True)[0], conf[:, 3:]), dim=1)
        out.append((loc.permute(0, 2, 3, 1).contiguous(), conf.permute(0, 2, 3, 1).contiguous()))
    return out


def s3fd_forward(sd, x, taps=None, hook=None):
    """S3FDNet.forward up to the call of Detect: (loc [n,P,4], conf [n,P,2] softmaxed, feature maps [(h, w)] * 6).  `taps` also
    receives the pre-softmax head outputs of each level, "head_loc0" .. "head_loc5" [n,h,w,4] and "head_conf0" .. [n,h,w,2]."""
    with torch.no_grad():
        hd = heads(sd, trunk(sd, x, taps, hook))
        if taps is not None:
            for i, (l, c) in enumerate(hd):
                taps[f"head_loc{i}"], taps[f"head_conf{i}"] = l, c
        n = x.shape[0]
        loc = torch.cat([l.reshape(n, -1) for l, _ in hd], 1).view(n, -1, 4)
        conf = torch.cat([c.reshape(n, -1) for _, c in hd], 1).view(n, -1, 2)
    return loc, F.softmax(conf, dim=-1), [tuple(l.shape[1:3]) for l, _ in hd]


def s3fd_forward64(sd, frames_bgr_u8, taps=None, hook=None, dtype=torch.float64):
    """s3fd_forward of u8 BGR frames [h,w,3] or [n,h,w,3] in float64: a comparison against it measures the library's rounding alone.
    dtype=torch.float32 runs the same function in float32: the CPU's own rounding of the graph, the yardstick of the stage tests."""
    sdt = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    fr = frames_bgr_u8 if frames_bgr_u8.ndim == 4 else frames_bgr_u8[None]
    x = torch.cat([preprocess(f, False, dtype) for f in fr])
    return s3fd_forward(sdt, x, taps, hook)


def num_priors(h: int, w: int) -> int:
    """The extent rule of avcer_s3fd_num_priors, restated."""
    def ext(v):
        b = v // 2 // 2
        f = [b, -(-b // 2)]
        f += [f[1] // 2]
        f += [f[2] // 2]
        f += [(f[3] - 1) // 2 + 1]
        f += [(f[4] - 1) // 2 + 1]
        return f
    return sum(a * b for a, b in zip(ext(h), ext(w)))


# ------------------------------------------------------------------------------------------------ Detect + the predictor's loop
def decode(loc, priors, variances=VARIANCE, dtype=np.float32):
    """utils.py:6-24, operation by operation, in float32 torch (so that exp is the reference's); dtype=np.float64 is the yardstick."""
    loc, priors = torch.as_tensor(np.asarray(loc, dtype)), torch.as_tensor(np.asarray(priors, dtype))
    boxes = torch.cat((priors[:, :2] + loc[:, :2] * variances[0] * priors[:, 2:], priors[:, 2:] * torch.exp(loc[:, 2:] * variances[1])), 1)
    boxes[:, :2] -= boxes[:, 2:] / 2
    boxes[:, 2:] += boxes[:, :2]
    return boxes.numpy()


@np.errstate(all="ignore")   # non-finite and degenerate boxes are inputs like any other (tests/golden/detect_edges.npz)
def nms_np(boxes, scores, overlap, top_k, ious=None, stable=False):
    """utils.py:94-128 in the precision of `boxes`; `ious` collects every IoU the loop evaluates.  numpy's maxima and minima
    propagate a NaN operand, so a box with a NaN corner has a NaN overlap with every other box and `ovr <= overlap` drops it.
    `stable`: the same with `argsort(kind="stable")`, the kernels' rule for tied scores (higher index first after the reversal);
    numpy's default sort leaves their order unspecified."""
    if scores.shape[0] == 0:
        return []
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    order = (scores.argsort(kind="stable") if stable else scores.argsort())[: -top_k - 1: -1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        xx1, yy1 = np.maximum(x1[i], x1[order[1:]]), np.maximum(y1[i], y1[order[1:]])
        xx2, yy2 = np.minimum(x2[i], x2[order[1:]]), np.minimum(y2[i], y2[order[1:]])
        w, h = np.maximum(0.0, xx2 - xx1), np.maximum(0.0, yy2 - yy1)
        ovr = w * h / (areas[i] + areas[order[1:]] - w * h)
        if ious is not None:
            ious.append(ovr)
        order = order[np.where(ovr <= overlap)[0] + 1]
    return keep


def detect(loc, conf, priors, im_h, im_w, threshold, top_k=750, conf_thresh=0.05, nms_thresh=0.3, nms_top_k=5000, ious=None,
           dtype=np.float32, stable=False):
    """Detect.__call__ for one frame and class 1, then the predictor's loop: [k,5] float32 = x0, y0, x1, y1 (pixels), score.
    dtype=np.float64: boxes, areas and overlaps in float64 (scores and the thresholds stay the float32 values they are)."""
    boxes = decode(loc, priors, dtype=dtype)
    scores = np.asarray(conf, np.float32)[:, 1]
    mask = scores > np.float32(conf_thresh)
    boxes, scores = boxes[mask], scores[mask]
    keep = nms_np(boxes, scores, np.float32(nms_thresh), nms_top_k, ious, stable)[:top_k]
    rows = []
    for i in keep:
        if not scores[i] >= np.float32(threshold):
            break
        rows.append(np.concatenate((boxes[i] * np.array([im_w, im_h, im_w, im_h], np.float32), scores[i:i + 1])))
    return np.asarray(rows, np.float32).reshape(-1, 5)
