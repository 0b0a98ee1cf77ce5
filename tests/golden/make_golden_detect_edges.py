#!/usr/bin/env python3
"""Generate tests/golden/detect_edges.npz: the detector tails on non-finite scores, non-finite and degenerate boxes and on values that
sit exactly on a comparison, as the REFERENCE's own code decides them.

  r_*  rows [T,P,5] = x1, y1, x2, y2, score through py_cpu_nms, unmodified, between the statements of RetinaFacePredictor.__call__
       around it (retina_face_predictor.py:86-108: `np.where(scores > conf_thresh)`, `[:top_k]`, `np.where(dets[:, 4] >= threshold)`);
  b_*  head outputs through RetinaFacePredictor.__call__, unmodified, around a stand-in network: decode, scale and the tail;
  s_*  loc / conf / priors through S3FD's Detect and S3FDPredictor.__call__, unmodified.

Run in the build container only (`python tests/golden/make_golden_detect_edges.py`), like make_golden.py and make_golden_s3fd.py,
whose stubs and paths it uses.  Nothing under tests/ reads the reference at test time: only the .npz travels.

Every case has a kind, which says how far the reference itself is deterministic on it and what else may judge it:
  plain     no two candidates tie, no score sits on a threshold and every finite overlap is at least MARGIN away from nms_thresh:
            the float64 oracle must agree as well;
  boundary  a value sits exactly on a comparison: float32 only;
  tie_rule  tied candidates (-0.0 and +0.0 are a tie for numpy): py_cpu_nms and nms_np visit ties in whatever order numpy's default
            argsort leaves them, and on a CPU whose numpy sorts float32 with its SIMD network that order is not the index order even
            for a handful of keys.  The reference is not deterministic there, so the expectation is the rule the kernels document --
            `argsort(kind="stable")` read backwards, ties higher index first -- taken from the oracle; this script prints whether the
            reference's default sort agreed on the machine it ran on;
  decode    the boxes come out of expf: rows within the decode tolerance, scores exact, same class where non-finite."""
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
import make_golden_s3fd as ms  # noqa: E402
import s3fd_ref  # noqa: E402
from avcer_amd import face_tiles as ft  # noqa: E402
from avcer_amd import synth  # noqa: E402
from oracle import face as of  # noqa: E402

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
MARGIN = 1e-4
NMS_MAX, TOP_K_MAX = 6144, 1024           # the kernels' documented limits
EXP_EDGES = (88.72, -87.34)               # expf overflows above the first; below the second its result is subnormal, then (-103.97) zero
EXP_SUBNORMAL = (-104.0, -87.34)          # no argument in here: a flushing expf and a gradual one would differ


# ------------------------------------------------------------------------------------------------ building blocks
def grid(n, per_row=64):
    """n pairwise disjoint 10 x 10 boxes (9 apart in corner coordinates), 20 pixels from one to the next."""
    k = np.arange(n)
    x, y = 20 * (k % per_row), 20 * (k // per_row)
    return np.stack([x, y, x + 9, y + 9], 1).astype(F32)


def falling(n, step):
    s = (0.9 - step * np.arange(n)).astype(F32)
    assert np.unique(s).size == n
    return s


def shuffled(seed, boxes, scores):
    """The rows in a seeded order, so that a row's index says nothing about its rank; returns rows [n,5] and the index of rank r."""
    perm = np.random.default_rng(seed).permutation(len(boxes))
    rows = np.concatenate([boxes, scores[:, None]], 1).astype(F32)[perm]
    return rows, np.argsort(perm)


def dense30(seed):
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 40, (30, 2))
    wh = rng.integers(10, 40, (30, 2))
    scores = rng.permutation(np.linspace(0.3, 0.95, 30)).astype(F32)
    return np.concatenate([xy, xy + wh, scores[:, None]], 1).astype(F32)


def geometry():
    """Small integers only, so every f32 and f64 operation on them is exact."""
    return np.array([
        [0, 0, 9, 9, .95], [0, 0, 9, 9, .94],                  # identical, IoU 1
        [30, 0, 30, 9, .93], [30, 0, 30, 9, .60],              # x2 = x1: Retina's width is 1, S3FD's 0
        [50, 0, 50, 0, .92], [50, 0, 50, 0, .59],              # a point: Retina's area 1, S3FD's 0 (0 / 0 against its twin)
        [70, 0, 60, 9, .91], [70, 0, 60, 9, .58],              # inverted in x: Retina's area -90, the union with its twin -180
        [100, 0, 108, 9, .90],                                   # Retina's area +90: the union with the inverted box is 0, 0 / 0
        [120, 0, 119, 9, .89], [120, 0, 119, 9, .57],          # x2 = x1 - 1: Retina's area 0 (0 / 0 against its twin), S3FD's -9
        [200, 0, 239, 39, .88], [210, 10, 219, 19, .56], [205, 5, 234, 34, .55],   # wholly inside: a small one and a large one
        [300, 0, 309, 9, .87], [309, 0, 318, 9, .54],          # touching at one pixel column: overlap for Retina, none for S3FD
        [350, 20, 340, 10, .86], [350, 20, 340, 10, .53],      # inverted in both axes: a positive area again
    ], dtype=F32)


# ------------------------------------------------------------------------------------------------ RetinaFace tail
def ref_retina(py_cpu_nms, rows5, conf_thresh, nms_thresh, nms_top_k, top_k, threshold):
    """retina_face_predictor.py:86-108 around the reference's py_cpu_nms; the thresholds are Python floats, as its config holds them.
    Returns the kept row indices of the frame."""
    scores = rows5[:, 4]
    inds = np.where(scores > conf_thresh)[0]
    if len(inds) == 0:
        return np.zeros(0, np.int64)
    dets = np.hstack((rows5[inds, :4], scores[inds][:, np.newaxis])).astype(np.float32, copy=False)
    keep = inds[np.asarray(py_cpu_nms(dets, nms_thresh, nms_top_k), np.int64)][:top_k]
    return keep[np.where(rows5[keep, 4] >= threshold)[0]]


def check_kind(name, kind, scores, conf_thresh, threshold, ious, nms_thresh):
    cand = scores[scores > F32(conf_thresh)]
    tied = np.unique(cand).size != cand.size
    on_edge = bool((scores == F32(conf_thresh)).any() or (scores == F32(threshold)).any())
    fin = np.concatenate([o[np.isfinite(o)] for o in ious]) if ious else np.zeros(0)
    near = bool(fin.size and np.abs(fin.astype(np.float64) - float(F32(nms_thresh))).min() <= MARGIN)
    if kind == "plain":
        assert not tied and not on_edge and not near, (name, tied, on_edge, near)
    elif kind == "boundary":
        assert not tied and (on_edge or near), name
    elif kind == "tie_rule":
        assert tied and not near, name
    else:
        raise AssertionError(kind)
    return cand.size


def retina_cases():
    cases = {}

    def add(name, kind, frames, conf=0.02, nms=0.4, nms_top_k=5000, top_k=750, thr=0.1):
        assert nms_top_k <= NMS_MAX and top_k <= TOP_K_MAX
        cases[name] = (kind, np.stack(frames).astype(F32), (conf, nms, nms_top_k, top_k, thr))

    # A: non-finite scores.  -0.0 has the higher index of the two zeros, so a key that orders them by sign bit visits them the other way
    rng = np.random.default_rng(1)
    a = np.concatenate([grid(45, 9), rng.permutation(np.linspace(0.06, 0.95, 45))[:, None]], 1).astype(F32)
    a[7, 4], a[13, 4], a[21, 4], a[30, 4], a[17, 4] = NAN, INF, -INF, F32(-0.0), F32(0.0)
    add("a_scores", "plain", [a], thr=0.5)
    add("a_scores_floor", "tie_rule", [a], conf=-1e30, thr=-1e30)
    t = np.concatenate([grid(16, 4), np.linspace(0.1, 0.9, 16)[:, None]], 1).astype(F32)
    t[9, :4], t[12, :4] = t[3, :4], t[14, :4]                 # two pairs of identical boxes: which twin is visited first is which is kept
    t[0, 4], t[5, 4], t[3, 4], t[9, 4], t[12, 4], t[14, 4] = NAN, INF, F32(0.0), F32(-0.0), F32(-0.0), F32(0.0)
    add("a_zero_tie", "tie_rule", [t], conf=-1e30, thr=-1e30)
    add("a_all_nan", "plain", [np.full_like(a, NAN), a], thr=0.5)

    # C: a NaN / inf box in every role of the walk
    for tag, col, val in (("nan_x1", 0, NAN), ("nan_y2", 3, NAN), ("inf_x2", 2, INF)):
        d = dense30(3)
        d[np.argmax(d[:, 4]), col] = val
        add(f"c30_{tag}", "plain", [d])
    d = dense30(3)
    d[np.argmax(d[:, 4]), [0, 2]] = -INF, INF                  # area inf: every overlap with it is 0
    add("c30_inf_span", "plain", [d])
    d = dense30(3)
    d[np.argsort(d[:, 4])[15], 0] = NAN                       # a NaN box in the middle of the order: the first kept box drops it
    add("c30_nan_mid", "plain", [d])
    big, rank = shuffled(5, grid(2100), falling(2100, 1e-4))
    d = big.copy()
    d[rank[0], 0] = NAN                                        # kept in chunk 1; chunks 2 and 3 meet it in the kept arrays
    add("c_chunk1_nan", "plain", [d])
    d = big.copy()
    d[rank[0], [0, 2]] = -INF, INF
    add("c_chunk1_inf", "plain", [d])
    d = big.copy()
    d[rank[1100], 0] = NAN                                     # behind 1100 kept boxes; top_k = 1024 ends the walk in front of it
    add("c_chunk2_low", "plain", [d], top_k=1024)
    d = big.copy()
    d[rank[1:1024:2], :4] = d[rank[0:1024:2], :4]             # chunk 1 keeps 512 of its 1024, so the walk goes on into chunk 2,
    d[rank[1100], 0] = NAN                                     # where the NaN box is tested against the kept arrays
    add("c_chunk2_reached", "plain", [d])

    # D: degenerate geometry, at the default threshold and at one between the touching pair's overlap (10 / 190) and 0
    add("d_geometry", "plain", [geometry()])
    add("d_geometry_tight", "plain", [geometry()], nms=0.05)

    # E: exactly on the comparisons
    half = np.array([[0, 0, 9, 9, .9], [0, 0, 19, 9, .8], [100, 0, 109, 9, .7]], F32)     # inter 100, union 200
    add("e_iou_at", "boundary", [half], nms=0.5)
    add("e_iou_below", "boundary", [half], nms=float(np.nextafter(F32(0.5), F32(0))))
    s = np.array([.9, F32(.8), np.nextafter(F32(.8), F32(0)), .5, F32(.02), np.nextafter(F32(.02), F32(1)), .01, .85, .7, .6], F32)
    e = np.concatenate([grid(10), s[:, None]], 1).astype(F32)
    add("e_floor_eq", "boundary", [e], thr=-1e30)
    add("e_thr_eq", "boundary", [e], thr=0.8)
    forty, _ = shuffled(6, grid(40), falling(40, 1e-2))
    add("e_nms_top_k_eq", "plain", [forty], nms_top_k=40)
    add("e_nms_top_k_below", "plain", [forty], nms_top_k=39)
    add("e_top_k_1024", "plain", [big[np.sort(rank[:1024])]], top_k=1024)    # reached by the last box of chunk 1
    add("e_top_k_1025", "plain", [big[np.sort(rank[:1025])]], top_k=1024)
    d = big[np.sort(rank[:1025])].copy()
    r2 = np.argsort(-d[:, 4])
    d[r2[11], :4] = d[r2[10], :4]                             # chunk 1 keeps 1023: the first box of chunk 2 is the 1024th
    add("e_top_k_next", "plain", [d], top_k=1024)
    add("e_top_k_750", "plain", [big[np.sort(rank[:1030])]], top_k=750)
    return cases


def gen_retina(out):
    from data.face_detection.ibug.face_detection.retina_face.py_cpu_nms import py_cpu_nms

    names = []
    for name, (kind, frames, par) in retina_cases().items():
        conf, nms, nms_top_k, top_k, thr = par
        for t, rows in enumerate(frames):
            with np.errstate(all="ignore"):
                ref = ref_retina(py_cpu_nms, rows, conf, nms, nms_top_k, top_k, thr)
            ious = []
            inds = np.where(rows[:, 4] > F32(conf))[0]
            mine = inds[of.nms(rows[inds], nms, nms_top_k, stable=True, ious=ious)][:top_k] if len(inds) else inds
            mine = mine[rows[mine, 4] >= F32(thr)]
            n_cand = check_kind(name, kind, rows[:, 4], conf, thr, ious, nms)
            agrees = np.array_equal(ref, mine)
            assert agrees or kind == "tie_rule", (name, t, ref.tolist(), mine.tolist())
            out[f"r_{name}_keep{t}"] = mine.astype(np.int64)
            print(f"retina {name:18s} {kind:9s} frame {t}: {len(rows):5d} rows, {n_cand:5d} candidates, kept {len(mine):4d}"
                  + ("" if agrees else "   (the reference's default sort orders the tie differently: the stable rule is recorded)"))
        out[f"r_{name}_dets"], out[f"r_{name}_par"], out[f"r_{name}_kind"] = frames, np.array(par, np.float64), np.array(kind)
        names.append(name)
    out["names_r"] = np.array(names)


# ------------------------------------------------------------------------------------------------ RetinaFace decode, end to end
B_SIZE = (120, 160)
B_SPECIAL = {"big": 100, "inf": 205, "zero": 310, "nan": 415, "lm": 520, "inf2": 610, "big2": 700}
B_VARIANTS = {"first": {"inf": .99, "big": .95, "zero": .6, "lm": .5}, "mid": {"inf": .64, "big": .95, "zero": .6, "lm": .5},
              "last": {"inf": .31, "big": .95, "zero": .6, "lm": .5},
              "multi": {"big": .97, "big2": .96, "zero": .955, "lm": .94, "nan": .33, "inf2": .32}}


def decode_inputs(seed, priors):
    """loc / landms with `loc * variance` at 80 (finite, huge), 100 (inf) and -110 (0), NaN in loc and in landms; 24 ordinary
    candidates; the scores of the special rows come from the variant."""
    P = len(priors)
    loc = synth.centered(seed, "loc", (P, 4), 1.0).astype(F32)
    landms = synth.centered(seed, "landms", (P, 10), 1.0).astype(F32)
    s = {k: v * P // 800 for k, v in B_SPECIAL.items()}       # (RetinaFace has 800 priors at B_SIZE: the indices as written)
    loc[s["big"], 2], loc[s["inf"], 2], loc[s["zero"], 3], loc[s["nan"], 0] = 400.0, 500.0, -550.0, NAN
    loc[s["inf2"], 2:], loc[s["big2"], 2:], landms[s["lm"], 3] = 500.0, 400.0, NAN
    arg = loc[:, 2:][np.isfinite(loc[:, 2:])].astype(np.float64) * 0.2
    assert all(np.abs(arg - e).min() >= 8 for e in EXP_EDGES) and not ((arg > EXP_SUBNORMAL[0]) & (arg < EXP_SUBNORMAL[1])).any()
    base = synth.uniform(seed, "low", (P,), 0.0, 0.015).astype(F32)
    free = np.setdiff1d(np.arange(P), list(s.values()))
    pick = free[np.argsort(synth.uniform01(seed, "pick", len(free)), kind="stable")[:24]]
    base[pick] = np.linspace(0.35, 0.93, 24).astype(F32)[np.argsort(synth.uniform01(seed, "rank", 24), kind="stable")]
    confs = {}
    for v, special in B_VARIANTS.items():
        sc = base.copy()
        for k, val in special.items():
            sc[s[k]] = val
        confs[v] = np.stack([1 - sc, sc], 1).astype(F32)
    return loc, landms, confs, s


def gen_retina_decode(out):
    from data.face_detection.ibug.face_detection.retina_face.box_utils import decode, decode_landm
    from data.face_detection.ibug.face_detection.retina_face.config import cfg_re50
    from data.face_detection.ibug.face_detection.retina_face.prior_box import PriorBox
    from data.face_detection.ibug.face_detection.retina_face.retina_face_predictor import RetinaFacePredictor

    h, w = B_SIZE
    priors = PriorBox(cfg_re50, image_size=B_SIZE).forward()
    np.testing.assert_array_equal(priors.numpy(), of.prior_boxes(B_SIZE))
    loc, landms, confs, s = decode_inputs(71, priors.numpy())
    boxes = (decode(torch.from_numpy(loc), priors, cfg_re50["variance"]) * torch.Tensor([w, h, w, h])).numpy()
    lm = (decode_landm(torch.from_numpy(landms), priors, cfg_re50["variance"]) * torch.Tensor([w, h] * 5)).numpy()
    assert s == B_SPECIAL and np.isfinite(boxes[s["big"]]).all() and boxes[s["big"], 2] > 1e30 and np.isnan(boxes[s["inf"], 2]) and boxes[s["inf"], 0] == -INF
    assert boxes[s["zero"], 1] == boxes[s["zero"], 3] and np.isnan(boxes[s["nan"], [0, 2]]).all() and np.isnan(lm[s["lm"], 3])
    out.update(b_size=np.array(B_SIZE), b_loc=loc, b_landms=landms, b_boxes=boxes, b_lm=lm, b_threshold=np.array(0.3),
               b_variants=np.array(list(confs)))
    for v, conf in confs.items():
        pred = object.__new__(RetinaFacePredictor)
        pred.threshold, pred.device, pred.priors, pred.previous_size = 0.3, "cpu", None, None
        pred.config = SimpleNamespace(**cfg_re50, **RetinaFacePredictor.create_config().__dict__)
        pred.net = lambda image, c=conf: (torch.from_numpy(loc)[None], torch.from_numpy(c)[None], torch.from_numpy(landms)[None])
        with np.errstate(all="ignore"):
            dets = pred(mg.face_frame(0, h, w), rgb=False)
        # a 2-ulp expf must not change a decision: every finite overlap keeps its distance from the threshold, no score ties
        sc = conf[:, 1]
        inds = np.where(sc > F32(0.02))[0]
        ious = []
        keep = inds[of.nms(np.hstack((boxes[inds], sc[inds, None])), 0.4, 5000, ious=ious)]
        check_kind(f"b_{v}", "plain", sc, 0.02, 0.3, ious, 0.4)
        np.testing.assert_array_equal(dets, np.hstack((boxes, sc[:, None], lm))[keep])
        out[f"b_conf_{v}"], out[f"b_pred_{v}"], out[f"b_keep_{v}"] = conf, dets, keep.astype(np.int64)
        print(f"retina decode {v:6s}: {len(inds)} candidates, kept {len(dets)}, non-finite rows {int((~np.isfinite(dets)).any(1).sum())}")


# ------------------------------------------------------------------------------------------------ S3FD
S_UNIT = 1024.0          # the integer boxes above become normalised ones: k / 1024 is exact, and so is every product of two of them
S_IMAGE = (256, 512)     # powers of two: the scale to pixels is exact too


def prior_of(boxes):
    """The prior whose decode with loc = 0 IS the box: cx - w / 2 and w + x0 are exact on these dyadic values."""
    b = np.asarray(boxes, np.float64) / S_UNIT
    p = np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(F32)
    back = np.stack([p[:, 0] - p[:, 2] / 2, p[:, 1] - p[:, 3] / 2, p[:, 2] + (p[:, 0] - p[:, 2] / 2), p[:, 3] + (p[:, 1] - p[:, 3] / 2)], 1)
    np.testing.assert_array_equal(back.astype(np.float64), b)
    return p


def s3fd_cases():
    cases = {}

    def add(name, kind, rows5, loc=None, priors=None, size=S_IMAGE, conf=0.05, nms=0.3, nms_top_k=5000, top_k=750, thr=0.5):
        """rows5 [T,P,5] or [P,5]: finite boxes in units of 1 / 1024 and scores; `loc` [T,P,4] departs from 0 where a box is to be
        non-finite; `priors` replaces the priors of frame 0's boxes."""
        rows5 = np.asarray(rows5, F32)
        rows5 = rows5[None] if rows5.ndim == 2 else rows5
        T, P = rows5.shape[:2]
        assert nms_top_k <= NMS_MAX and top_k <= TOP_K_MAX and (thr > 0 or kind == "tie_rule")
        priors = prior_of(rows5[0, :, :4]) if priors is None else priors
        loc = np.zeros((T, P, 4), F32) if loc is None else loc
        sc = rows5[:, :, 4]
        cases[name] = (kind, loc, np.stack([1 - sc, sc], 2).astype(F32), priors, size, (conf, nms, nms_top_k, top_k, thr))

    def with_loc(rows5, edits):
        loc = np.zeros((1, len(rows5), 4), F32)
        for i, c, v in edits:
            loc[0, i, c] = v
        return loc

    rng = np.random.default_rng(1)
    a = np.concatenate([grid(45, 9), rng.permutation(np.linspace(0.06, 0.95, 45))[:, None]], 1).astype(F32)
    a[7, 4], a[13, 4], a[21, 4], a[30, 4], a[17, 4] = NAN, INF, -INF, F32(-0.0), F32(0.0)
    add("a_scores", "plain", a)
    t = np.concatenate([grid(16, 4), np.linspace(0.1, 0.9, 16)[:, None]], 1).astype(F32)
    t[9, :4], t[12, :4] = t[3, :4], t[14, :4]
    t[0, 4], t[5, 4], t[3, 4], t[9, 4], t[12, 4], t[14, 4] = NAN, INF, F32(0.0), F32(-0.0), F32(-0.0), F32(0.0)
    add("a_zero_tie", "tie_rule", t, conf=-1e30, thr=-1.0)
    nan_frame = np.full_like(a, NAN)
    add("a_all_nan", "plain", np.stack([nan_frame, a]), loc=np.stack([np.full((45, 4), NAN, F32), np.zeros((45, 4), F32)]), priors=prior_of(a[:, :4]))

    d = dense30(3)
    top, mid = int(np.argmax(d[:, 4])), int(np.argsort(d[:, 4])[15])
    add("c30_nan_x", "plain", d, loc=with_loc(d, [(top, 0, NAN)]))
    add("c30_nan_y", "plain", d, loc=with_loc(d, [(top, 1, NAN)]))
    add("c30_nan_mid", "plain", d, loc=with_loc(d, [(mid, 0, NAN)]))
    p = prior_of(d[:, :4])
    p[top, 2:] = F32(2.0 ** 100)                               # w = h = 2^100: the area overflows to inf, every overlap with it is 0
    add("c30_inf_area", "plain", d, priors=p)
    big, rank = shuffled(5, grid(2100), falling(2100, 2e-5))
    thr_of = lambda r: float(big[rank[r], 4]) - 1e-5           # noqa: E731  (fewer than top_k rows pass, or the reference's loop leaves its tensor)
    add("c_chunk1_nan", "plain", big, loc=with_loc(big, [(rank[0], 0, NAN)]), thr=thr_of(700))
    p = prior_of(big[:, :4])
    p[rank[0], 2:] = F32(2.0 ** 100)
    add("c_chunk1_inf", "plain", big, priors=p, thr=thr_of(700))
    d2 = big.copy()
    d2[rank[1:1024:2], :4] = d2[rank[0:1024:2], :4]
    add("c_chunk2_reached", "plain", d2, loc=with_loc(d2, [(rank[1100], 0, NAN)]), thr=thr_of(1200))

    add("d_geometry", "plain", geometry())
    add("d_geometry_tight", "plain", geometry(), nms=0.05)

    half = np.array([[0, 0, 8, 8, .9], [0, 0, 16, 8, .8], [128, 0, 136, 8, .7]], F32)     # inter 64, union 128, all / 1024^2
    add("e_iou_at", "boundary", half, nms=0.5)
    add("e_iou_below", "boundary", half, nms=float(np.nextafter(F32(0.5), F32(0))))
    s = np.array([.9, F32(.8), np.nextafter(F32(.8), F32(0)), .5, F32(.05), np.nextafter(F32(.05), F32(1)), .01, .85, .7, .6], F32)
    e = np.concatenate([grid(10), s[:, None]], 1).astype(F32)
    add("e_floor_eq", "boundary", e, thr=0.05)
    add("e_thr_eq", "boundary", e, thr=0.8)
    forty, _ = shuffled(6, grid(40), falling(40, 1e-2))
    add("e_nms_top_k_eq", "plain", forty, nms_top_k=40)
    add("e_nms_top_k_below", "plain", forty, nms_top_k=39)
    return cases


def ref_s3fd(loc, conf, priors, size, par):
    """One frame through the reference: S3FDPredictor.__call__ around Detect."""
    from data.face_detection.ibug.face_detection.s3fd.utils import Detect

    (h, w), (conf_thresh, nms, nms_top_k, top_k, thr) = size, par
    config = ms._config(top_k=top_k, conf_thresh=conf_thresh, nms_thresh=nms, nms_top_k=nms_top_k)
    pred = ms._predictor(thr, config)
    pred.net = lambda image: Detect(config)(torch.from_numpy(loc)[None], torch.from_numpy(conf)[None], torch.from_numpy(priors))
    with np.errstate(all="ignore"):
        return np.asarray(pred(np.zeros((h, w, 3), np.uint8), rgb=True), np.float32).reshape(-1, 5)


def gen_s3fd(out):
    names = []
    for name, (kind, loc, conf, priors, size, par) in s3fd_cases().items():
        conf_thresh, nms, nms_top_k, top_k, thr = par
        for t in range(len(loc)):
            ious = []
            mine = s3fd_ref.detect(loc[t], conf[t], priors, size[0], size[1], thr, top_k, conf_thresh, nms, nms_top_k, ious, stable=True)
            n_cand = check_kind(f"s_{name}", kind, conf[t, :, 1], conf_thresh, thr, ious, nms)
            if kind == "tie_rule":   # the predictor's `while score >= threshold` loop cannot report a zero score: the stable rule alone
                ref = mine
            else:
                ref = ref_s3fd(loc[t], conf[t], priors, size, par)
                np.testing.assert_array_equal(mine, ref, err_msg=name)
            assert len(ref) < top_k
            out[f"s_{name}_rows{t}"] = ref
            print(f"s3fd   {name:18s} {kind:9s} frame {t}: {len(priors):5d} priors, {n_cand:5d} candidates, rows {len(ref):4d}, "
                  f"non-finite rows {int((~np.isfinite(ref)).any(1).sum())}")
        out[f"s_{name}_loc"], out[f"s_{name}_conf"], out[f"s_{name}_priors"] = loc, conf, priors
        out[f"s_{name}_size"], out[f"s_{name}_par"], out[f"s_{name}_kind"] = np.array(size), np.array(par, np.float64), np.array(kind)
        names.append(name)
    out["names_s"] = np.array(names)


def gen_s3fd_decode(out):
    h, w = 77, 101
    priors = np.array(ft.s3fd_prior_boxes((h, w)))
    loc, _, confs, _ = decode_inputs(72, priors)
    out.update(sb_size=np.array([h, w]), sb_loc=loc, sb_priors=priors, sb_threshold=np.array(0.3), sb_variants=np.array(list(confs)))
    par = (0.05, 0.3, 5000, 750, 0.3)
    for v, conf in confs.items():
        ref = ref_s3fd(loc, conf, priors, (h, w), par)
        ious = []
        mine = s3fd_ref.detect(loc, conf, priors, h, w, 0.3, ious=ious)
        check_kind(f"sb_{v}", "plain", conf[:, 1], 0.05, 0.3, ious, 0.3)
        np.testing.assert_array_equal(mine, ref)
        out[f"sb_conf_{v}"], out[f"sb_rows_{v}"] = conf, ref
        print(f"s3fd decode {v:6s}: rows {len(ref)}, non-finite rows {int((~np.isfinite(ref)).any(1).sum())}")


if __name__ == "__main__":
    mg.install_stubs()
    out = {}
    gen_retina(out)
    gen_retina_decode(out)
    gen_s3fd(out)
    gen_s3fd_decode(out)
    path = os.path.join(HERE, "detect_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
