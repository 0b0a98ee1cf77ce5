"""The cases of tests/golden/detect_edges.npz (tests/golden/make_golden_detect_edges.py: the reference's own decisions on non-finite
scores, non-finite and degenerate boxes and values exactly on a comparison) and what the project's oracles say about them.  Shared by
the CPU tests that hold the oracles to the fixture and by tests/test_gpu_detect_edges.py, so every expectation is computed once.

A case's kind says who may judge it: "plain" -- the fixture, the float32 oracle and the float64 oracle; "boundary" -- a value sits
exactly on a comparison, so float32 only; "tie_rule" -- tied scores, where the reference's order is numpy's unspecified one and the
fixture holds the kernels' documented rule (`stable=True`: ties higher index first)."""
from __future__ import annotations

import functools
import os

import numpy as np

import s3fd_ref
from oracle import face as of

E = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_edges.npz"))
R_CASES = [str(n) for n in E["names_r"]]
S_CASES = [str(n) for n in E["names_s"]]
B_VARIANTS = [str(n) for n in E["b_variants"]]
PAR = ("conf_thresh", "nms_thresh", "nms_top_k", "top_k", "threshold")
COUNTING_P = 16400   # more than the 16384 keys the LDS sort holds: the counting kernel orders the candidates


def _par(a):
    return {k: (int(v) if k.endswith("top_k") else float(v)) for k, v in zip(PAR, a)}


def retina_case(name):
    """kind, rows [T,P,5], the arguments of Engine.face_nms, the kept row indices per frame."""
    frames = E[f"r_{name}_dets"]
    return str(E[f"r_{name}_kind"]), frames, _par(E[f"r_{name}_par"]), [E[f"r_{name}_keep{t}"] for t in range(len(frames))]


def rows15(frames5, pad_to=None):
    """[T,P,5] -> the kernel's rows [T,P',15]: column 5 carries the row index, the landmark columns count on from it.  Padded rows
    are non-candidates under every floor: their score is -inf."""
    t, p = frames5.shape[:2]
    rows = np.zeros((t, pad_to or p, 15), np.float32)
    rows[:, :p, :5] = frames5
    rows[:, :, 5:] = np.arange(rows.shape[1], dtype=np.float32)[None, :, None] + np.arange(10, dtype=np.float32)
    rows[:, p:, 4] = -np.inf
    return rows


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def retina_oracle(name, dtype):
    """oracle/face.py on the case, statement by statement as retina_face_predictor.py:86-108 has them, in float32 or float64 (the
    scores and the thresholds stay the float32 values the kernel sees)."""
    kind, frames, par, _ = retina_case(name)
    return retina_keep(frames, par, dtype, stable=kind == "tie_rule")


def retina_keep(frames, par, dtype=np.float32, stable=True):
    """The kept row indices per frame of rows [T,P,5]: the statements of retina_oracle on any frames."""
    out = []
    for rows in frames:
        score = rows[:, 4]
        inds = np.where(score > np.float32(par["conf_thresh"]))[0]
        keep = inds
        if len(inds):
            keep = inds[of.nms(rows[inds].astype(dtype), float(np.float32(par["nms_thresh"])), par["nms_top_k"], stable=stable)]
        keep = keep[:par["top_k"]]
        out.append(keep[score[keep] >= np.float32(par["threshold"])])
    return out


def s3fd_case(name):
    """kind, loc [T,P,4], conf [T,P,2], priors [P,4], (h, w), the arguments of Engine.s3fd_detect, the rows per frame."""
    loc = E[f"s_{name}_loc"]
    return (str(E[f"s_{name}_kind"]), loc, E[f"s_{name}_conf"], E[f"s_{name}_priors"], tuple(int(v) for v in E[f"s_{name}_size"]),
            _par(E[f"s_{name}_par"]), [E[f"s_{name}_rows{t}"] for t in range(len(loc))])


@functools.lru_cache(maxsize=None)
def s3fd_oracle(name, dtype):
    kind, loc, conf, priors, (h, w), par, _ = s3fd_case(name)
    return [s3fd_ref.detect(loc[t], conf[t], priors, h, w, par["threshold"], par["top_k"], par["conf_thresh"], par["nms_thresh"],
                            par["nms_top_k"], dtype=dtype, stable=kind == "tie_rule") for t in range(len(loc))]


def assert_decoded(got, want):
    """Rows that came out of expf: the same class (NaN, +inf, -inf) wherever `want` is non-finite, elsewhere the decode tolerance of
    tests/test_gpu_face.py::test_decode_all_priors (expf is at most 2 ulp apart)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    np.testing.assert_allclose(got[fin], want[fin], rtol=3e-6, atol=3e-5)
