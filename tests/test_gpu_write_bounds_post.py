"""Guard bands (tests/guard_band.py) around the outputs of the audio, fusion, face-output and picture entries that the first round
of tests/test_gpu_write_bounds.py left out.  Every output of an entry is a band of one `check` call and every device input is in
`inputs`: guards and gap elements untouched, every "must" element written, the same bits in all three runs, the inputs unchanged.
The VALUES are the business of the parity tests; here they are compared with a host statement only where that is one line.  Where
an Engine wrapper allocates its output, the C entry is called through engine.lib so that the guarded buffer is the one written.
Every data-dependent extent comes from the project's CPU statement of the operation (oracle.face.nms, tests/s3fd_ref.py,
ceil(n * len / o)), never from what the device call returned.  Scratch inside the context's workspace (the candidate order of the
two NMS entries, the chart's envelope) cannot be guarded from outside.

Entries and the edge each shape was chosen for:
  avcer_resample             n_out = 1, n - 1, n + 1 and one short of / one past a block's qb * n outputs (the only store guard is
                             m < n_out inside a block of qb whole periods); three rate pairs, the equal-rate path, the unaligned
                             s16 stereo source
  avcer_audio_chunks         windows of 1, 511, 512, 513 samples against blocks of 512 threads; an empty range, one ending at the
                             signal's end; all three padding modes
  avcer_audio_frame_mean     n_frames * c on either side of one block of 128 threads; frames without a window; out and count
  avcer_fuse                 n = 1, 63, 64, 65 against blocks of 64 threads; n_aud < n; aud_c 7 and 8; comp_prob and comp_argmax
  avcer_fuse_videos          videos of 1, 63, 0 and 66 frames (130 frames: a third block of 64); all four outputs, and the two
                             that remain when aud_mean / count are NULL
  avcer_weight_search_counts m = 2, 3; w = 1, 255, 257 candidates; n = 1, 1000 frames with labels outside 0..c-1; tp and pred
  avcer_face_decode_batch    T = 3; P = 255, 256, 257
  avcer_face_nms             per frame rows [0, count) written and [count, top_k) a gap, count from the oracle: a frame that keeps
                             more than top_k, one that keeps a handful, one without a candidate; top_k 100 and 750; 3000 priors
                             (the sort orders them) and the same padded to 20000 (the counting kernel does)
  avcer_s3fd_detect          the same on the `trunc` case of tests/golden/s3fd_detect.npz plus a frame without detections
  avcer_crop_resize_linear   valid, 1 x 1, empty, frame out of range and frame-leaving rectangles; 224 x 224 and 7 x 5 (6 * 7 * 5 =
                             210 outputs: no multiple of 256; 224 * 224 is one, whatever n)
  avcer_cam_render           n = 3 overlays of M = 5 maps, a map used twice, classes 0 and 6
  avcer_chart_series         two charts in one call, one on each envelope path, plot width no multiple of the 64-wide paint tile;
                             painted in place over a prepared canvas"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import chart_cases as cc
import s3fd_ref
from avcer_amd import chart
from avcer_amd import heatmaps as hm
from avcer_amd.audio_pipeline import resample_out_len, resample_plan
from avcer_amd.engine import _ptr
from avcer_amd.fusion import WEIGHTS_AV_1, covered_frames
from guard_band import Band, check
from oracle import face as of

pytestmark = pytest.mark.gpu

DET = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s3fd_detect.npz"))


def _call(engine, name, *args):
    engine._check(getattr(engine.lib, name)(engine.ctx, *args, engine._stream()))


def _rng(*key):
    return np.random.default_rng([int(k) for k in key] + [20240])


# ----------------------------------------------------------------------------- avcer_resample
# csrc/resample.hip: qb = RS_R * ceil(RS_ITEMS / n) = 4 * ceil(512 / n) periods a block (the LDS bound, (12288 - 2 * width) / o
# rounded down to a multiple of 4, is larger for all three pairs), so a block owns qb * n outputs:
#   44100 -> 16000: o = 441, n = 160, qb = 16, 2560 outputs a block
#   48000 -> 16000: o = 3,   n = 1,   qb = 2048, 2048 outputs a block
#    8000 -> 16000: o = 1,   n = 2,   qb = 1024, 2048 outputs a block
RATES = {(44100, 16000): (441, 160, 16), (48000, 16000): (3, 1, 2048), (8000, 16000): (1, 2, 1024)}
SOURCES = {(44100, 16000): ("s16", 2), (48000, 16000): ("f32", 6), (8000, 16000): ("s16", 1)}


def _len_for(n_out, o, n):
    """The smallest source length with ceil(n * len / o) == n_out."""
    length = ((n_out - 1) * o) // n + 1
    assert resample_out_len(length, o, n) == n_out == -(-n * length // o)
    return length


def _source(kind, ch, length, dev, seed):
    rng = _rng(length, ch, seed)
    if kind == "s16":
        return torch.from_numpy(rng.integers(-32768, 32768, (length, ch), dtype=np.int16)).to(dev)
    return torch.from_numpy(rng.uniform(-1, 1, (ch, length)).astype(np.float32)).to(dev)


def _resample_bounds(engine, src, kind, length, ch, rates):
    dev = engine.device
    if rates is None:
        taps = first = None
        o = n = 1
        span = width = 0
        extra = []
    else:
        plan = resample_plan(*rates)
        taps = torch.from_numpy(np.array(plan.taps.T, dtype=np.float32, order="C")).to(dev)
        first = torch.from_numpy(np.array(plan.first, dtype=np.int32)).to(dev)
        o, n, span, width = plan.o, plan.n, plan.span, plan.width
        extra = [taps, first]
    n_out = -(-n * length // o)

    def run(outs):
        _call(engine, "avcer_resample", _ptr(src), 0 if kind == "s16" else 1, length, ch, _ptr(taps), _ptr(first), o, n, span, width,
              _ptr(outs[0]), n_out)

    y, = check(run, [Band("out", (n_out,), torch.float32)], [src] + extra, device=dev)
    assert torch.isfinite(y).all() and float(y.abs().max()) <= 1.5
    return y


@pytest.mark.parametrize("rates", list(RATES), ids=lambda r: f"{r[0]}-{r[1]}")
def test_resample(engine, rates):
    o, n, qb = RATES[rates]
    plan = resample_plan(*rates)
    assert (plan.o, plan.n) == (o, n) and qb == 4 * -(-512 // n) <= (12288 - 2 * plan.width) // o // 4 * 4
    kind, ch = SOURCES[rates]
    for n_out in sorted({1, max(n - 1, 1), n + 1, qb * n - 1, qb * n + 1}):
        if n == 2 and n_out % 2:              # 8000 -> 16000 has no odd n_out: test_resample_8000_reaches_the_block_edge
            continue
        length = _len_for(n_out, o, n)
        _resample_bounds(engine, _source(kind, ch, length, engine.device, n_out), kind, length, ch, rates)


def test_resample_8000_reaches_the_block_edge(engine):
    """8000 -> 16000 doubles: n_out is even, so the block edge is 2046 / 2048 / 2050 outputs and the shortest signal gives 2."""
    for length in (1, 1023, 1024, 1025):
        _resample_bounds(engine, _source("s16", 1, length, engine.device, 7), "s16", length, 1, (8000, 16000))


def test_resample_equal_rates(engine):
    """taps == NULL: conversion and downmix alone, n_out = len; 255, 256 and 257 frames against blocks of 256 threads."""
    for kind, ch in (("s16", 2), ("s16", 1), ("f32", 6)):
        for length in (1, 255, 256, 257):
            _resample_bounds(engine, _source(kind, ch, length, engine.device, 3), kind, length, ch, None)


def test_resample_unaligned_s16_stereo(engine):
    """A stereo int16 source at an odd int16 offset is not 4-byte aligned: K_S16 instead of K_S16_STEREO, the same numbers."""
    o, n, qb = RATES[(44100, 16000)]
    length = _len_for(qb * n + 1, o, n)
    flat = torch.from_numpy(_rng(5).integers(-32768, 32768, 2 * length + 2, dtype=np.int16)).to(engine.device)
    odd, even = flat[1:1 + 2 * length].view(length, 2), flat[1:1 + 2 * length].clone().view(length, 2)
    assert odd.data_ptr() % 4 == 2 and even.data_ptr() % 4 == 0
    a = _resample_bounds(engine, odd, "s16", length, 2, (44100, 16000))
    b = _resample_bounds(engine, even, "s16", length, 2, (44100, 16000))
    assert torch.equal(a, b)
    a = _resample_bounds(engine, odd, "s16", length, 2, None)
    assert torch.equal(a, _resample_bounds(engine, even, "s16", length, 2, None))


# ----------------------------------------------------------------------------- avcer_audio_chunks, avcer_audio_frame_mean
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["mean", "zeros", "repeat"])
@pytest.mark.parametrize("window", [1, 511, 512, 513])
def test_audio_chunks(engine, window, mode):
    """5 windows of a 1000-sample signal: a full one, a short one, an empty one (mean: NaN, repeat: NaN, never an index), a
    one-sample one and one that ends at the signal's end."""
    dev = engine.device
    wav = torch.from_numpy(_rng(window).uniform(-1, 1, 1000).astype(np.float32)).to(dev)
    short = max(window // 3, 1)
    starts = np.array([0, 100, 500, 700, 1000 - short], np.int32)
    ends = starts + np.array([window, short, 0, 1, short], np.int32)
    assert ends.max() == 1000 and (ends - starts).max() == window
    sd, ed = torch.from_numpy(starts).to(dev), torch.from_numpy(ends).to(dev)

    def run(outs):
        _call(engine, "avcer_audio_chunks", _ptr(wav), _ptr(sd), _ptr(ed), 5, window, mode, _ptr(outs[0]))

    out, = check(run, [Band("out", (5, window), torch.float32)], [wav, sd, ed], device=dev)
    w = wav.cpu()
    assert torch.equal(out[0], w[:window]) and torch.equal(out[4, :short], w[1000 - short:])
    assert bool(torch.isnan(out[2]).all()) == (mode != 1) and (mode != 1 or not out[2].any())


# n_frames * c against one block of 128 threads.  127 and 129 are products of neither 7 nor 8: the nearest on either side are taken.
@pytest.mark.parametrize("c,n_frames", [(7, 18), (7, 19), (8, 15), (8, 16), (8, 17)], ids=["126", "133", "120", "128", "136"])
def test_audio_frame_mean(engine, c, n_frames):
    """Windows cover frames 0..11 (some twice); the frames behind them have no window: count 0 and a row of zeros, but a WRITTEN one."""
    dev = engine.device
    win = torch.from_numpy(_rng(c, n_frames).normal(0, 2, (4, c)).astype(np.float32)).to(dev)
    lo = torch.tensor([0, 3, 6, 9], dtype=torch.int32, device=dev)
    hi = torch.tensor([5, 8, 11, 12], dtype=torch.int32, device=dev)

    def run(outs):
        _call(engine, "avcer_audio_frame_mean", _ptr(win), _ptr(lo), _ptr(hi), 4, c, n_frames, _ptr(outs[0]), _ptr(outs[1]))

    out, count = check(run, [Band("out", (n_frames, c), torch.float32), Band("count", (n_frames,), torch.int32, row_bytes=4 * c)],
                       [win, lo, hi], device=dev)
    want = [sum(a <= f < b for a, b in zip(lo.tolist(), hi.tolist())) for f in range(n_frames)]
    assert count.tolist() == want and not out[12:].any() and out[:12].abs().min() > 0


# ----------------------------------------------------------------------------- avcer_fuse, avcer_fuse_videos
def _tables(n, rng):
    e = np.exp(rng.normal(0, 1.5, (n, 7)))
    return (torch.from_numpy((e / e.sum(1, keepdims=True)).astype(np.float32)), torch.from_numpy(rng.normal(0, 2, (n, 7)).astype(np.float32)))


def _weights(w1):
    return ((C.c_double * 21)(*np.asarray(WEIGHTS_AV_1, dtype=np.float64).reshape(21)) if w1 else None), (C.c_double * 3)(0.5, 1.25, 2.0)


@pytest.mark.parametrize("aud_c", [7, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_fuse(engine, n, aud_c):
    """One thread a frame in blocks of 64; n_aud = n // 2 + 1 < n (n = 1: 1), so the rows behind repeat the last audio row."""
    dev = engine.device
    rng = _rng(n, aud_c)
    stat, dyn = (t.to(dev) for t in _tables(n, rng))
    n_aud = n // 2 + 1 if n > 1 else 1
    aud = torch.from_numpy(rng.normal(0, 2, (n_aud, aud_c)).astype(np.float32)).to(dev)
    for w1 in (True, False):
        a1, a2 = _weights(w1)

        def run(outs):
            _call(engine, "avcer_fuse", _ptr(stat), _ptr(dyn), _ptr(aud), n, n_aud, aud_c, a1, a2, 0, 1, _ptr(outs[0]), _ptr(outs[1]))

        prob, am = check(run, [Band("comp_prob", (4, n, 7), torch.float64), Band("comp_argmax", (4, n), torch.int32, row_bytes=4)],
                         [stat, dyn, aud], device=dev)
        assert torch.isfinite(prob).all() and int(am.min()) >= 0 and int(am.max()) <= 6


@pytest.mark.parametrize("with_mean", [True, False])
@pytest.mark.parametrize("c", [7, 8])
def test_fuse_videos(engine, c, with_mean):
    """Videos of 1, 63, 0 and 66 frames with 1, 4, 0 and 7 windows; video 3's windows cover 60 of its 66 frames (the tail rule).
    aud_mean and count are optional: with NULL for both, comp_prob and comp_argmax are all the entry has to write."""
    dev = engine.device
    fc = [1, 63, 0, 66]
    spans = [[(0, 2)], [(0, 20), (10, 40), (30, 63), (50, 70)], [], [(a, a + 12) for a in range(0, 56, 8)]]
    wc = [len(s) for s in spans]
    n, w = sum(fc), sum(wc)
    rng = _rng(c, 4)
    stat, dyn = (t.to(dev) for t in _tables(n, rng))
    win = torch.from_numpy(rng.normal(0, 2, (w, c)).astype(np.float32)).to(dev)
    lo, hi = (np.array([s[k] for v in spans for s in v], np.int32) for k in (0, 1))
    n_aud = [covered_frames([a for a, _ in s], [b for _, b in s], t) if t else 1 for t, s in zip(fc, spans)]
    assert n_aud == [1, 63, 1, 60]
    dv = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)
    lo_d, hi_d, fo_d, wo_d, na_d = dv(lo), dv(hi), dv(np.cumsum([0] + fc)), dv(np.cumsum([0] + wc)), dv(n_aud)
    a1, a2 = _weights(True)
    bands = [Band("comp_prob", (4, n, 7), torch.float64), Band("comp_argmax", (4, n), torch.int32, row_bytes=4)]
    if with_mean:
        bands += [Band("aud_mean", (n, c), torch.float32), Band("count", (n,), torch.int32, row_bytes=4)]

    def run(outs):
        _call(engine, "avcer_fuse_videos", _ptr(stat), _ptr(dyn), _ptr(win), _ptr(lo_d), _ptr(hi_d), _ptr(fo_d), _ptr(wo_d), _ptr(na_d), 4, n,
              w, c, a1, a2, 0, 1, _ptr(outs[2]) if with_mean else None, _ptr(outs[3]) if with_mean else None, _ptr(outs[0]), _ptr(outs[1]))

    got = check(run, bands, [stat, dyn, win, lo_d, hi_d, fo_d, wo_d, na_d], device=dev)
    assert torch.isfinite(got[0]).all()
    if with_mean:
        assert got[3][64 + 60:].tolist() == [0] * 6 and not got[2][64 + 60:].any() and int(got[3][:64 + 60].min()) >= 1


# ----------------------------------------------------------------------------- avcer_weight_search_counts
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("w", [1, 255, 257])
@pytest.mark.parametrize("m", [2, 3])
def test_weight_search_counts(engine, m, w, n):
    dev = engine.device
    c = 7
    rng = _rng(m, w, n)
    preds = torch.from_numpy(rng.dirichlet(np.ones(c), (m, n))).to(dev)
    labels = torch.from_numpy(rng.integers(-1, c + 2, n).astype(np.int32)).to(dev)        # -1, 7 and 8 match no class
    weights = torch.from_numpy(rng.dirichlet(np.ones(m), (w, c)).transpose(0, 2, 1).copy()).to(dev)
    assert tuple(weights.shape) == (w, m, c) and (n == 1 or int((labels < 0).sum()) and int((labels >= c).sum()))

    def run(outs):
        _call(engine, "avcer_weight_search_counts", _ptr(preds), _ptr(labels), n, m, c, _ptr(weights), w, _ptr(outs[0]), _ptr(outs[1]))

    tp, pred = check(run, [Band("tp", (w, c), torch.int32), Band("pred", (w, c), torch.int32)], [preds, labels, weights], device=dev)
    assert pred.sum(1).tolist() == [n] * w and bool((tp <= pred).all()) and int(tp.min()) >= 0


# ----------------------------------------------------------------------------- the face detectors' outputs
@pytest.mark.parametrize("p", [255, 256, 257])
def test_face_decode_batch(engine, p):
    dev = engine.device
    t = 3
    rng = _rng(p)
    loc, landms = (torch.from_numpy(rng.normal(0, 1, (t, p, k)).astype(np.float32)).to(dev) for k in (4, 10))
    conf = torch.from_numpy(rng.uniform(0, 1, (t, p, 2)).astype(np.float32)).to(dev)
    priors = torch.from_numpy(rng.uniform(0.05, 0.95, (p, 4)).astype(np.float32)).to(dev)

    def run(outs):
        _call(engine, "avcer_face_decode_batch", _ptr(loc), _ptr(conf), _ptr(landms), _ptr(priors), t, p, 120, 160, 0.1, 0.2, _ptr(outs[0]))

    dets, = check(run, [Band("dets", (t, p, 15), torch.float32)], [loc, conf, landms, priors], device=dev)
    assert torch.isfinite(dets).all() and torch.equal(dets[:, :, 4], conf.cpu()[:, :, 1])


NMS = dict(conf_thresh=0.02, nms_thresh=0.4, nms_top_k=5000, threshold=0.1)


@functools.lru_cache(maxsize=None)
def _nms_case():
    """Three frames of 3000 boxes from the generator of test_nms_kernel_matches_reference_keep_lists: a thousand small candidates that
    hardly overlap (more than 750 are kept), seven candidates among non-candidates, no candidate at all.  Returns the rows and, from the
    oracle, the kept count of each frame before the top_k cut."""
    rng = np.random.default_rng(5)
    n = 3000
    xy = rng.uniform(0, 600, (n, 2)).astype(np.float32)
    d = np.zeros((3, n, 15), np.float32)
    d[0, :, :4] = np.concatenate([xy, xy + rng.uniform(2, 12, (n, 2)).astype(np.float32)], axis=1)
    d[1, :, :4] = d[2, :, :4] = np.concatenate([xy, xy + rng.uniform(5, 120, (n, 2)).astype(np.float32)], axis=1)
    d[0, rng.choice(n, 1000, replace=False), 4] = rng.uniform(0.03, 1, 1000).astype(np.float32)   # (the plain-loop oracle is O(n^2))
    d[1, rng.choice(n, 7, replace=False), 4] = rng.uniform(0.5, 1, 7).astype(np.float32)
    d[:, :, 5] = np.arange(n)
    kept = []
    for b in d:
        inds = np.where(b[:, 4] > NMS["conf_thresh"])[0]
        keep = inds[of.nms(b[inds, :5], NMS["nms_thresh"], NMS["nms_top_k"], stable=True)] if len(inds) else inds
        kept.append(b[keep, 4])                                    # the kept scores, descending
    d.setflags(write=False)
    return d, kept


@pytest.mark.parametrize("priors", [3000, 20000], ids=["sort", "counting"])
@pytest.mark.parametrize("top_k", [100, 750])
def test_face_nms(engine, top_k, priors):
    """out [T, top_k, 15]: rows [0, count_f) of frame f are written, rows [count_f, top_k) are a gap (the header: out "receives, per
    frame, the kept rows"; nothing else).  Padded to 20000 priors with non-candidates the counting kernel orders the candidates
    instead of the LDS sort (16384 priors is its limit), and the same rows come out."""
    dev = engine.device
    d, kept = _nms_case()
    counts = [int((s[:top_k] >= NMS["threshold"]).sum()) for s in kept]
    assert counts[0] == top_k and len(kept[0]) > 750 and 0 < counts[1] <= 7 and counts[2] == 0
    rows = np.zeros((3, priors, 15), np.float32)
    rows[:, :3000] = d
    rows[:, 3000:, 4] = -5.0
    dets = torch.from_numpy(rows).to(dev)
    written = torch.zeros(3, top_k, 1, dtype=torch.bool)
    for f, k in enumerate(counts):
        written[f, :k] = True

    def run(outs):
        _call(engine, "avcer_face_nms", _ptr(dets), 3, priors, NMS["conf_thresh"], NMS["nms_thresh"], NMS["nms_top_k"], top_k,
              NMS["threshold"], _ptr(outs[0]), _ptr(outs[1]))

    out, out_n = check(run, [Band("out", (3, top_k, 15), torch.float32, written=written), Band("out_n", (3,), torch.int32, row_bytes=60)],
                       [dets], device=dev)
    assert out_n.tolist() == counts
    for f, k in enumerate(counts):
        assert np.array_equal(out[f, :k, 4].numpy(), kept[f][:k])


@functools.lru_cache(maxsize=None)
def _s3fd_case():
    """The four frames of the golden `trunc` case (nms_top_k = 64) and a fifth whose scores are all below the floor; the row counts
    from tests/s3fd_ref.py's Detect."""
    h, w = (int(v) for v in DET["size"])
    p = len(DET["priors"])
    loc = np.concatenate([DET["loc"], np.zeros((1, p, 4), np.float32)])
    conf = np.concatenate([DET["conf"], np.tile(np.array([[[1.0, 0.0]]], np.float32), (1, p, 1))])
    k = int(DET["trunc_nms_top_k"])
    thr = float(DET["threshold"])
    rows = [s3fd_ref.detect(loc[t], conf[t], DET["priors"], h, w, thr, top_k=1024, nms_top_k=k) for t in range(5)]
    return loc, conf, (h, w), k, thr, rows


@pytest.mark.parametrize("top_k", [3, 750])
def test_s3fd_detect(engine, top_k):
    """out [T, top_k, 5]: rows [0, count_f) written, the rest of each frame's slot a gap; a cut at top_k = 3 and none at 750."""
    dev = engine.device
    loc, conf, (h, w), k, thr, ref = _s3fd_case()
    counts = [min(len(r), top_k) for r in ref]
    assert counts[:4] == [min(int(v), top_k) for v in DET["trunc_counts"]] and counts[4] == 0 and max(counts) == min(top_k, max(map(len, ref)))
    assert any(len(r) > 3 for r in ref)
    loc_d, conf_d, pri_d = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (loc, conf, DET["priors"]))
    written = torch.zeros(5, top_k, 1, dtype=torch.bool)
    for f, c in enumerate(counts):
        written[f, :c] = True

    def run(outs):
        _call(engine, "avcer_s3fd_detect", _ptr(loc_d), _ptr(conf_d), _ptr(pri_d), 5, int(pri_d.shape[0]), h, w, 0.1, 0.2, 0.05, 0.3, k, top_k,
              thr, _ptr(outs[0]), _ptr(outs[1]))

    out, out_n = check(run, [Band("out", (5, top_k, 5), torch.float32, written=written), Band("out_n", (5,), torch.int32, row_bytes=20)],
                       [loc_d, conf_d, pri_d], device=dev)
    assert out_n.tolist() == counts
    for f, c in enumerate(counts):
        assert np.array_equal(out[f, :c, 4].numpy(), ref[f][:c, 4])


# ----------------------------------------------------------------------------- the pictures
@pytest.mark.parametrize("out_h,out_w", [(224, 224), (7, 5)])
@pytest.mark.parametrize("swap", [0, 1])
def test_crop_resize_linear(engine, out_h, out_w, swap):
    """The six rectangles of test_crop_tiles_rgb_identity_and_bad_rects: the bad ones yield zeros, but WRITTEN zeros."""
    dev = engine.device
    fr = np.random.default_rng(3).integers(0, 256, (2, 300, 260, 3), dtype=np.uint8)
    rects = np.array([[0, 10, 20, 234, 244], [1, 0, 0, 260, 300], [1, 5, 7, 6, 8], [0, 100, 100, 100, 150], [2, 0, 0, 10, 10],
                      [0, 200, 0, 270, 50]], dtype=np.int32)
    assert (6 * out_h * out_w) % 256 or (out_h, out_w) == (224, 224)
    frames, rd = torch.from_numpy(fr).to(dev), torch.from_numpy(rects).to(dev)

    def run(outs):
        _call(engine, "avcer_crop_resize_linear", _ptr(frames), 2, 300, 260, _ptr(rd), 6, swap, out_h, out_w, _ptr(outs[0]))

    got, = check(run, [Band("out", (6, out_h, out_w, 3), torch.uint8, row_bytes=3 * out_w)], [frames, rd], device=dev)
    got = got.numpy()
    px = fr[1, 7, 5][::-1] if swap else fr[1, 7, 5]
    assert (got[2] == px).all() and not got[3:].any() and got[0].any() and got[1].any()
    if (out_h, out_w) == (224, 224) and not swap:
        np.testing.assert_array_equal(got[0], fr[0, 20:244, 10:234])                # a rect of the output's size is copied


def test_cam_render(engine):
    dev = engine.device
    rng = _rng(5, 3)
    cam = torch.from_numpy(rng.standard_normal((5, 7, 7, 7)).astype(np.float32)).to(dev)
    rows = torch.tensor([4, 1, 4], dtype=torch.int32, device=dev)
    cls = torch.tensor([0, 6, 3], dtype=torch.int32, device=dev)
    base = torch.from_numpy(rng.integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)).to(dev)
    lut = torch.from_numpy(np.ascontiguousarray(hm.JET_BGR, dtype=np.uint8)).to(dev)

    def run(outs):
        _call(engine, "avcer_cam_render", _ptr(cam), _ptr(rows), _ptr(cls), _ptr(base), 3, _ptr(lut), 0.8, _ptr(outs[0]))

    got, = check(run, [Band("out", (3, 224, 224, 3), torch.uint8, row_bytes=3 * 224)], [cam, rows, cls, base, lut], device=dev)
    want = hm.render_overlay(hm.normalise_map(cam.cpu().numpy()[4, 0]), base.cpu().numpy()[0], hm.JET_BGR, 0.8)
    np.testing.assert_array_equal(got.numpy()[0], want)


def test_chart_series(engine):
    """Two charts of 96 x 64 in one call: 1000 frames (a column reduces its frames) and 7 frames (a column evaluates the segment
    that crosses it).  The entry paints over a prepared canvas, so `run` first copies that canvas into the band: what comes back
    is chart.series_numpy's picture over the canvas, each chart's pixels its own, and the guards untouched."""
    dev = engine.device
    refs = [cc.reference("random", 1000), cc.reference("alternating", 7)]
    plans = [r[1] for r in refs]
    assert [p.path for p in plans] == [chart.PATH_REDUCE, chart.PATH_SEGMENT] and plans[1].pw % 64 and plans[1].ph % 4
    table = torch.from_numpy(np.concatenate([r[0] for r in refs], axis=1)).to(dev)
    bg = np.random.default_rng(9).integers(0, 256, (2, cc.HEIGHT, cc.WIDTH, 3), dtype=np.uint8)
    src = torch.from_numpy(bg).to(dev)

    def run(outs):
        outs[0].copy_(src)
        assert engine.chart_series(table, plans, outs[0]) is outs[0]

    got, = check(run, [Band("out", (2, cc.HEIGHT, cc.WIDTH, 3), torch.uint8, row_bytes=3 * cc.WIDTH)], [table, src], device=dev)
    for v, (_, _, masks) in enumerate(refs):
        want = bg[v].copy()
        for s, m in enumerate(masks):
            want[m] = chart.COLOURS[s]
        np.testing.assert_array_equal(got.numpy()[v], want, err_msg=f"chart {v}")
