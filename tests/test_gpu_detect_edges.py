"""The detector tails (decode, order, NMS of csrc/detect_tail.hip) where "the keep decisions are the reference's" had no
test: NaN / inf / -inf / signed-zero scores, a frame that is NaN throughout (what an overflowed x3 pass hands over before the guarded
caller repeats it in fp32), boxes that leave expf as inf, NaN or with zero size, a NaN or inf box in every role of the chunked walk,
zero-size and inverted boxes, an overlap exactly on nms_thresh, scores exactly on conf_thresh and threshold, nms_top_k and top_k reached
exactly.  tests/golden/detect_edges.npz holds what the reference's own py_cpu_nms, Detect and predictors decide (its generator lists the
cases and says of each how far the reference is deterministic); tests/detect_edge_cases.py adds the project's oracles, which the CPU
tests hold to the same fixture.

Every RetinaFace case runs in both order forms -- as it is (the LDS sort) and padded with non-candidates past 16384 priors (the
counting kernel) -- and every NMS call runs inside the guard bands of tests/guard_band.py as well: rows [0, count) of a frame are
written, nothing else of `out`, and `out_n`.  The kernels take no address from a score or a coordinate (loads and stores are indexed
by thread and block ids, by candidate counts and by ranks that are sums of comparisons, each checked against nms_top_k / top_k), so a
non-finite value can change a decision but not where anything is read or written; these tests pin the decisions.

Everything is exact but the rows that came out of expf, which carry the decode tolerance of tests/test_gpu_face.py."""
import numpy as np
import pytest
import torch

import detect_edge_cases as ec
import s3fd_ref
from avcer_amd.engine import _ptr
from guard_band import Band, check
from oracle import face as of

pytestmark = pytest.mark.gpu

E = ec.E
FORMS = {"sort": None, "counting": ec.COUNTING_P}


def _call(engine, name, *args):
    engine._check(getattr(engine.lib, name)(engine.ctx, *args, engine._stream()))


def _written(counts, top_k):
    m = torch.zeros(len(counts), top_k, 1, dtype=torch.bool)
    for f, k in enumerate(counts):
        m[f, :k] = True
    return m


def _retina_nms(engine, rows, par, want_rows):
    """Engine.face_nms, then avcer_face_nms inside guard bands: both give `want_rows` (one [k,15] array per frame) bit for bit."""
    counts = [len(w) for w in want_rows]
    out, cnt = engine.face_nms(rows, **par)
    assert cnt.cpu().tolist() == counts
    got = [out[f, :k].cpu().numpy() for f, k in enumerate(counts)]
    dets = torch.from_numpy(rows).to(engine.device)
    t, p, top_k = rows.shape[0], rows.shape[1], par["top_k"]

    def run(outs):
        _call(engine, "avcer_face_nms", _ptr(dets), t, p, par["conf_thresh"], par["nms_thresh"], par["nms_top_k"], top_k, par["threshold"],
              _ptr(outs[0]), _ptr(outs[1]))

    band, band_n = check(run, [Band("out", (t, top_k, 15), torch.float32, written=_written(counts, top_k)),
                               Band("out_n", (t,), torch.int32, row_bytes=60)], [dets], device=engine.device)
    assert band_n.tolist() == counts
    for f, k in enumerate(counts):
        assert ec.same_bits(band[f, :k].numpy(), got[f])
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ec.R_CASES)
def test_retina_tail(engine, name, form):
    kind, frames, par, want = ec.retina_case(name)
    assert [k.tolist() for k in ec.retina_oracle(name, np.float32)] == [k.tolist() for k in want]
    if kind == "plain":
        assert [k.tolist() for k in ec.retina_oracle(name, np.float64)] == [k.tolist() for k in want]
    rows = ec.rows15(frames, FORMS[form])
    got = _retina_nms(engine, rows, par, [rows[f, k] for f, k in enumerate(want)])
    for f, k in enumerate(want):
        assert got[f][:, 5].astype(int).tolist() == k.tolist()     # the keep list, readable in a failure
        assert ec.same_bits(got[f], rows[f, k])


def _b_inputs():
    size = tuple(int(v) for v in E["b_size"])
    return size, of.prior_boxes(size)


def test_retina_decode_overflow_underflow_and_nan(engine):
    """face_decode_kernel where `loc * variance` is 80, 100 and -110 and where loc / landms hold NaN: the class of the reference at its
    non-finite positions, the decode tolerance elsewhere, scores and landmarks bit for bit (NaN included)."""
    size, pri = _b_inputs()
    conf = E[f"b_conf_{ec.B_VARIANTS[0]}"]
    dets = engine.face_decode(E["b_loc"], conf, E["b_landms"], pri, size).cpu().numpy()
    ec.assert_decoded(dets[:, :4], E["b_boxes"])
    with np.errstate(all="ignore"):
        ec.assert_decoded(dets[:, :4], of.decode(E["b_loc"], pri) * np.array([size[1], size[0]] * 2, np.float32))
        lm = of.decode_landm(E["b_landms"], pri) * np.array([size[1], size[0]] * 5, np.float32)
    assert ec.same_bits(dets[:, 4], conf[:, 1]) and ec.same_bits(dets[:, 5:], E["b_lm"]) and ec.same_bits(dets[:, 5:], lm)
    bad = ~np.isfinite(E["b_boxes"])
    assert np.isnan(E["b_boxes"]).any() and (E["b_boxes"] == -np.inf).any() and bad.any(1).sum() >= 3 and np.isnan(E["b_lm"]).any()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", ec.B_VARIANTS)
def test_retina_decode_then_tail(engine, variant, form):
    """Those decoded rows on through order and NMS with the reference's defaults, the non-finite box scored first (it is kept and
    every later overlap with it is NaN: one row), in the middle and last: RetinaFacePredictor.__call__'s rows."""
    size, pri = _b_inputs()
    conf, ref, keep = E[f"b_conf_{variant}"], E[f"b_pred_{variant}"], E[f"b_keep_{variant}"]
    dets = engine.face_decode(E["b_loc"], conf, E["b_landms"], pri, size).cpu().numpy()
    rows = np.zeros((1, FORMS[form] or len(dets), 15), np.float32)
    rows[0, len(dets):, 4] = -np.inf
    rows[0, :len(dets)] = dets
    par = dict(conf_thresh=0.02, nms_thresh=0.4, nms_top_k=5000, top_k=750, threshold=float(E["b_threshold"]))
    got, = _retina_nms(engine, rows, par, [dets[keep]])
    ec.assert_decoded(got[:, :4], ref[:, :4])
    assert ec.same_bits(got[:, 4:], ref[:, 4:])


def _s3fd(engine, loc, conf, priors, size, par, want, exact):
    counts = [len(w) for w in want]
    out, cnt = engine.s3fd_detect(loc, conf, priors, size, **par)
    assert cnt.cpu().tolist() == counts
    got = [out[f, :k].cpu().numpy() for f, k in enumerate(counts)]
    for g, w in zip(got, want):
        if exact:
            assert ec.same_bits(g, w), (g, w)
        else:
            ec.assert_decoded(g[:, :4], w[:, :4])
            assert ec.same_bits(g[:, 4], w[:, 4])
    dev = engine.device
    loc_d, conf_d, pri_d = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (loc, conf, priors))
    t, p, top_k = len(loc), len(priors), par["top_k"]

    def run(outs):
        _call(engine, "avcer_s3fd_detect", _ptr(loc_d), _ptr(conf_d), _ptr(pri_d), t, p, size[0], size[1], 0.1, 0.2, par["conf_thresh"],
              par["nms_thresh"], par["nms_top_k"], top_k, par["threshold"], _ptr(outs[0]), _ptr(outs[1]))

    band, band_n = check(run, [Band("out", (t, top_k, 5), torch.float32, written=_written(counts, top_k)),
                               Band("out_n", (t,), torch.int32, row_bytes=20)], [loc_d, conf_d, pri_d], device=dev)
    assert band_n.tolist() == counts
    for f, k in enumerate(counts):
        assert ec.same_bits(band[f, :k].numpy(), got[f])


@pytest.mark.parametrize("name", ec.S_CASES)
def test_s3fd_tail(engine, name):
    """The same roles on S3FD's normalised boxes and its areas without "+1", through avcer_s3fd_detect (decode, order, NMS).  The
    priors are dyadic and loc is 0 wherever a box is to be finite, so decode is exact and the rows are the reference's bit for bit."""
    kind, loc, conf, priors, size, par, want = ec.s3fd_case(name)
    assert all(ec.same_bits(g, w) for g, w in zip(ec.s3fd_oracle(name, np.float32), want))
    if kind == "plain":
        assert all(ec.same_bits(g, w) for g, w in zip(ec.s3fd_oracle(name, np.float64), want))
    _s3fd(engine, loc, conf, priors, size, par, want, exact=True)


@pytest.mark.parametrize("variant", ec.B_VARIANTS)
def test_s3fd_decode_then_tail(engine, variant):
    """s3fd_decode_kernel with `loc * variance` of 80, 100 and -110 and NaN in loc, then order and NMS: S3FDPredictor.__call__'s rows
    within the decode tolerance, scores exact, the same class where a corner is not finite."""
    size = tuple(int(v) for v in E["sb_size"])
    par = dict(conf_thresh=0.05, nms_thresh=0.3, nms_top_k=5000, top_k=750, threshold=float(E["sb_threshold"]))
    _s3fd(engine, E["sb_loc"][None], E[f"sb_conf_{variant}"][None], E["sb_priors"], size, par, [E[f"sb_rows_{variant}"]], exact=False)


# ------------------------------------------------------------------------------------------------ the shared order kernel's paths
# One order kernel serves both detectors (csrc/detect_tail.hip order_kernel), so each of them reaches sizes it did not before: S3FD
# the unrolled sort of 4096 and 8192 keys and compaction into LDS, RetinaFace the sorts below 2048 keys.  Disjoint boxes on a grid
# (NMS keeps every one, the oracles stay fast), scores drawn from 200 values so that long runs of ties cross every 2048-key boundary:
# the rows are the oracles' (tests/s3fd_ref.py, oracle/face.py, ties by the kernels' documented rule) bit for bit.
GRID = 256
SCORES = (np.float32(0.5) + np.arange(200, dtype=np.float32) / np.float32(512))   # 200 distinct values, all above both floors


def _scores(rng, p, n_cand):
    """[p] scores: n_cand candidates at random places with values of SCORES, the others under every confidence floor."""
    s = np.full(p, 0.01, np.float32)
    s[rng.permutation(p)[:n_cand]] = SCORES[rng.integers(0, len(SCORES), n_cand)]
    return s


def _s3fd_grid(cands, p, seed):
    """loc, conf, priors of len(cands) frames: prior i is a box of half a cell in cell (i % GRID, i // GRID) of a dyadic grid and loc
    is 0, so decode is exact; on a GRID x GRID image the boxes are half a pixel wide."""
    rng = np.random.default_rng(seed)
    i = np.arange(p)
    priors = np.stack([(i % GRID + 0.5) / GRID, (i // GRID + 0.5) / GRID, np.full(p, 0.5 / GRID), np.full(p, 0.5 / GRID)], 1).astype(np.float32)
    score = np.stack([_scores(rng, p, c) for c in cands])
    return np.zeros((len(cands), p, 4), np.float32), np.stack([1 - score, score], -1), priors


def _s3fd_grid_case(engine, cands, p, seed, par, rows):
    loc, conf, priors = _s3fd_grid(cands, p, seed)
    want = [s3fd_ref.detect(loc[t], conf[t], priors, GRID, GRID, par["threshold"], par["top_k"], par["conf_thresh"], par["nms_thresh"],
                            par["nms_top_k"], stable=True) for t in range(len(cands))]
    assert [len(w) for w in want] == rows
    _s3fd(engine, loc, conf, priors, (GRID, GRID), par, want, exact=True)


@pytest.mark.parametrize("top_k,rows", [(1024, [125, 228]), (7, [7, 7])])
def test_s3fd_through_the_unrolled_sort(engine, top_k, rows):
    """2049 candidates of 5000 priors (4096 keys, one exchange per thread and pass) and all 5000 (8192 keys, two); the walk stops at
    the cap top_k, and with top_k = 1024 the threshold, which is one of the scores, cuts the kept rows short."""
    par = dict(conf_thresh=0.05, nms_thresh=0.3, nms_top_k=6144, top_k=top_k, threshold=float(SCORES[190]))
    _s3fd_grid_case(engine, [2049, 5000], 5000, 1, par, rows)


def test_s3fd_counting_branch_at_its_first_size(engine):
    """16385 priors, every one a candidate: one key more than LDS holds, ranked by counting.  All top_k = 1024 rows are reported, so
    the first 1024 ranks, with their runs of some 80 tied scores, are checked one by one."""
    par = dict(conf_thresh=0.05, nms_thresh=0.3, nms_top_k=2000, top_k=1024, threshold=0.1)
    _s3fd_grid_case(engine, [16385], 16385, 2, par, [1024])


def test_s3fd_few_candidates_compacted_into_lds(engine):
    """300 priors (the keys are compacted into LDS, not memory) with 0, 1, 63, 64 and 65 candidates: the floor of 64 keys with padding,
    without, and the first size past it."""
    par = dict(conf_thresh=0.05, nms_thresh=0.3, nms_top_k=5000, top_k=750, threshold=0.1)
    _s3fd_grid_case(engine, [0, 1, 63, 64, 65], 300, 3, par, [0, 1, 63, 64, 65])


def test_retina_below_2048_candidates(engine):
    """0, 1, 63, 64, 65 and 2047 candidates among 3000 priors: the looped sort of 64 .. 1024 keys and, at 2047, the first unrolled one.
    The threshold sits on one of the scores, so the last selection cuts inside the kept rows."""
    rng = np.random.default_rng(4)
    cands, p = [0, 1, 63, 64, 65, 2047], 3000
    i = np.arange(p, dtype=np.float32)
    x, y = 4 * (i % 64), 4 * (i // 64)   # 2 x 2 pixel boxes ("+1" widths) 4 apart
    frames = np.stack([np.stack([x, y, x + 1, y + 1, _scores(rng, p, c)], 1) for c in cands]).astype(np.float32)
    par = dict(conf_thresh=0.02, nms_thresh=0.4, nms_top_k=5000, top_k=750, threshold=float(SCORES[100]))
    want = ec.retina_keep(frames, par)
    assert [len(k) for k in want[:5]] == [int((f[:, 4] >= SCORES[100]).sum()) for f in frames[:5]] and len(want[5]) == 750
    assert 0 < len(want[3]) < 64
    rows = ec.rows15(frames)
    got = _retina_nms(engine, rows, par, [rows[f, k] for f, k in enumerate(want)])
    for f, k in enumerate(want):
        assert got[f][:, 5].astype(int).tolist() == k.tolist()
        assert ec.same_bits(got[f], rows[f, k])
