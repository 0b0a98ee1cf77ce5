"""The fusion weight search on the device (csrc/search.hip through Engine.weight_search_counts and avcer_amd/weight_search.py).

Everything is exact: the kernel's outputs are integer counts, compared with `==` against the numpy statement of the kernel
(weight_search.counts_numpy, itself pinned to the reference bit for bit by tests/test_weight_search_cpu.py), and the mirrors'
returned weights against what the reference returned (tests/golden/weight_search.npz)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from avcer_amd import synth
from avcer_amd import weight_search as ws
from test_weight_search_cpu import CASES, C, case_inputs

pytestmark = pytest.mark.gpu


def device(engine, tables, labels, weights):
    tp, pred = engine.weight_search_counts(tables, labels, weights)
    assert tp.dtype == pred.dtype == torch.int32 and tp.is_cuda and pred.is_cuda
    assert tuple(tp.shape) == tuple(pred.shape) == (weights.shape[0], tables.shape[2])
    return tp.cpu().numpy(), pred.cpu().numpy()


def random_case(seed, n, m, c, w):
    rng = np.random.default_rng(seed)
    tables = rng.random((m, n, c))
    labels = rng.integers(0, c, size=n)
    weights = rng.dirichlet(np.ones(m), size=(w, c)).transpose(0, 2, 1).copy()
    return tables, labels, weights


@pytest.mark.parametrize("name", CASES)
def test_device_counts_equal_the_statement_on_every_golden_case(engine, golden, name):
    g = golden("weight_search")
    labels, tables, weights = case_inputs(g, name)
    tp, pred = device(engine, tables, labels, weights)
    want_tp, want_pred = ws.counts_numpy(tables, labels, weights)
    assert np.array_equal(pred, g[f"{name}_hist"].astype(np.int32))
    assert np.array_equal(tp, want_tp) and np.array_equal(pred, want_pred)
    r = ws.result_from_counts(tp, pred, labels, weights)
    assert np.array_equal(r.metric.view(np.uint64), g[f"{name}_metric"].view(np.uint64))


def test_device_counts_equal_the_statement_at_200k_frames_by_4096_candidates(engine):
    """The statement is evaluated on a subset: every 16th candidate (0, 16, ..., 4080: 256 of them, spread over every block of
    the launch); the pred rows of ALL candidates must also sum to the frame count."""
    n, m, w = 200_000, 3, 4096
    labels, tables = synth.fusion_tables(7, n, m, C)
    np.random.seed(7)
    weights = ws.dirichlet_weights(w, m, C)
    tp, pred = device(engine, tables, labels, weights)
    assert (pred.sum(axis=1) == n).all() and (tp <= pred).all()
    subset = np.arange(0, w, 16)
    want_tp, want_pred = ws.counts_numpy(tables, labels, weights[subset])
    assert np.array_equal(tp[subset], want_tp) and np.array_equal(pred[subset], want_pred)


@pytest.mark.parametrize("name,fn", (("prob_m2", "prob"), ("prob_m3", "prob"), ("prob_m3_label7", "prob"), ("prob_m2_tie", "prob"),
                                     ("grid_v", "v"), ("grid_av", "av")))
def test_mirrors_return_the_reference_weights(engine, golden, name, fn):
    g = golden("weight_search")
    seed, n, m, label_classes, w = (int(v) for v in g[f"{name}_params"])
    labels, tables = synth.fusion_tables(seed, n, m, C, label_classes)
    np.random.seed(42)
    if fn == "prob":
        got = ws.get_weights_prob_model(engine, labels, list(tables), w, C)
    elif fn == "v":
        got = ws.get_weights_v_model(engine, g["grid"], labels, list(tables))
    else:
        got = ws.get_weights_av_model(engine, g["grid"], labels, list(tables))
    assert np.array_equal(np.asarray(got), g[f"{name}_best"])


def test_counts_are_identical_across_calls_and_uneven_splits(engine):
    tables, labels, weights = random_case(11, 5000, 3, 7, 1000)
    tp, pred = device(engine, tables, labels, weights)
    tp2, pred2 = device(engine, tables, labels, weights)
    assert np.array_equal(tp, tp2) and np.array_equal(pred, pred2)
    cuts = [0, 1, 258, 300, 811, 1000]  # launches of 1, 257, 42, 511 and 189 candidates
    parts = [device(engine, tables, labels, weights[a:b]) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), tp) and np.array_equal(np.concatenate([p[1] for p in parts]), pred)
    tp3, pred3 = ws.device_counts(engine, tables, labels, weights, max_pairs=5000 * 77)
    assert np.array_equal(tp3, tp) and np.array_equal(pred3, pred)
    want = ws.counts_numpy(tables, labels, weights)
    assert np.array_equal(tp, want[0]) and np.array_equal(pred, want[1])


@pytest.mark.parametrize("m", (1, 2, 3, 4))
@pytest.mark.parametrize("c", (2, 3, 4, 5, 6, 7, 8))
def test_every_model_and_class_count(engine, m, c):
    tables, labels, weights = random_case(100 * m + c, 700, m, c, 300)  # three uneven slabs, a partly filled second block
    labels[::50] = c  # a label no table has
    tp, pred = device(engine, tables, labels, weights)
    want_tp, want_pred = ws.counts_numpy(tables, labels, weights)
    assert np.array_equal(tp, want_tp) and np.array_equal(pred, want_pred)


def test_nan_rows_and_float32_tables(engine):
    tables, labels, weights = random_case(5, 400, 2, 7, 64)
    tables = tables.astype(np.float32)
    tables[0, 3, [2, 5]] = np.nan
    tables[1, 9, 6] = np.nan
    tables[0, 11, 0] = np.inf
    weights[1, 0, 0] = 0.0  # inf * 0
    with np.errstate(invalid="ignore"):
        want_tp, want_pred = ws.counts_numpy(tables, labels, weights)
    tp, pred = device(engine, tables, labels, weights)
    assert np.array_equal(tp, want_tp) and np.array_equal(pred, want_pred)


def test_invalid_sizes(engine):
    tables, labels, weights = random_case(1, 64, 2, 7, 8)
    for bad in ((np.ones((5, 64, 7)), labels, np.ones((8, 5, 7))),      # M = 5
                (np.ones((2, 64, 9)), labels, np.ones((8, 2, 9))),      # C = 9
                (np.ones((2, 64, 1)), labels, np.ones((8, 2, 1))),      # C = 1
                (tables, labels, weights[:0]),                          # W = 0
                (tables[:, :0], labels[:0], weights),                   # N = 0
                (tables, labels[:-1], weights),                         # labels disagree
                (tables, labels, weights[:, :1]),                       # weights disagree
                (tables[0], labels, weights)):                          # rank
        with pytest.raises(ValueError):
            engine.weight_search_counts(*bad)
    # the entry point itself refuses them with AVCER_EINVAL (-1) before it touches a buffer
    buf = torch.zeros(4096, dtype=torch.float64, device=engine.device)
    p = ctypes.c_void_p(buf.data_ptr())
    for n, m, c, w in ((64, 5, 7, 8), (64, 0, 7, 8), (64, 2, 9, 8), (64, 2, 1, 8), (0, 2, 7, 8), (2 ** 31, 2, 7, 8), (64, 2, 7, 0),
                       (64, 2, 7, 2 ** 24 + 1)):
        assert engine.lib.avcer_weight_search_counts(engine.ctx, p, p, n, m, c, p, w, p, p, engine._stream()) == -1, (n, m, c, w)


def fl(x: Fraction) -> float:
    return float(x)  # int / int true division: correctly rounded to nearest-even


def contraction_frames(draws=400, m=3, seed=3):
    """Frames on which an FMA-chained sum picks another class than the separately rounded one.

    One candidate w [m, C].  Per draw, classes a < b and class a's probabilities p[0..m): the reference's value is
    S = fl(fl(p0 w0) + fl(p1 w1)) ..., the contracted chain is T = fma(p_i, w_i, T) from T = fl(p0 w0), computed exactly in
    rationals.  Draws with T < S are kept.  Class b gets one non-zero probability q (model 0) with fl(q * w[0][b]) == S, found
    within a few ulps of S / w[0][b]; every other entry of the frame is 0.  Then the reference ties and takes a, the first;
    a contracted kernel sees T < S and takes b."""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.ones(m), size=C).T.copy()  # [m, C]
    frames, picks = [], []
    for _ in range(draws):
        a, b = sorted(rng.choice(C, size=2, replace=False).tolist())
        p = rng.random(m)
        s = p[0] * w[0, a]
        t = s
        for i in range(1, m):
            s = s + p[i] * w[i, a]
            t = fl(Fraction(p[i]) * Fraction(w[i, a]) + Fraction(t))
        if not t < s:
            continue
        q = s / w[0, b]
        cands = [q]
        for _ in range(4):
            cands = [np.nextafter(cands[0], -np.inf)] + cands + [np.nextafter(cands[-1], np.inf)]
        q = next((x for x in cands if x * w[0, b] == s), None)
        if q is None:
            continue
        row = np.zeros((m, C))
        row[:, a] = p
        row[0, b] = q
        frames.append(row)
        picks.append((a, b))
    tables = np.stack(frames, axis=1)  # [m, frames, C]
    return tables, np.array(picks), w


def test_contraction_guard(engine):
    tables, picks, w = contraction_frames()
    n = tables.shape[1]
    print("qualifying frames with a tie partner:", n)
    assert n >= 16
    labels = picks[:, 0]
    weights = np.concatenate([w[None], random_case(2, 1, 3, C, 7)[2]])  # the directed candidate and seven ordinary ones
    want_tp, want_pred = ws.counts_numpy(tables, labels, weights)
    # the construction holds: the statement takes a on every frame, the rational FMA chain takes b
    assert want_pred[0].tolist() == np.bincount(picks[:, 0], minlength=C).tolist() and want_tp[0].sum() == n
    for i, (a, b) in enumerate(picks):
        chain = []
        for cl in (a, b):
            t = tables[0, i, cl] * w[0, cl]
            for k in range(1, 3):
                t = fl(Fraction(tables[k, i, cl]) * Fraction(w[k, cl]) + Fraction(t))
            chain.append(t)
        assert chain[0] < chain[1]
    tp, pred = device(engine, tables, labels, weights)
    assert np.array_equal(pred, want_pred) and np.array_equal(tp, want_tp)
