"""Host side of the fusion weight search (avcer_amd/weight_search.py) against tests/golden/weight_search.npz: the reference's
unmodified get_weights_prob_model / get_weights_v_model / get_weights_av_model with sklearn's classification_report, recorded
per candidate (tests/golden/make_golden_weight_search.py).  Everything here is exact: metrics are compared bit for bit.

The mirrors take an engine; here it is a stand-in whose one kernel entry is the numpy statement of the kernel (counts_numpy),
so that candidate generation, launch splitting, metrics and selection run without a GPU.  tests/test_gpu_weight_search.py runs
the same mirrors on the device."""
import numpy as np
import pytest
import torch

from avcer_amd import synth
from avcer_amd import weight_search as ws

CASES = ("prob_m2", "prob_m3", "prob_m3_label7", "prob_m2_tie", "grid_v", "grid_av")
C = 7


def case_inputs(g, name):
    """The tables, labels and candidates of a stored case, regenerated (only results are stored)."""
    seed, n, m, label_classes, w = (int(v) for v in g[f"{name}_params"])
    labels, tables = synth.fusion_tables(seed, n, m, C, label_classes)
    if name.startswith("prob"):
        np.random.seed(42)
        weights = ws.dirichlet_weights(w, m, C)
    else:
        weights = ws.grid_weights(g["grid"], m, C)
    assert weights.shape == (w, m, C)
    return labels, tables, weights


class NumpyEngine:
    """Engine stand-in: the kernel entry answered by its numpy statement, tensors on the CPU."""

    def __init__(self):
        self.launches = []

    def _dev(self, t, dtype):
        return torch.as_tensor(np.asarray(t)).to(dtype).contiguous()

    def weight_search_counts(self, preds, labels, weights):
        self.launches.append(int(np.asarray(weights).shape[0]))
        tp, pred = ws.counts_numpy(preds.numpy(), labels.numpy(), np.asarray(weights))
        return torch.from_numpy(tp), torch.from_numpy(pred)


@pytest.mark.parametrize("name", CASES)
def test_counts_metrics_and_selection_reproduce_the_reference(golden, name):
    g = golden("weight_search")
    labels, tables, weights = case_inputs(g, name)
    tp, pred = ws.counts_numpy(tables, labels, weights)
    assert np.array_equal(pred, g[f"{name}_hist"].astype(np.int32))
    r = ws.result_from_counts(tp, pred, labels, weights)
    stored = g[f"{name}_metric"]
    assert r.metric.dtype == np.float64 and np.array_equal(r.metric.view(np.uint64), stored.view(np.uint64))  # bit for bit
    assert r.best_index == int(np.argmax(stored)) and r.best_metric == stored.max()
    assert np.array_equal(r.best_weights[:, 0] if name.startswith("grid") else r.best_weights, g[f"{name}_best"])


@pytest.mark.parametrize("name", ("prob_m2_tie", "grid_v", "grid_av"))
def test_the_first_of_several_maxima_wins(golden, name):
    g = golden("weight_search")
    stored = g[f"{name}_metric"]
    sharing = np.flatnonzero(stored == stored.max())
    assert len(sharing) >= 2  # the fixture's point: the reference's strict `>` keeps the first
    assert ws.select(stored) == (int(sharing[0]), float(stored.max()))


@pytest.mark.parametrize("name", ("prob_m2", "prob_m3", "prob_m3_label7", "prob_m2_tie"))
def test_dirichlet_weights_consume_the_reference_stream(golden, name):
    g = golden("weight_search")
    _, _, m, _, w = (int(v) for v in g[f"{name}_params"])
    np.random.seed(42)
    weights = ws.dirichlet_weights(w, m, C)
    assert np.array_equal(weights[int(np.argmax(g[f"{name}_metric"]))], g[f"{name}_best"])
    assert np.allclose(weights.sum(axis=1), 1.0)


def test_grid_weights_follow_the_reference_loops():
    values = [0.5, 0.25, 2.0]
    expect2 = [(a, b) for a in values for b in values]
    expect3 = [(a, b, c) for a in values for b in values for c in values]
    assert np.array_equal(ws.grid_weights(values, 2)[:, :, 0], np.array(expect2))
    g3 = ws.grid_weights(values, 3, 7)
    assert g3.shape == (27, 3, 7) and np.array_equal(g3[:, :, 0], np.array(expect3))
    assert all(np.array_equal(g3[:, :, c], g3[:, :, 0]) for c in range(7))


@pytest.mark.parametrize("name,fn", (("prob_m3_label7", "prob"), ("grid_v", "v"), ("grid_av", "av")))
def test_mirrors_return_the_reference_weights_and_split_launches(golden, name, fn, monkeypatch):
    g = golden("weight_search")
    seed, n, m, label_classes, w = (int(v) for v in g[f"{name}_params"])
    labels, tables = synth.fusion_tables(seed, n, m, C, label_classes)
    monkeypatch.setattr(ws, "MAX_PAIRS_PER_LAUNCH", 77 * n)  # uneven launches of 77 candidates
    eng = NumpyEngine()
    np.random.seed(42)
    if fn == "prob":
        got = ws.get_weights_prob_model(eng, labels, list(tables), w, C)
    elif fn == "v":
        got = ws.get_weights_v_model(eng, g["grid"], labels, list(tables))
    else:
        got = ws.get_weights_av_model(eng, g["grid"], labels, list(tables))
    assert np.array_equal(np.asarray(got), g[f"{name}_best"])
    assert eng.launches == [77] * (w // 77) + ([w % 77] if w % 77 else [])
    if fn != "prob":
        assert isinstance(got, list) and len(got) == m


def zero_metric_tables(m):
    """Every class 1..6 is predicted by every candidate and none is ever right: each metric is 0, nothing is selected."""
    n = 12
    tables = np.full((m, n, C), 0.01)
    tables[:, np.arange(n), 1 + np.arange(n) % 6] = 0.9
    return np.zeros(n, dtype=np.int64), tables


def test_nothing_selected_returns():
    eng = NumpyEngine()
    labels, t3 = zero_metric_tables(3)
    np.random.seed(42)
    assert ws.get_weights_prob_model(eng, labels, list(t3), 20, C) is None
    assert ws.get_weights_v_model(eng, [0.1, 0.2], labels, list(t3[:2])) == [0, 0]
    assert ws.get_weights_av_model(eng, [0.1, 0.2], labels, list(t3)) == [0, 0, 0]
    r = ws.search(eng, labels, list(t3), ws.grid_weights([0.1, 0.2], 3, C))
    assert r.best_index is None and r.best_weights is None and r.best_metric == 0.0 and not r.metric.any()


def test_a_class_in_neither_labels_nor_predictions_is_a_key_error():
    labels = np.array([0, 1, 2, 3, 5, 6] * 3)  # no 4 ...
    tables = np.full((2, labels.size, C), 0.01)
    tables[:, np.arange(labels.size), labels] = 0.9  # ... and no model ever picks it
    tp, pred = ws.counts_numpy(tables, labels, ws.grid_weights([0.3, 0.7], 2, C))
    with pytest.raises(KeyError) as e:
        ws.metrics_from_counts(tp, pred, np.bincount(labels, minlength=C))
    assert e.value.args == ("4",)
    # predicted once (wrongly) is enough for the report to carry it: precision, recall and F1 of 0 / 0-support are 0.0
    tables[0, 0] = tables[1, 0] = np.eye(C)[4]
    tp, pred = ws.counts_numpy(tables, labels, ws.grid_weights([0.3, 0.7], 2, C))
    p, f1, r, _ = ws.metrics_from_counts(tp, pred, np.bincount(labels, minlength=C))
    assert (p[:, 4] == 0).all() and (r[:, 4] == 0).all() and (f1[:, 4] == 0).all()


def test_nan_is_the_maximum_and_the_first_nan_wins():
    tables = np.array([[[0.1, 0.9, 0.0, np.nan, 0.0, np.nan, 0.0],     # two NaN: the first one
                        [0.1, 0.2, 0.7, 0.0, 0.0, 0.0, 0.0],           # none
                        [np.inf, 0.0, 0.0, 0.0, np.nan, 0.0, 0.0],     # NaN beats +inf
                        [0.3, 0.3, 0.3, 0.0, 0.0, 0.0, 0.0],           # tie: the first
                        [np.nan, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0]]])      # NaN in class 0 stays
    labels = np.array([3, 2, 4, 1, 0])
    weights = np.ones((2, 1, C))
    weights[1, 0, 0] = 0.0  # inf * 0 = NaN in class 0 of row 2: now the first NaN
    with np.errstate(invalid="ignore"):
        tp, pred = ws.counts_numpy(tables, labels, weights)
    assert pred.tolist() == [[2, 0, 1, 1, 1, 0, 0], [2, 1, 1, 1, 0, 0, 0]]
    assert tp.tolist() == [[1, 0, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 0, 0]]


def test_float32_tables_are_promoted_like_numpy(golden):
    g = golden("weight_search")
    labels, tables, weights = case_inputs(g, "prob_m2")
    assert tables.dtype == np.float32
    k = 5
    f = tables[0] * weights[k, 0]
    f += tables[1] * weights[k, 1]
    assert f.dtype == np.float64  # numpy: float32 array times float64 array
    tp, pred = ws.counts_numpy(tables, labels, weights[k:k + 1])
    assert np.array_equal(pred[0], np.bincount(np.argmax(f, axis=-1), minlength=C))
    tp64, pred64 = ws.counts_numpy(tables.astype(np.float64), labels, weights[k:k + 1])
    assert np.array_equal(tp, tp64) and np.array_equal(pred, pred64)


def test_shape_errors():
    labels, tables = synth.fusion_tables(1, 50, 2, C)
    with pytest.raises(ValueError):
        ws.counts_numpy(tables, labels, np.ones((3, 3, C)))
    with pytest.raises(ValueError):
        ws.counts_numpy(tables, labels[:-1], np.ones((3, 2, C)))
    with pytest.raises(ValueError):
        ws.search(NumpyEngine(), labels[:-1], list(tables), np.ones((3, 2, C)))
