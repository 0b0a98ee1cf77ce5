"""Guard bands (tests/guard_band.py) around every output of avcer_eval_tables and avcer_eval_confusion: only the output is written,
all of it, the same bits in every run, the inputs unchanged.  The values are the business of tests/test_gpu_evaluate.py."""
import numpy as np
import pytest
import torch

from avcer_amd import evaluate as ev
from guard_band import Band, check

pytestmark = pytest.mark.gpu


def _case(seed=3):
    rng = np.random.default_rng(seed)
    keys = [rng.permutation(np.repeat(np.arange(4, 41), 3)), np.array([9, 2, 2]), rng.permutation(np.arange(300))]
    rows = [rng.normal(0, 3, size=(len(k), 8)) for k in keys]
    need = [np.arange(0, 45, 2), np.zeros(0, dtype=np.int64), np.arange(1, 299, 3)]
    return rows, keys, need, [30, 0, 101]


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("video_level", [False, True])
def test_eval_tables_bounds(engine, keyed, video_level):
    rows, keys, need, out_counts = _case()
    t = ev._keyed_table("audio", rows, keys, out_counts) if keyed else ev._plain_table("dyn", rows, out_counts, True)
    x = torch.from_numpy(t.rows).to(engine.device)
    k = torch.from_numpy(t.keys).to(engine.device) if keyed else None
    n_out = len(rows) if video_level else sum(out_counts)

    def run(outs):
        engine.eval_tables(x, t.row_counts, np.concatenate(need), [len(n) for n in need], t.out_counts, True, video_level, k, t.key_lo,
                           t.key_spans, out=outs[0])

    out, = check(run, [Band("out", (n_out, 7), torch.float64)], inputs=[x] + ([k] if keyed else []), device=engine.device)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("n", [1, 777])
def test_eval_confusion_bounds(engine, n):
    rng = np.random.default_rng(n)
    tables = torch.from_numpy(rng.random((2, n, 7))).to(engine.device)
    labels = torch.from_numpy(rng.integers(-1, 8, size=n).astype(np.int32)).to(engine.device)
    w1, w2 = rng.random((2, 7)), rng.random(2)

    def run(outs):
        engine.eval_confusion(tables, labels, w1, w2, pred=outs[0], cm=outs[1])

    pred, cm = check(run, [Band("pred", (n,), torch.int32), Band("cm", (7, 7), torch.int64)], inputs=[tables, labels],
                     device=engine.device)
    assert int(cm.sum()) == int(((labels >= 0) & (labels < 7)).sum()) and int(pred.min()) >= 0 and int(pred.max()) <= 6
