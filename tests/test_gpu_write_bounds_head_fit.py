"""Guard bands (tests/guard_band.py) around the outputs of avcer_head_fit and avcer_head_apply, in the style of
tests/test_gpu_write_bounds_post.py: every output is a band of one `check` call and every device input is in `inputs`; guards
untouched, every element written, the same bits in all three runs, the inputs unchanged.  The C entries are called through
engine.lib so that the guarded buffers are the ones written.

  avcer_head_fit    w_hist, b_hist, batch_loss, epoch_loss; F = 64 (threads 64 .. 255 own no column), F = 320 (the second column
                    of threads 64 .. 255 is past the row's end), F = 1024 with C = 8 and F = 256 with C = 16 (the two register
                    placements), C = 7 and 2 (class slots past the last class); a short last batch; K = 3 runs
  avcer_head_apply  m = 1, 15, 16, 17 rows against blocks of 16 rows and waves of 4; H = 1 and 5 heads"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_fit_cases as cases
from avcer_amd import head_fit as hf
from avcer_amd.engine import _ptr
from guard_band import Band, check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f,c", [(64, 7), (320, 2), (1024, 8), (256, 16)])
def test_head_fit_writes_its_outputs_and_nothing_else(engine, f, c):
    n, bsz, epochs = 37, 16, 2
    rs = np.random.RandomState(f + c)
    feats = (rs.standard_normal((n, f)) * 0.5).astype(np.float32)
    targets = rs.randint(0, c, n)
    runs = []
    for k in range(3):
        run = hf.HeadRun(w0=(rs.standard_normal((c, f)) * 0.05).astype(np.float32), b0=np.zeros(c, np.float32),
                         order=hf.make_order(n, epochs, seed=k), kind=("ce", "soft_focal", "ce")[k], gamma=2.0, lr=1e-3, t0=2)
        if k:
            run.mix_lam, run.mix_index = hf.make_mixup(n, epochs, bsz, 0.3, seed=k)
        runs.append(run)
    pk = hf._pack(feats.shape, targets, runs, epochs, bsz, 1)
    dev = engine.device
    x, t, cw, w0, b0, order, lam, idx = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in
                                        (feats, pk.targets, pk.class_w, pk.w0, pk.b0, pk.order, pk.mix_lam, pk.mix_index))
    scratch = torch.zeros(3, hf.HYPER, dtype=torch.float64, device=dev)

    def run_call(outs):
        engine._check(engine.lib.avcer_head_fit(engine.ctx, _ptr(x), _ptr(t), n, f, c, 3, epochs, bsz, pk.hyper.ctypes.data_as(C.c_void_p),
                                                _ptr(scratch), _ptr(cw), _ptr(w0), _ptr(b0), _ptr(order), _ptr(lam), _ptr(idx),
                                                *(_ptr(o) for o in outs), engine._stream()))

    bands = [Band("w_hist", (3, epochs, c, f), torch.float32), Band("b_hist", (3, epochs, c), torch.float32),
             Band("batch_loss", (3, epochs, 3), torch.float32), Band("epoch_loss", (3, epochs), torch.float64)]
    w_hist, b_hist, batch_loss, epoch_loss = check(run_call, bands, [x, t, cw, w0, b0, order, lam, idx], device=dev)
    assert all(torch.isfinite(v).all() for v in (w_hist, b_hist, batch_loss, epoch_loss))
    want = (batch_loss.double() * bsz).sum(dim=2) / 3
    assert float((epoch_loss - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("m", [1, 15, 16, 17])
@pytest.mark.parametrize("heads", [1, 5])
def test_head_apply_writes_its_logits_and_nothing_else(engine, m, heads):
    f, c = 192, 7
    rng = np.random.default_rng([m, heads])
    x, w, b = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(engine.device) for s in ((m, f), (heads, c, f), (heads, c)))

    def run_call(outs):
        engine._check(engine.lib.avcer_head_apply(engine.ctx, _ptr(x), _ptr(w), _ptr(b), m, f, c, heads, _ptr(outs[0]), engine._stream()))

    got, = check(run_call, [Band("logits", (heads, m, c), torch.float32)], [x, w, b], device=engine.device)
    want = torch.einsum("mf,hcf->hmc", x.double(), w.double()).cpu() + b.double().cpu()[:, None, :]
    assert float((got.double() - want).abs().max()) <= 1e-4
