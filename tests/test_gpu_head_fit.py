"""Fitting the audio classifier head on the device (avcer_amd/head_fit.py, csrc/head_fit.hip).

1. avcer_head_fit against head_fit_numpy (float64) on w_hist, b_hist and batch_loss, K runs in one launch, within
   max(4 * f32_dev of the run, the largest f32_dev of the case): f32_dev is how far torch's float32 run of the same iteration lies
   from the float64 one (tests/golden/head_fit.npz for the golden cases, tests/head_fit_cases.f32_deviation for the others).
   Kernel and torch are both float32 chains of the same steps that differ in the order of their sums; the factor covers the
   order.  epoch_loss is a float64 sum of the float32 batch losses: it is held to n_batches * batch_size * that tolerance / n_batches.
   The figures are printed (-s) before they are asserted.
2. Two calls give the same bits.  3. A run alone gives the bits it gives among K; a head alone the logits it gives among 12.
4. Short and single-row batches: n = 1, n = B, n = B + 1, and batch_size = 256 with n = 300.
5. head_apply against its float64 statement.  6. Limits: AVCER_EINVAL before any launch.
7. select's best epochs are validate.best_epoch over stats made from head_fit_numpy.
8. End to end: extract_features -> fit_heads -> write_checkpoint -> load_audio -> run_corpus gives the softmax of head_apply on the
   extracted features within the project's 1e-4 probability gate, with equal argmax.
The guard bands of both entries: tests/test_gpu_write_bounds_head_fit.py."""
import os

import numpy as np
import pytest
import torch

import head_fit_cases as cases
from avcer_amd import audio_corpus as ac
from avcer_amd import head_fit as hf
from avcer_amd import synth
from avcer_amd import validate as va
from avcer_amd._lib import AvcerError
from avcer_amd.engine import Engine

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_fit.npz"))
PROB_GATE = 1e-4


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a: hf.HeadFit, b: hf.HeadFit, rows=slice(None)):
    return all(np.array_equal(_bits(x)[rows], _bits(y)) for x, y in zip(a[:4], b[:4]))


def _against_statement(engine, name, feats, targets, runs, bsz, devs, epochs=cases.EPOCHS):
    fit = hf.fit_heads(engine, torch.from_numpy(feats).to(engine.device), targets, list(runs.values()), epochs, bsz)
    want = hf.head_fit_numpy(feats, targets, list(runs.values()), epochs, bsz)
    got = [a.cpu().numpy() for a in fit[:4]]
    n_batches = -(-feats.shape[0] // bsz)
    assert got[0].shape == (len(runs), epochs) + runs[next(iter(runs))].w0.shape and got[2].shape == (len(runs), epochs, n_batches)
    assert got[0].dtype == got[1].dtype == got[2].dtype == np.float32 and got[3].dtype == np.float64
    floor = max(devs.values())
    worst = []
    for k, r in enumerate(runs):
        tol = max(4.0 * devs[r], floor)
        dev = cases.deviation([g[k] for g in got[:3]], want[k])
        epoch_dev = float(np.abs(got[3][k] - want[k].epoch_loss).max())
        print(f"head_fit {name:10s} {r:10s} f32_dev {devs[r]:.3e}  tolerance {tol:.3e}  kernel - statement {dev:.3e}  epoch_loss {epoch_dev:.3e}")
        worst.append((r, dev, tol, epoch_dev))
    for r, dev, tol, epoch_dev in worst:
        assert np.isfinite(dev) and dev <= tol, (name, r, dev, tol)
        assert epoch_dev <= bsz * tol, (name, r, epoch_dev, bsz * tol)   # sum_b(loss_b * B) / n_batches: B times a batch loss's error
    return fit


@pytest.mark.parametrize("name", list(cases.GOLDEN) + list(cases.GPU_ONLY))
def test_kernel_against_the_statement(engine, name):
    """Measured on MI355X: see DESIGN.md section 5 (head_fit)."""
    feats, targets, runs, bsz = cases.inputs(name)
    if name in cases.GOLDEN:
        devs = {r: float(GOLD[f"{name}/{r}/f32_dev"]) for r in runs}
    else:
        want = hf.head_fit_numpy(feats, targets, list(runs.values()), cases.EPOCHS, bsz)
        devs = {r: cases.deviation(cases.torch_fit(feats, targets, run, bsz, torch.float32), want[k]) for k, (r, run) in enumerate(runs.items())}
    assert len(runs) >= 2 and all(d > 0 for d in devs.values())
    _against_statement(engine, name, feats, targets, runs, bsz, devs)


@pytest.mark.parametrize("n,bsz", [(17, 16), (300, 256)], ids=["n_is_B_plus_1", "B256_n300"])
def test_short_batches(engine, n, bsz):
    """n = 1 and n = B are the golden cases one_row and one_batch above."""
    feats, targets, runs, bsz = cases.inputs("f64_c7", n=n, bsz=bsz, epochs=2)
    want = hf.head_fit_numpy(feats, targets, list(runs.values()), 2, bsz)
    devs = {r: cases.deviation(cases.torch_fit(feats, targets, run, bsz, torch.float32, epochs=2), want[k]) for k, (r, run) in enumerate(runs.items())}
    fit = _against_statement(engine, f"n{n}_B{bsz}", feats, targets, runs, bsz, devs, epochs=2)
    assert tuple(fit.batch_loss.shape) == (4, 2, 2)


def test_two_calls_give_the_same_bits_and_a_run_alone_its_bits_among_many(engine):
    feats, targets, more, bsz = cases.inputs("f1024_c8")
    runs = list(more.values())
    x = torch.from_numpy(feats).to(engine.device)
    a = hf.fit_heads(engine, x, targets, runs, cases.EPOCHS, bsz)
    b = hf.fit_heads(engine, x, targets, runs, cases.EPOCHS, bsz)
    assert _same(a, b) and torch.isfinite(a.w_hist).all()
    for k, run in enumerate(runs):
        alone = hf.fit_heads(engine, x, targets, [run], cases.EPOCHS, bsz)
        assert _same(a, alone, slice(k, k + 1)), k
    assert not np.array_equal(_bits(a.w_hist)[0], _bits(a.w_hist)[1])


def test_head_apply_against_its_statement_and_a_head_alone(engine):
    """|error| <= (F / 64 + 7) * 2^-24 * (|x| . |w| + |b|): a lane's fmaf chain of F / 64 terms, six folds and the bias, each one
    rounding of a partial sum that |x| . |w| + |b| bounds."""
    for name, m in (("f64_c7", 1), ("f256_c16", 37), ("f1024_c8", 70)):
        f, c, _, _ = cases.shape(name)
        rng = np.random.default_rng([f, c, m])
        x = rng.standard_normal((m, f)).astype(np.float32)
        w, b = rng.standard_normal((12, c, f)).astype(np.float32), rng.standard_normal((12, c)).astype(np.float32)
        dx, dw, db = (torch.from_numpy(v).to(engine.device) for v in (x, w, b))
        got = engine.head_apply(dx, dw, db)
        assert tuple(got.shape) == (12, m, c) and got.dtype == torch.float32
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        want = np.einsum("mf,hcf->hmc", x64, w64) + b[:, None, :]
        bound = (f / 64 + 7) * 2.0 ** -24 * (np.einsum("mf,hcf->hmc", np.abs(x64), np.abs(w64)) + np.abs(b)[:, None, :])
        err = np.abs(got.cpu().numpy() - want)
        print(f"head_apply {name}: worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        for h in (0, 5, 11):
            one = engine.head_apply(dx, dw[h:h + 1], db[h:h + 1])
            assert np.array_equal(_bits(one)[0], _bits(got)[h]), (name, h)
    with pytest.raises(ValueError):
        engine.head_apply(dx, dw, db[:, :-1])


def test_limits_are_refused_before_any_launch(engine):
    feats, targets, runs, bsz = cases.inputs("one_batch", epochs=2)
    pk = hf._pack(feats.shape, targets, [runs["ce_w_mix"]], 2, bsz, 1)

    def call(**change):
        a = dict(feats=feats, targets=pk.targets, hyper=pk.hyper, class_w=pk.class_w, w0=pk.w0, b0=pk.b0, order=pk.order,
                 mix_lam=pk.mix_lam, mix_index=pk.mix_index, epochs=2, batch_size=bsz)
        a.update(change)
        return engine.head_fit(**a)

    call()
    def hyper(slot, value):
        h = pk.hyper.copy()
        h[0, slot] = value
        return h

    c17 = dict(w0=np.zeros((1, 17, 64), np.float32), b0=np.zeros((1, 17), np.float32), class_w=np.ones((1, 17), np.float32))
    c1 = dict(w0=np.zeros((1, 1, 64), np.float32), b0=np.zeros((1, 1), np.float32), class_w=np.ones((1, 1), np.float32))
    wide = dict(feats=np.zeros((16, 1088), np.float32), w0=np.zeros((1, 8, 1088), np.float32))
    odd = dict(feats=np.zeros((16, 96), np.float32), w0=np.zeros((1, 8, 96), np.float32))
    for bad in (c17, c1, wide, odd, dict(batch_size=257, order=pk.order), dict(hyper=hyper(0, 2.0)), dict(hyper=hyper(1, 1.5)),
                dict(hyper=hyper(2, -1.0)), dict(hyper=hyper(3, np.nan)), dict(hyper=hyper(4, 1.0)), dict(hyper=hyper(6, np.inf)),
                dict(hyper=hyper(7, 0.0)), dict(hyper=hyper(7, 2.5)), dict(hyper=hyper(8, np.inf)), dict(hyper=hyper(9, 0.5)),
                dict(hyper=hyper(10, -1.0))):
        with pytest.raises(AvcerError) as err:
            call(**bad)
        assert err.value.code == -1 and "head fit" in str(err.value), bad.keys()
    h = pk.hyper.copy()
    with pytest.raises(AvcerError, match="mixup without its tables"):
        call(mix_lam=None, mix_index=None, hyper=h)
    for bad in (dict(epochs=0, order=pk.order[:, :0]), dict(epochs=3), dict(mix_lam=None), dict(b0=pk.b0[:, :-1]), dict(targets=pk.targets[:-1])):
        with pytest.raises((ValueError, AvcerError)):
            call(**bad)
    x, w, b = torch.zeros(4, 64), torch.zeros(2, 17, 64), torch.zeros(2, 17)
    with pytest.raises(AvcerError, match="head apply"):
        engine.head_apply(x, w, b)
    with pytest.raises(AvcerError, match="head apply"):
        engine.head_apply(torch.zeros(4, 96), torch.zeros(2, 8, 96), torch.zeros(2, 8))
    with pytest.raises(AvcerError, match="head apply"):
        engine.head_apply(torch.zeros(0, 64), torch.zeros(2, 8, 64), torch.zeros(2, 8))
    with pytest.raises(ValueError):   # fit_heads checks on the host what head_fit_numpy checks
        hf.fit_heads(engine, torch.from_numpy(feats), targets, [runs["ce"]], 2, 257)


def test_select_names_the_best_epoch_of_the_statement(engine):
    feats, targets, runs, bsz = cases.inputs("f64_c7")
    dev_feats, dev_targets, _, _ = cases.inputs("f64_c7", n=50)
    names = list(va.C_NAMES[7])
    metrics = ("recall", "f1", "accuracy")
    weights = runs["ce_w_mix"].weights
    fit = hf.fit_heads(engine, torch.from_numpy(feats).to(engine.device), targets, list(runs.values()), cases.EPOCHS, bsz, first_epoch=4)
    picked = hf.select(engine, fit, torch.from_numpy(dev_feats).to(engine.device), dev_targets, names, metrics, "ce", weights, batch_size=8)
    want = hf.head_fit_numpy(feats, targets, list(runs.values()), cases.EPOCHS, bsz, first_epoch=4)
    assert len(picked) == len(runs)
    for (stats, best), w in zip(picked, want):
        rows = []
        for e in range(cases.EPOCHS):
            logits = (dev_feats.astype(np.float64) @ w.w_hist[e].T + w.b_hist[e]).astype(np.float32)
            probs = np.exp(logits - logits.max(axis=1, keepdims=True))
            perf = va.measures(va.NumpyEngine(), dev_targets, probs / probs.sum(axis=1, keepdims=True), names, metrics)
            row = {"epoch": 4 + e, "devel_loss": va.losses_numpy(logits, dev_targets, "ce", weights, 0.2, 0.0, 8).epoch}
            row.update({f"devel_{m}": perf[m] for m in metrics})
            rows.append(row)
        assert [list(r) for r in stats] == [list(r) for r in rows] and [r["epoch"] for r in stats] == [4, 5, 6]
        assert best == va.best_epoch(stats, "devel", metrics) and best["epoch"] == va.best_epoch(rows, "devel", metrics)["epoch"]
        assert all(abs(a["devel_loss"] - b["devel_loss"]) <= 1e-4 for a, b in zip(stats, rows))
        assert va.stats_csv(stats).startswith(b"epoch;devel_loss;devel_recall;devel_f1;devel_accuracy\n")


def test_end_to_end_on_a_corpus(tmp_path):
    """extract_features -> fit_heads -> write_checkpoint -> load_audio -> run_corpus on the corpus of tests/test_gpu_validate.py."""
    sr, max_w = 16000, 2
    lens = (32000, 64000, 96000)
    files = [(f"f{k}.wav", synth.waveforms(90 + k, 1, n)[0]) for k, n in enumerate(lens)]
    tables = [ac.afew_windows(n, lab, shift=2, min_w_len=1, max_w_len=max_w) for n, lab in zip(lens, ("Happy", "Sad", "Neutral"))]
    sd = synth.to_torch(synth.audio_state_dict(42))
    eng = Engine(0)
    try:
        eng.load_audio(sd)
        table = ac.extract_features(eng, files, tables, sr, max_w, windows_per_pass=4)
        feats = np.stack([row for name, _ in files for row in table[name]["features"]])
        targets = np.array([t for name, _ in files for t in table[name]["targets"]], dtype=np.int64)
        assert feats.shape == (6, 1024) and targets.tolist() == [4, 5, 5, 0, 0, 0]
        run = hf.HeadRun(w0=sd["feature_downsample.weight"].numpy(), b0=sd["feature_downsample.bias"].numpy(),
                         order=hf.make_order(6, 2, seed=1), weights=va.class_weights([50, 10, 20, 30, 40, 25, 5, 15]), lr=1e-3)
        run.mix_lam, run.mix_index = hf.make_mixup(6, 2, 4, 0.3, seed=1)
        x = torch.from_numpy(feats).to(eng.device)
        fit = hf.fit_heads(eng, x, targets, [run], 2, batch_size=4)
        w, b = fit.w_hist[0, -1], fit.b_hist[0, -1]
        assert float((w.cpu() - sd["feature_downsample.weight"]).abs().max()) > 1e-3
        path = hf.write_checkpoint(sd, w, b, 2, tmp_path / "epoch_2.pth")
        eng.load_audio(torch.load(path, map_location="cpu", weights_only=False))
        res = ac.run_corpus(eng, files, tables, sr, max_w, windows_per_pass=4)
        want = torch.softmax(eng.head_apply(x, w[None], b[None])[0].double(), dim=1).cpu().numpy()
        got = res.probs.cpu().numpy()
        print(f"end to end: worst |dprob| {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= PROB_GATE and np.array_equal(got.argmax(axis=1), want.argmax(axis=1))
        stats, best = va.validate_checkpoints(eng, [(2, path)], files, tables, weights=run.weights, batch_size=4, max_w_len=max_w)
        assert stats[0]["epoch"] == 2 and np.isfinite(stats[0]["devel_loss"])
    finally:
        eng.close()
