"""avcer_amd/head_fit.py on the CPU.

1. head_fit_numpy against the reference's train iteration in torch float64 (tests/golden/head_fit.npz, written by
   tests/golden/make_head_fit_golden.py with the reference's own SoftFocalLoss) at 1e-12 absolute, the project's figure for
   `validate`: weights, batch losses, epoch losses; both losses, with and without class weights and mixup, a short last batch, a
   single batch, a single row, a warm restart, a mixup tie at lam = 0.5 between differing labels.
2. Every ValueError of the argument checks.
3. write_checkpoint round-trips through packing's checkpoint reader, and refuses a base of another head shape.
4. make_order / make_mixup draw what the checks accept."""
import os

import numpy as np
import pytest
import torch

import head_fit_cases as cases
from avcer_amd import head_fit as hf
from avcer_amd import packing, synth

TOL = 1e-12
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_fit.npz"))


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_statement_against_the_reference_iteration(name):
    feats, targets, runs, bsz = cases.inputs(name)
    got = hf.head_fit_numpy(feats, targets, list(runs.values()), cases.EPOCHS, bsz)
    assert len(got) == len(runs)
    for r, g in zip(runs, got):
        for key, value in zip(g._fields, g):
            want = GOLD[f"{name}/{r}/{key}"]
            assert value.shape == want.shape and np.isfinite(value).all()
            assert np.abs(value - want).max() <= TOL, (name, r, key, np.abs(value - want).max())
        assert 0 < GOLD[f"{name}/{r}/f32_dev"] < 1e-4
        moved = np.abs(g.w_hist[-1] - runs[r].w0).max()
        assert moved > 1e-3, (name, r, moved)   # the run went somewhere


def test_the_tie_of_a_half_mix_takes_the_first_label():
    x = np.arange(8, dtype=np.float32).reshape(4, 2)
    y = np.array([3, 1, 2, 2])
    index = np.array([1, 0, 3, 2])
    mx, my = hf.mix_batch(x, y, 0.5, index)
    assert my.tolist() == [1, 1, 2, 2] and np.array_equal(mx, np.float32(0.5) * x + np.float32(0.5) * x[index])
    assert hf.mix_batch(x, y, 0.75, index)[1].tolist() == [3, 1, 2, 2] and hf.mix_batch(x, y, 0.25, index)[1].tolist() == [1, 3, 2, 2]
    assert hf.mix_batch(x, y, 0.0, index)[1].tolist() == [1, 3, 2, 2] and hf.mix_batch(x, y, 1.0, index)[1].tolist() == [3, 1, 2, 2]


def test_the_rate_follows_the_warm_restarts():
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=3e-3), T_0=2,
                                                                 eta_min=1e-5)
    for at in (0.0, 0.2, 1.0, 1.8, 2.0, 2.2, 3.0, 4.0, 5.4):
        sched.step(at)
        assert abs(hf.cosine_lr(3e-3, 1e-5, 2, at) - sched.get_last_lr()[0]) <= 1e-18, at


def _args(**change):
    feats, targets, runs, bsz = cases.inputs("one_batch")
    run = runs["ce_w_mix"]
    for k, v in change.items():
        if hasattr(run, k):
            setattr(run, k, v)
    return dict(feats=change.get("feats", feats), targets=change.get("targets", targets), runs=change.get("runs", [run]),
                epochs=change.get("epochs", cases.EPOCHS), batch_size=change.get("batch_size", bsz))


def _swap(a, i, j, value):
    a = np.array(a)
    a[i, j] = value
    return a


_RUN = cases.inputs("one_batch")[2]["ce_w_mix"]
BAD = {
    "feats_1d": dict(feats=np.zeros(64, np.float32)),
    "no_rows": dict(feats=np.zeros((0, 64), np.float32), targets=np.zeros(0, np.int64)),
    "features_not_64": dict(feats=np.zeros((16, 65), np.float32)),
    "features_above_1024": dict(feats=np.zeros((16, 1088), np.float32)),
    "targets_short": dict(targets=np.zeros(15, np.int64)),
    "target_negative": dict(targets=np.array([-1] + [0] * 15)),
    "target_is_c": dict(targets=np.array([8] + [0] * 15)),
    "targets_float": dict(targets=np.zeros(16)),
    "no_runs": dict(runs=[]),
    "epochs_0": dict(epochs=0),
    "batch_0": dict(batch_size=0),
    "batch_257": dict(batch_size=257),
    "kind": dict(kind="mse"),
    "weights_7": dict(weights=np.ones(7, np.float32)),
    "weights_nan": dict(weights=np.array([np.nan] + [1] * 7, np.float32)),
    "smoothing": dict(label_smoothing=1.5),
    "gamma_inf": dict(gamma=float("inf")),
    "lr_nan": dict(lr=float("nan")),
    "eta_min_inf": dict(eta_min=float("inf")),
    "eps_nan": dict(eps=float("nan")),
    "beta_nan": dict(betas=(0.9, float("nan"))),
    "beta_1": dict(betas=(1.0, 0.999)),
    "t0_0": dict(t0=0),
    "t0_float": dict(t0=2.5),
    "w0_shape": dict(w0=np.zeros((8, 128), np.float32)),
    "w0_nan": dict(w0=_swap(_RUN.w0, 0, 0, np.nan)),
    "b0_shape": dict(b0=np.zeros(7, np.float32)),
    "b0_missing": dict(b0=None),
    "order_missing": dict(order=None),
    "order_shape": dict(order=_RUN.order[:2]),
    "order_repeats": dict(order=_swap(_RUN.order, 1, 0, _RUN.order[1, 1])),
    "order_out_of_range": dict(order=_swap(_RUN.order, 2, 3, 16)),
    "order_float": dict(order=_RUN.order.astype(np.float64)),
    "lam_without_index": dict(mix_index=None),
    "index_without_lam": dict(mix_lam=None),
    "lam_above_1": dict(mix_lam=_swap(_RUN.mix_lam, 0, 0, 1.5)),
    "lam_nan": dict(mix_lam=_swap(_RUN.mix_lam, 1, 0, np.nan)),
    "lam_shape": dict(mix_lam=_RUN.mix_lam[:, :0]),
    "index_repeats": dict(mix_index=_swap(_RUN.mix_index, 0, 0, _RUN.mix_index[0, 1])),
    "index_out_of_batch": dict(mix_index=_swap(_RUN.mix_index, 0, 5, 16)),
}


@pytest.mark.parametrize("name", list(BAD))
def test_arguments_are_refused_before_any_work(name):
    with pytest.raises(ValueError):
        hf.head_fit_numpy(**_args(**BAD[name]))


def test_a_mix_index_must_stay_inside_its_batch():
    feats, targets, runs, bsz = cases.inputs("f64_c7")   # 70 rows in batches of 16: the last holds 6
    run = runs["ce_w_mix"]
    run.mix_index = np.array(run.mix_index)
    run.mix_index[0, 64] = 9   # a position of a full batch that the short one does not have
    with pytest.raises(ValueError, match="inside batch 4"):
        hf.head_fit_numpy(feats, targets, [run], cases.EPOCHS, bsz)
    with pytest.raises(ValueError, match="first_epoch"):
        hf.head_fit_numpy(*cases.inputs("one_row")[:2], list(cases.inputs("one_row")[2].values()), cases.EPOCHS, 16, first_epoch=-1)


def test_the_draws_pass_the_checks():
    order = hf.make_order(70, 3, seed=5)
    lam, index = hf.make_mixup(70, 3, 16, 0.3, seed=5)
    assert order.shape == (3, 70) and order.dtype == np.int64 and lam.shape == (3, 5) and index.shape == (3, 70)
    assert np.array_equal(order, hf.make_order(70, 3, seed=5)) and not np.array_equal(order, hf.make_order(70, 3, seed=6))
    assert not np.array_equal(order[0], order[1]) and ((lam >= 0) & (lam <= 1)).all() and len(np.unique(lam)) > 5
    assert (hf.make_mixup(70, 3, 16, 0.0, seed=5)[0] == 1).all()
    feats, targets, runs, bsz = cases.inputs("f64_c7")
    run = runs["ce"]
    run.order, run.mix_lam, run.mix_index = order, lam, index
    out, = hf.head_fit_numpy(feats, targets, [run], 3, bsz)
    assert np.isfinite(out.w_hist).all() and out.batch_loss.shape == (3, 5)
    with pytest.raises(ValueError):
        hf.make_order(0, 3, 1)
    with pytest.raises(ValueError):
        hf.make_mixup(70, 3, 16, float("nan"), 1)


def test_write_checkpoint_round_trips_through_the_checkpoint_reader(tmp_path, sd_audio):
    c, f = (int(v) for v in sd_audio["feature_downsample.weight"].shape)
    rng = np.random.default_rng(3)
    w, b = rng.standard_normal((c, f)).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    path = hf.write_checkpoint({"epoch": 1, "model_state_dict": sd_audio}, w, torch.from_numpy(b), 7, tmp_path / "sub" / "epoch_7.pth")
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert list(saved) == ["epoch", "model_state_dict"] and saved["epoch"] == 7
    sd = packing._unwrap(saved)
    assert list(sd) == list(sd_audio)
    for k in sd_audio:
        want = {"feature_downsample.weight": w, "feature_downsample.bias": b}.get(k, packing._np(sd_audio[k]))
        assert np.array_equal(packing._np(sd[k]), want), k
    base, fitted = packing.pack_audio(sd_audio), packing.pack_audio(saved)
    assert list(base) == list(fitted)
    for k in base:
        want = {"fd.w": w, "fd.b": b}.get(k, base[k])
        assert np.array_equal(fitted[k], want), k
    again = hf.write_checkpoint(path, w * 2, b, 8, tmp_path / "epoch_8.pth")   # a path as the base
    assert np.array_equal(packing._np(packing._unwrap(torch.load(again, weights_only=False))["feature_downsample.weight"]), w * 2)
    with pytest.raises(ValueError, match="shapes"):
        hf.write_checkpoint(sd_audio, w[:-1], b[:-1], 1, tmp_path / "bad.pth")
    with pytest.raises(ValueError, match="feature_downsample"):
        hf.write_checkpoint({"a.weight": torch.zeros(1)}, w, b, 1, tmp_path / "bad.pth")
    assert not (tmp_path / "bad.pth").exists()
