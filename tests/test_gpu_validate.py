"""Validation of audio checkpoints on the device (avcer_amd/validate.py, csrc/losses.hip).

1. avcer_window_losses against validate.losses_numpy at 1e-12 absolute -- the bound tests/test_gpu_evaluate.py holds its float64
   tables to (tests/eval_cases.py TABLE_TOL) -- on every output: row, batch, epoch, mean.
   What 1e-12 absolute means here: the statement performs the kernel's operations in the kernel's order, so the two differ only
   where the device's exp / log and numpy's differ, by an ulp of a log-sum-exp in [0, log 16] (4e-16) at the most likely.  That
   difference can move the rounding of a later result by one ulp OF THAT RESULT, and 1e-12 is one ulp at 4096 .. 8192: no
   implementation can promise it for figures above 8192.  So the inputs keep every output below that:
     weights 1 .. 400   logits of unit variance (a row loss is w * nll <= 400 * 7 = 2800) in batches of 8: the soft focal loss does
                        not divide by the weights, and batch_size * loss at 64 would be 64 * 300;
     700 rows           no weights, for the same reason (701 * loss);
     logits at +-80     no weights (a row loss is <= 161 + its smoothing share, the epoch figure batch_size * loss ~ 64 * 85 = 5400).
   Measured on MI355X (printed with -s): see the docstring of test_losses_against_the_numpy_statement.
2. Two identical launches give the same bits.
3. avcer_ccc against validate.ccc_numpy, NaN where numpy gives NaN.
4. validate_checkpoints end to end on two synthetic checkpoints, and run_corpus rows untouched by a plan handed in."""
import os

import numpy as np
import pytest
import torch

from avcer_amd import audio_corpus as ac
from avcer_amd import synth
from avcer_amd import validate as va
from avcer_amd.engine import Engine

pytestmark = pytest.mark.gpu

TOL = 1e-12   # tests/eval_cases.py TABLE_TOL


def _case(name, c, n, seed=0):
    """(logits f32 [n, c], targets [n], weights f32 [c] or None)"""
    rng = np.random.default_rng([c, n, seed, sum(map(ord, name))])
    logits = (rng.standard_normal((n, c)) * 3).astype(np.float32)
    targets = rng.integers(0, c, n)
    weights = va.class_weights(rng.integers(40, 900, c))                 # 1 .. 22: a train set's label counts
    if name == "class_missing":
        targets[targets == 3] = 4                                         # class 3 occurs in no batch
    elif name == "weights_400":
        logits = rng.standard_normal((n, c)).astype(np.float32)
        weights = np.geomspace(1, 400, c).astype(np.float32)[rng.permutation(c)]
        targets[:c] = np.arange(c)                                        # the heaviest class is a target
    elif name == "logits_80":
        logits = (np.where(rng.random((n, c)) < 0.5, -80.0, 80.0) + rng.standard_normal((n, c))).astype(np.float32)
        logits[0] = 80.0                                                  # a row of equal logits
        logits[1 % n] = [-80.0] * (c - 1) + [80.0]
        weights = None
    return logits, targets, weights


def _compare(engine, logits, targets, weights, kind, eps, gamma, bsz, worst):
    got = va.window_losses(engine, torch.from_numpy(logits).to(engine.device), targets, kind, weights, eps, gamma, bsz)
    want = va.losses_numpy(logits, targets, kind, weights, eps, gamma, bsz)
    n = logits.shape[0]
    assert tuple(got.row.shape) == (n,) and tuple(got.batch.shape) == (-(-n // bsz),) and got.row.dtype == torch.float64
    for name, g, w in (("row", got.row, want.row), ("batch", got.batch, want.batch), ("epoch", got.epoch, want.epoch), ("mean", got.mean, want.mean)):
        g, w = np.atleast_1d(g.cpu().numpy()), np.atleast_1d(w)
        assert np.isfinite(w).all() and np.abs(w).max() < 8192
        err = float(np.abs(g - w).max())
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= TOL, (name, kind, eps, gamma, bsz, n, err)
    return got, want


LOSSES = [("ce", 0.2, 0.0), ("ce", 0.0, 0.0), ("soft_focal", 0.0, 0.0), ("soft_focal", 0.0, 2.0)]


@pytest.mark.parametrize("c", [7, 8])
@pytest.mark.parametrize("kind,eps,gamma", LOSSES)
def test_losses_against_the_numpy_statement(engine, c, kind, eps, gamma):
    """Batch shapes: B = 64 with N = 1, 63, 64, 65 (a remainder of one row), 130 (three batches, the last of two rows); B = 1;
    B > N; 700 rows in one batch of 701 (a thread adds three rows).  Inputs: a class that occurs in no batch, weights over 1 .. 400,
    logits at +-80 (exp(-160) vanishes in the sum: the log-softmax is stable only max-subtracted).
    Measured on MI355X, the worst |kernel - statement| over all these cases: row 5.7e-14 (CE) and 3.4e-13 (soft focal, 8 classes,
    gamma 2: one ulp of a row loss near 2000 under a weight of 400), batch 1.4e-14, epoch and mean 0.0."""
    worst = {}
    for n in (1, 63, 64, 65, 130):
        _compare(engine, *_case("plain", c, n), kind, eps, gamma, 64, worst)
    _compare(engine, *_case("plain", c, 10), kind, eps, gamma, 1, worst)
    got, want = _compare(engine, *_case("plain", c, 5), kind, eps, gamma, 100, worst)
    assert want.epoch != pytest.approx(want.mean) and want.epoch == pytest.approx(want.mean * 100)   # one batch of 5 rows counts as 100
    logits, targets, _ = _case("plain", c, 700)
    _compare(engine, logits, targets, None, kind, eps, gamma, 701, worst)
    _compare(engine, *_case("class_missing", c, 130), kind, eps, gamma, 64, worst)
    _compare(engine, *_case("weights_400", c, 130), kind, eps, gamma, 8, worst)   # 17 batches; see the module's note on magnitudes
    logits, targets, _ = _case("logits_80", c, 130)
    got, want = _compare(engine, logits, targets, None, kind, eps, gamma, 64, worst)
    assert want.row.max() > (100 if kind == "ce" else 16)               # a target at -80 under a maximum at +80
    if kind == "ce":
        assert want.row[0] == pytest.approx(np.log(c), abs=1e-14)       # equal logits: log c whatever the smoothing
    print(f"window losses c={c} {kind} eps={eps} gamma={gamma}: worst |kernel - statement| " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_two_launches_give_the_same_bits(engine):
    logits, targets, weights = _case("plain", 8, 130)
    lg = torch.from_numpy(logits).to(engine.device)
    for kind in ("ce", "soft_focal"):
        a = va.window_losses(engine, lg, targets, kind, weights, 0.2, 2.0, 7)    # 19 batches: the last block is whichever finishes last
        b = va.window_losses(engine, lg, targets, kind, weights, 0.2, 2.0, 7)
        for x, y in zip(a, b):
            assert np.array_equal(np.atleast_1d(x.cpu().numpy()).view(np.uint64), np.atleast_1d(y.cpu().numpy()).view(np.uint64))


def test_losses_refuse_what_they_cannot_take(engine):
    lg = torch.zeros(4, 8)
    for bad in (dict(targets=[0, 1, -1, 2]), dict(targets=[0, 1, 8, 2]), dict(targets=[0, 1, 2]), dict(kind="mse"), dict(batch_size=0),
                dict(weights=np.ones(7, np.float32)), dict(label_smoothing=1.5), dict(gamma=-1.0)):
        args = dict(targets=[0, 1, 2, 3], kind="ce", weights=None, label_smoothing=0.2, gamma=0.0, batch_size=64)
        args.update(bad)
        with pytest.raises(ValueError):
            va.window_losses(engine, lg, **args)
    with pytest.raises(ValueError):
        va.window_losses(engine, torch.zeros(0, 8), [])
    with pytest.raises(Exception, match="classes"):
        engine.window_losses(torch.zeros(4, 17), torch.zeros(4, dtype=torch.int32))


@pytest.mark.parametrize("n", [1, 2, 64, 65, 10000])
def test_ccc_against_the_numpy_statement(engine, n):
    """Random series, a shifted and scaled copy (a CCC near 1), and constant series -- of 0.5, whose sums are exact in any order,
    so that the centred values are exactly 0 and the coefficient 0 / 0 = NaN on the device as in numpy; n = 1 is NaN for the
    same reason."""
    rng = np.random.default_rng(n)
    t, p = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    pairs = [(t, p), (t, 0.9 * t + 0.05), (np.full(n, 0.5), p), (t, np.full(n, 0.5)), (np.full(n, 0.5), np.full(n, 0.5))]
    for k, (a, b) in enumerate(pairs):
        got, want = float(va.ccc(engine, a, b).cpu()[0]), va.ccc_numpy(a, b)
        if n == 1 or k >= 2:
            assert np.isnan(want) and np.isnan(got), (n, k, got, want)
        else:
            assert abs(got - want) <= TOL, (n, k, got, want)
    if n >= 64:
        assert va.ccc_numpy(*pairs[1]) > 0.9
    # the valence / arousal scores read their column of the [n, t, 2] tables in place
    tt, pp = rng.uniform(-1, 1, (n, 3, 2)), rng.uniform(-1, 1, (n, 3, 2))
    dt, dp = torch.from_numpy(tt).to(engine.device), torch.from_numpy(pp).to(engine.device)
    v, a = float(va.v_score(engine, dt, dp).cpu()[0]), float(va.a_score(engine, dt, dp).cpu()[0])
    assert abs(v - va.ccc_numpy(tt[:, :, 0], pp[:, :, 0])) <= TOL and abs(a - va.ccc_numpy(tt[:, :, 1], pp[:, :, 1])) <= TOL
    assert abs(float(va.va_score(engine, dt, dp).cpu()[0]) - 0.5 * (v + a)) <= 1e-15


@pytest.mark.parametrize("c", [5, 7, 8])
def test_measures_on_the_device_are_the_statement(engine, c):
    rng = np.random.default_rng(c)
    n = 300
    probs = rng.random((n, c)).astype(np.float32)
    probs[::9] = probs[::9, :1]                                           # rows of equal values: the first class
    probs[5::11, c - 1] = 2.0                                             # the last class wins
    targets = rng.integers(0, c - 1, n)                                   # the last class is never a target: its recall is undefined
    names = [str(k) for k in range(c)]
    got = va.measures(engine, targets, torch.from_numpy(probs).to(engine.device), names)
    want = va.measures(va.NumpyEngine(), targets, probs, names)
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (targets, probs.argmax(axis=1)), 1)
    assert list(got) == list(va.MEASURES) and np.array_equal(got["conf_matrix"], cm) and np.array_equal(want["conf_matrix"], cm)
    assert cm[:, c - 1].sum() > 0 and cm[c - 1].sum() == 0 and cm[:, 0].sum() > 20
    assert all(got[m] == want[m] for m in va.SCORES)


# ----------------------------------------------------------------------------- end to end
SR, MAX_W = 16000, 2


@pytest.fixture(scope="module")
def corpus():
    """Three files of 2 s, 4 s and 6 s in windows of 2 s: 1 + 2 + 3 windows, one label per file."""
    lens = (32000, 64000, 96000)
    files = [(f"f{k}.wav", synth.waveforms(90 + k, 1, n)[0]) for k, n in enumerate(lens)]
    tables = [ac.afew_windows(n, lab, shift=2, min_w_len=1, max_w_len=MAX_W) for n, lab in zip(lens, ("Happy", "Sad", "Neutral"))]
    assert [len(t) for t in tables] == [1, 2, 3]
    return files, tables


def test_validate_checkpoints_end_to_end(engine, corpus, tmp_path):
    files, tables = corpus
    eng = Engine(0)
    try:
        sds = [synth.to_torch(synth.audio_state_dict(seed)) for seed in (42, 43)]
        weights = va.class_weights([50, 10, 20, 30, 40, 25, 5, 15])
        stats, best = va.validate_checkpoints(eng, [(3, sds[0]), (8, {"epoch": 8, "model_state_dict": sds[1]})], files, tables, weights=weights,
                                              batch_size=4, log_dir=tmp_path, save_figures=True, max_w_len=MAX_W, windows_per_pass=4)
        voted, voted_best = va.validate_checkpoints(eng, [(8, sds[1])], files, tables, loss="soft_focal", gamma=2.0, weights=weights,
                                                    batch_size=4, metrics=("f1", "recall"), group="majority", max_w_len=MAX_W)
        cols = ["epoch", "devel_loss", "devel_recall", "devel_precision", "devel_f1", "devel_accuracy"]
        assert [list(r) for r in stats] == [cols, cols] and [r["epoch"] for r in stats] == [3, 8]
        assert [list(r) for r in voted] == [["epoch", "devel_loss", "devel_f1", "devel_recall"]] and voted[0]["epoch"] == 8
        names = list(va.C_NAMES[8])
        plan = ac.plan_corpus(eng, files, tables, SR, MAX_W, 4)
        for k, sd in enumerate(sds):
            eng.load_audio(sd)
            res = ac.run_corpus(eng, files, tables, SR, MAX_W, windows_per_pass=4)
            assert res.passes == (4, 2) and res.targets.tolist() == [4, 5, 5, 0, 0, 0]
            logits, probs = res.logits.cpu().numpy(), res.probs.cpu().numpy()
            # the rows of the corpus pass are what they were: a plan handed in changes no bit, and every row is its own one-window forward
            again = ac.run_corpus(eng, files, tables, SR, MAX_W, windows_per_pass=4, plan=plan)
            assert np.array_equal(again.logits.cpu().numpy().view(np.uint32), logits.view(np.uint32))
            for f, (_, wav) in enumerate(files):
                for i in range(int(res.file_off[f]), int(res.file_off[f + 1])):
                    cut = np.zeros((1, MAX_W * SR), np.float32)
                    cut[0, :res.ends[i] - res.starts[i]] = wav[res.starts[i]:res.ends[i]]
                    one = eng.audio_forward(torch.from_numpy(cut), normalize=True)
                    assert np.array_equal(one.cpu().numpy().view(np.uint32)[0], logits.view(np.uint32)[i]), (k, i)
            want = va.losses_numpy(logits, res.targets, "ce", weights, 0.2, 0.0, 4)
            assert abs(stats[k]["devel_loss"] - want.epoch) <= TOL and want.epoch != pytest.approx(want.mean)   # 6 rows in batches of 4
            perf = va.measures(va.NumpyEngine(), res.targets, probs, names)
            assert all(stats[k][f"devel_{m}"] == perf[m] for m in va.SCORES)
            if k == 1:   # the per-file scores of the second checkpoint; the loss stays per window
                t, p, _ = ac.majority_voting(eng, res.logits, res.targets, res.file_off, names=res.names)
                perf = va.measures(va.NumpyEngine(), np.asarray(t), np.stack(p), names)
                focal = va.losses_numpy(logits, res.targets, "soft_focal", weights, 0.2, 2.0, 4)
                assert abs(voted[0]["devel_loss"] - focal.epoch) <= TOL and all(voted[0][f"devel_{m}"] == perf[m] for m in ("f1", "recall"))
        assert {k: v for k, v in best.items() if k != "figures"} == va.best_epoch(stats, "devel", va.SCORES)
        assert voted_best == va.best_epoch(voted, "devel", ("f1", "recall"))
        assert (tmp_path / "stats.csv").read_bytes() == va.stats_csv(stats)
        improving = [r for j, r in enumerate(stats) if r["devel_recall"] > max([0] + [q["devel_recall"] for q in stats[:j]])]
        assert [os.path.basename(p) for p in best["figures"]] == [f"epoch_{r['epoch']}_devel_{r['devel_recall']}.jpg" for r in improving]
        for p in best["figures"]:
            assert open(p, "rb").read(2) == b"\xff\xd8"
    finally:
        eng.close()
