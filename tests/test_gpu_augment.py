"""The waveform augmentations on the device (avcer_amd/augment.py, csrc/augment.hip) and what is built on them.

1. avcer_wave_augment against augment_numpy: win in {1, 2, 63, 64, 65, 257, 4099, 64000} x n in {1, 3, 130}, the four kinds mixed in
   one call.  Kind 0: bytes untouched; kinds 1 and 3: tolerance zero; kind 2 with `noise=`: tolerance zero; kind 2 with the device's
   stream: std32 within 1 ulp of the statement's and every sample within
       (Z_BOUND + 5.77 * 2^-23) * noise_std + 2^-23 * |x + noise|
   Z_BOUND = 8e-6 is the bound on a z (about three times what 1 to 2 ulp of error in logf, sqrtf, sinpif and cospif come to at
   |z| <= 5.77); the second term is the one ulp std32 may differ by, carried through noise_std to the largest |z|; the last is the
   rounding of the product and of the sum.  NaN windows, zero windows, win == 1.
2. The z themselves, read back from windows that are zero but for one sample (x + noise is then the rounded product alone), within
   Z_BOUND of normal_stream.  Measured on MI355X: see DESIGN.md section 5 (wave_augment).
3. Two launches give equal bits; a window alone gives the bits it gives among 130; 1 + 129 gives the bits of one call.
4. run_corpus(transform=spec): bit-identical for windows_per_pass in {1, 3, 128}; its feature rows are audio_forward on
   augment(chunks, plan) of the same windows; transform=None is the call without the argument and reaches no augmentation code.
5. fit_heads with views: [1, n, F] and two equal views give the bits of [n, F]; two different views against head_fit_numpy by the
   rule of tests/test_gpu_head_fit.py; a run alone gives the bits it gives among 5.   6. Limits: AVCER_EINVAL before any launch."""
import copy

import numpy as np
import pytest
import torch

import augment_cases as aug_cases
import head_fit_cases as cases
from avcer_amd import audio_corpus as ac
from avcer_amd import augment as ag
from avcer_amd import head_fit as hf
from avcer_amd import synth
from avcer_amd._lib import AvcerError
from avcer_amd.engine import Engine

pytestmark = pytest.mark.gpu

WINS = (1, 2, 63, 64, 65, 257, 4099, 64000)
Z_BOUND = 8e-6
Z_MAX = 5.77


def _bits(a):
    a = a.detach().contiguous().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _windows(n, win, seed=0):
    """(x f32 [n, win], plan): kinds 2, 3, 0, 1, 2, .. so that n = 1 is a noise window; samples beyond +-1, +-0 and a subnormal in
    every window, zeros behind 70 % of it (the chunker's padding); among 130 a window of zeros, one holding a NaN and one whose
    samples all lie beyond +-1, all of kind 2."""
    rng = np.random.default_rng([n, win, seed])
    x = (0.4 * rng.standard_normal((n, win))).astype(np.float32)
    x[:, int(0.7 * win) + 1:] = 0.0
    if win >= 63:
        x[:, 3], x[:, 5], x[:, 6], x[:, 7], x[:, 9] = 1.75, -0.0, 0.0, np.float32(1e-41), -3.5
    kind = (np.arange(n) + 2) % 4
    if n >= 130:
        x[4], x[8, win // 2], x[12] = 0.0, np.nan, x[12] + 2.0
    plan = ag.make_plan(kind, u=rng.random(n), gain_db=rng.uniform(-20.0, 6.0, n), key=rng.integers(0, 2 ** 64, n, dtype=np.uint64))
    return x, plan


@pytest.fixture(scope="module")
def statements():
    """win, n -> (x, plan, augment_numpy(x, plan)): computed once, shared, never written to"""
    memo = {}

    def get(n, win):
        if (n, win) not in memo:
            x, plan = _windows(n, win)
            want = ag.augment_numpy(x, plan)
            for a in (x, want):
                a.setflags(write=False)
            memo[(n, win)] = (x, plan, want)
        return memo[(n, win)]

    return get


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n", [1, 3, 130])
@pytest.mark.parametrize("win", WINS)
def test_kernel_against_the_statement(engine, statements, win, n):
    x, plan, want = statements(n, win)
    dev = torch.from_numpy(x.copy()).to(engine.device)
    out, std = ag.augment(engine, dev, plan, return_std=True)
    assert out is dev
    got, std = out.cpu().numpy(), std.cpu().numpy()
    worst = 0.0
    for w in range(n):
        k = int(plan.kind[w])
        if k != ag.KIND_NOISE:
            assert np.array_equal(_bits(got[w]), _bits(want[w])), (w, k)        # kind 0: `want` is x itself
            assert np.isnan(std[w])
            continue
        s_want = ag.std32_numpy(x[w])
        if np.isnan(s_want):                                                   # win == 1, or a NaN sample
            assert np.isnan(std[w]) and np.isnan(got[w]).all() and np.isnan(want[w]).all(), w
            continue
        assert abs(int(std[w].view(np.int32)) - int(s_want.view(np.int32))) <= 1, (w, std[w], s_want)
        ns = ag.noise_std_numpy(s_want, plan.u[w], plan.min_snr, plan.max_snr)
        bound = (Z_BOUND + Z_MAX * 2.0 ** -23) * ns + 2.0 ** -23 * np.abs(want[w].astype(np.float64))
        err = np.abs(got[w].astype(np.float64) - want[w].astype(np.float64))
        assert (err <= bound).all(), (w, float((err - bound).max()))
        if ns > 0:
            worst = max(worst, float((err / bound).max()))
            assert not np.array_equal(got[w], x[w])
        else:
            assert not got[w].any()                                            # the window of zeros
    print(f"wave_augment win {win} n {n}: worst |out - statement| / bound {worst:.3f}")
    # the reference's own draw fed through: tolerance zero
    rng = np.random.default_rng([win, n])
    noise = (1e-3 * rng.standard_normal((n, win))).astype(np.float32)
    fed = ag.augment(engine, torch.from_numpy(x.copy()).to(engine.device), plan, noise=torch.from_numpy(noise).to(engine.device))
    assert np.array_equal(_bits(fed), _bits(ag.augment_numpy(x, plan, noise=noise)))


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("win", [w for w in WINS if w > 1])     # one sample: no sample is left at zero, and std is NaN
def test_the_device_draws_the_statements_normal_values(engine, win):
    """Window 0 is zero but for its last sample, window 1 but for its first: where x is 0 the output is float32(noise_std * z), so
    z = out / noise_std up to that one rounding (2^-24 * 5.77 = 3.4e-7 at most, which the bound is asked to absorb as well)."""
    x = np.zeros((2, win), np.float32)
    x[0, -1] = x[1, 0] = 1.0
    keys = np.asarray([0xFEDCBA9876543210, 3], dtype=np.uint64)
    plan = ag.make_plan([2, 2], u=[0.0, 0.0], key=keys, min_snr=0.5, max_snr=0.5)
    out, std = ag.augment(engine, torch.from_numpy(x.copy()).to(engine.device), plan, return_std=True)
    got, std = out.cpu().numpy().astype(np.float64), std.cpu().numpy()
    worst = 0.0
    for w, zero in ((0, slice(0, win - 1)), (1, slice(1, win))):
        ns = ag.noise_std_numpy(std[w], 0.0, 0.5, 0.5)
        z = got[w, zero] / ns
        want = ag.normal_stream(int(keys[w]), win)[zero].astype(np.float64)
        worst = max(worst, float(np.abs(z - want).max()))
    print(f"device z, win {win}: worst |z - statement| {worst:.3e} (bound {Z_BOUND:.1e})")
    assert worst <= Z_BOUND


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("win", [65, 4099, 64000])
def test_determinism(engine, statements, win):
    x, plan, _ = statements(130, win)
    host = torch.from_numpy(x.copy())
    a = _bits(ag.augment(engine, host.to(engine.device), plan))
    b = _bits(ag.augment(engine, host.to(engine.device), plan))
    assert np.array_equal(a, b)
    for i in (0, 1, 2, 3, 64, 129):                       # one of every kind, the first and the last
        alone = _bits(ag.augment(engine, host[i:i + 1].to(engine.device), plan.rows(i, i + 1)))
        assert np.array_equal(alone[0], a[i]), i
    dev = host.to(engine.device)
    ag.augment(engine, dev[:1], plan.rows(0, 1))          # contiguous row ranges of one buffer, as the passes of a corpus are
    ag.augment(engine, dev[1:], plan.rows(1, 130))
    assert np.array_equal(_bits(dev), a)
    empty = torch.zeros(0, win, device=engine.device)
    assert ag.augment(engine, empty, ag.make_plan(np.zeros(0, np.int32))) is empty


# ------------------------------------------------------------------------------------------------ 4
SR, MAX_W = 16000, 2     # 99 tokens; the head refuses the 49 tokens of a 1 s window


@pytest.fixture(scope="module")
def eng(engine):   # `engine`: the session's fixture skips where there is no GPU
    e = Engine(0)
    e.load_audio(synth.to_torch(synth.audio_state_dict(42)))
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus():
    """three files of 2 s, 3 s and 5 s: 1 + 2 + 3 windows of 2 s, the smallest whole number of seconds the model takes"""
    lens = (32000, 48000, 80000)
    files = [(f"f{k}.wav", synth.waveforms(30 + k, 1, n)[0]) for k, n in enumerate(lens)]
    tables = [ac.afew_windows(n, lab, shift=2, min_w_len=1, max_w_len=MAX_W) for n, lab in zip(lens, ("Happy", "Sad", "Neutral"))]
    assert [len(t) for t in tables] == [1, 2, 3]
    return files, tables


def test_run_corpus_with_a_transform(eng, corpus, monkeypatch):
    files, tables = corpus
    spec = ag.AugmentSpec(seed=5)
    plain = ac.run_corpus(eng, files, tables, SR, MAX_W, windows_per_pass=3, features=True)
    res = {p: ac.run_corpus(eng, files, tables, SR, MAX_W, windows_per_pass=p, features=True, transform=spec) for p in (1, 3, 128)}
    assert res[1].passes == (1,) * 6 and res[3].passes == (3, 3) and res[128].passes == (6,)
    for p in (1, 3):
        assert np.array_equal(_bits(res[p].logits), _bits(res[128].logits)) and np.array_equal(_bits(res[p].features), _bits(res[128].features))
    assert not np.array_equal(_bits(res[128].features), _bits(plain.features)) and torch.isfinite(res[128].logits).all()
    # the rows are audio_forward on augment(chunks, plan) of the same windows
    plan = ag.draw_plan(spec, 6)
    wav_all = torch.from_numpy(np.concatenate([w for _, w in files])).to(eng.device)
    base = np.repeat(np.cumsum([0] + [len(w) for _, w in files])[:-1], [1, 2, 3])
    chunks = eng.audio_chunks(wav_all, plain.starts + base, plain.ends + base, MAX_W * SR, "constant")
    ag.augment(eng, chunks, plan)
    logits, feats = eng.audio_forward(chunks, normalize=True, return_features=True)
    assert np.array_equal(_bits(logits), _bits(res[128].logits)) and np.array_equal(_bits(feats), _bits(res[128].features))
    table = ac.extract_features(eng, files, tables, SR, MAX_W, windows_per_pass=4, transform=spec)
    assert np.array_equal(_bits(np.stack(table["f2.wav"]["features"])), _bits(res[128].features)[3:])
    # transform=None: today's call, and no augmentation code is reached
    def never(*a, **k):
        raise AssertionError("wave_augment reached without a transform")

    monkeypatch.setattr(Engine, "wave_augment", never)
    monkeypatch.setattr(ag, "draw_plan", never)
    none = ac.run_corpus(eng, files, tables, SR, MAX_W, windows_per_pass=3, features=True, transform=None)
    assert np.array_equal(_bits(none.logits), _bits(plain.logits)) and np.array_equal(_bits(none.features), _bits(plain.features))
    assert np.array_equal(_bits(none.probs), _bits(plain.probs)) and none.passes == plain.passes


def test_augmented_views(eng, corpus):
    files, tables = corpus
    spec = ag.AugmentSpec(seed=5)
    views = hf.augmented_views(eng, files, tables, 2, spec, SR, MAX_W, windows_per_pass=4)
    assert tuple(views.shape) == (2, 6, 1024) and views.dtype == torch.float32
    for v in range(2):
        one = ac.run_corpus(eng, files, tables, SR, MAX_W, windows_per_pass=4, features=True, transform=ag.AugmentSpec(seed=5 + v))
        assert np.array_equal(_bits(views[v]), _bits(one.features))
    assert not np.array_equal(_bits(views[0]), _bits(views[1]))


# ------------------------------------------------------------------------------------------------ 5
def _fit_bits(fit):
    return [_bits(t) for t in fit[:4]]


def test_fit_heads_with_views(engine):
    feats, targets, runs, _ = cases.inputs("f64_c7", n=10, bsz=4)        # F = 64, n = 10, batches of 4, 4, 2
    targets = targets % 3
    rl = []
    for r in runs.values():                                             # C = 3: the first three rows of every head
        r = copy.copy(r)
        r.w0, r.b0, r.weights = r.w0[:3].copy(), r.b0[:3].copy(), None if r.weights is None else np.asarray(r.weights)[:3].copy()
        rl.append(r)
    rl.append(copy.copy(rl[0]))
    rl[-1].lr = 2e-3                                                     # five runs
    rng = np.random.default_rng(17)
    other = (feats + 0.05 * rng.standard_normal(feats.shape)).astype(np.float32)
    x, two = torch.from_numpy(feats).to(engine.device), torch.from_numpy(np.stack([feats, other])).to(engine.device)
    one = _fit_bits(hf.fit_heads(engine, x, targets, rl, 3, 4))
    for same in (x[None], torch.stack([x, x])):
        assert all(np.array_equal(a, b) for a, b in zip(_fit_bits(hf.fit_heads(engine, same, targets, rl, 3, 4)), one))
    fit = hf.fit_heads(engine, two, targets, rl, 3, 4)                   # view = e % 2
    got = [a.cpu().numpy() for a in fit[:4]]
    assert np.array_equal(_bits(fit.batch_loss)[:, 0], one[2][:, 0]) and not np.array_equal(_bits(fit.batch_loss)[:, 1], one[2][:, 1])
    want = hf.head_fit_numpy(np.stack([feats, other]), targets, rl, 3, 4)
    # the rule of tests/test_gpu_head_fit.py: max(4 * f32_dev of the run, the largest f32_dev of the case), f32_dev = torch's
    # float32 run of the same iteration against the float64 statement
    devs = [cases.deviation(aug_cases.torch_fit_views(np.stack([feats, other]), targets, r, [0, 1, 0], 4, torch.float32, 3), want[k])
            for k, r in enumerate(rl)]
    assert all(d > 0 for d in devs)
    for k in range(len(rl)):
        tol = max(4.0 * devs[k], max(devs))
        dev = cases.deviation([g[k] for g in got[:3]], want[k])
        epoch_dev = float(np.abs(got[3][k] - want[k].epoch_loss).max())
        print(f"head_fit views run {k}: f32_dev {devs[k]:.3e}  tolerance {tol:.3e}  kernel - statement {dev:.3e}  epoch_loss {epoch_dev:.3e}")
        assert np.isfinite(dev) and dev <= tol and epoch_dev <= 4 * tol, (k, dev, tol, epoch_dev)
    for r in rl:
        r.view = np.asarray([0, 1, 0])
    assert all(np.array_equal(a, b) for a, b in zip(_fit_bits(hf.fit_heads(engine, two, targets, rl, 3, 4)), _fit_bits(fit)))
    for k in (0, 2, 4):                                                  # a run alone gives the bits it gives among 5
        alone = _fit_bits(hf.fit_heads(engine, two, targets, [rl[k]], 3, 4))
        assert all(np.array_equal(a[0], b[k]) for a, b in zip(alone, _fit_bits(fit))), k
    rl[0].view = np.asarray([0, 2, 0])
    with pytest.raises(ValueError, match="view"):
        hf.fit_heads(engine, two, targets, rl, 3, 4)
    # the kernel's own guard: a view out of range turns its epoch, and what follows, into NaN and reads nothing
    pk = hf._pack((2, 10, 64), targets, rl[1:2], 3, 4, 1)
    bad = engine.head_fit(two, pk.targets, pk.hyper, pk.class_w, pk.w0, pk.b0, pk.order, pk.mix_lam, pk.mix_index, 3, 4,
                          view=np.asarray([[0, 2, 0]], np.int32))
    loss = bad[2].cpu().numpy()
    assert np.isfinite(loss[0, 0]).all() and np.isnan(loss[0, 1:]).all()


# ------------------------------------------------------------------------------------------------ 6
def test_limits_are_refused_before_any_launch(engine):
    x = torch.zeros(2, 64, device=engine.device)
    plan = ag.make_plan([1, 2])

    def recs(**change):
        r = plan.records()
        for k, v in change.items():
            r[k][1] = v
        return r

    for bad in (dict(recs=recs(kind=4)), dict(recs=recs(kind=-1)), dict(recs=recs(u=1.0)), dict(recs=recs(u=np.nan)),
                dict(min_snr=1.0, max_snr=0.5), dict(min_snr=np.nan), dict(max_snr=np.inf)):
        args = dict(recs=plan.records())
        args.update(bad)
        with pytest.raises(AvcerError, match="wave augment") as err:
            engine.wave_augment(x, **args)
        assert err.value.code == -1
    r = plan.records()
    r["kind"][1], r["ratio"][1] = 3, np.nan
    with pytest.raises(AvcerError, match="wave augment"):
        engine.wave_augment(x, r)
    assert not x.any()                                                   # nothing ran
    for bad in (lambda: engine.wave_augment(x, plan.records()[:1]), lambda: engine.wave_augment(x[:, ::2], plan.records()),
                lambda: engine.wave_augment(x.cpu(), plan.records()), lambda: engine.wave_augment(x.double(), plan.records()),
                lambda: engine.wave_augment(x, np.zeros(2)), lambda: engine.wave_augment(x, plan.records(), noise=x[:, :8]),
                lambda: ag.augment(engine, x, ag.make_plan([1]))):
        with pytest.raises(ValueError):
            bad()
