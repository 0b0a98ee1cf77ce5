"""The host side of the waveform augmentations (avcer_amd/augment.py), the MELD window planner (audio_corpus.meld_windows) and the
views of head_fit_numpy, without a GPU.

1. philox4x32: Random123's two known-answer vectors, and a second plain-integer implementation written from the paper.
2. normal_stream: mean, variance and a Kolmogorov-Smirnov test of 2^20 values under one fixed key; slices of a stream.
3. Polarity and gain against the torch expressions the reference (and torchaudio's Vol) consist of, at tolerance zero.
4. WhiteNoise: the reference's own run (tests/golden/augment.npz) reproduced at tolerance zero from its recorded draw; std32 within
   one float32 ulp of torch.std.
5. meld_windows / read_meld_labels against MeldDataset.prepare_data's recorded rows.
6. draw_plan: a window's record does not depend on the call that covers it.
7. head_fit_numpy with views.   8. Every refusal, before any work."""
import os

import numpy as np
import pytest
import torch

import augment_cases as aug_cases
import head_fit_cases as cases
from avcer_amd import audio_corpus as ac
from avcer_amd import augment as ag
from avcer_amd import head_fit as hf

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz"))
KEY = 0x0123456789ABCDEF       # the one key of the normal-stream test


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1
def _philox_plain(counter, key):
    """Philox4x32-10 with Python integers, from the paper's description: ten rounds of two 32 x 32 -> 64 bit products whose high
    halves are xored with the other counter words and the key, the key bumped by the Weyl constants between rounds."""
    c, k = [int(v) for v in counter], [int(v) for v in key]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + 0x9E3779B9) % 2 ** 32, (k[1] + 0xBB67AE85) % 2 ** 32]
        prod0, prod1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(prod1 // 2 ** 32) ^ c[1] ^ k[0], prod1 % 2 ** 32, (prod0 // 2 ** 32) ^ c[3] ^ k[1], prod0 % 2 ** 32]
    return c


KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD))]


def test_philox_known_answers_and_a_second_implementation():
    for counter, key, want in KAT:
        assert tuple(_philox_plain(counter, key)) == want
        assert tuple(int(v) for v in ag.philox4x32(counter, key)) == want
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, (50, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (50, 2), dtype=np.uint64)
    got = ag.philox4x32(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (50, 4)
    for i in range(50):
        assert [int(v) for v in got[i]] == _philox_plain(ctr[i], key[i])
    assert np.array_equal(ag.philox4x32(ctr, key[0]), ag.philox4x32(ctr, np.broadcast_to(key[0], (50, 2))))
    with pytest.raises(ValueError):
        ag.philox4x32([0, 0, 0], [0, 0])


# ------------------------------------------------------------------------------------------------ 2
def test_normal_stream_statistics():
    from scipy import stats

    n = 2 ** 20
    z = ag.normal_stream(KEY, n)
    assert z.dtype == np.float32 and z.shape == (n,) and np.isfinite(z).all() and np.abs(z).max() <= 5.78
    z64 = z.astype(np.float64)
    p = stats.kstest(z64, "norm").pvalue
    print(f"normal_stream: mean {z64.mean():.3e} (bound {5 / np.sqrt(n):.3e})  var - 1 {z64.var() - 1:.3e} (bound "
          f"{5 * np.sqrt(2 / n):.3e})  KS p {p:.3f}")
    assert abs(z64.mean()) <= 5 / np.sqrt(n)
    assert abs(z64.var() - 1.0) <= 5 * np.sqrt(2 / n)
    assert p > 1e-3


def test_normal_stream_slices_and_lanes():
    z = ag.normal_stream(KEY, 4099)
    for first, count in ((0, 1), (1, 6), (3, 2), (4, 4), (4095, 4), (64, 0)):
        assert np.array_equal(_bits(ag.normal_stream(KEY, count, first)), _bits(z[first:first + count]))
    # the statement spelled out for one counter
    a, b, c, d = (int(v) for v in ag.philox4x32([1, 0, 0, 0], [KEY & 0xFFFFFFFF, KEY >> 32]))
    r = np.sqrt(-2.0 * np.log(((a >> 8) + 1) * 2.0 ** -24))
    assert z[4] == np.float32(r * np.cos(2 * np.pi * (b >> 8) * 2.0 ** -24)) and z[5] == np.float32(r * np.sin(2 * np.pi * (b >> 8) * 2.0 ** -24))
    assert not np.array_equal(z[:64], ag.normal_stream(KEY + 1, 64))


# ------------------------------------------------------------------------------------------------ 3
def _edge_values():
    rng = np.random.default_rng(11)
    sub = np.float32(1e-41)
    special = np.asarray([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 37.0, -1e30, sub, -sub, np.nan, np.inf, -np.inf, 0.99999994, 1.0000001],
                         dtype=np.float32)
    return np.concatenate([special, (2.5 * rng.standard_normal(241)).astype(np.float32)])


def test_polarity_and_gain_equal_the_torch_expressions():
    x = _edge_values()
    gains = [-20.0, -1.0, -6.0206, -13.37, 0.0, 3.0]
    chunks = np.stack([x] * (len(gains) + 1))
    plan = ag.make_plan([ag.KIND_POLARITY] + [ag.KIND_GAIN] * len(gains), gain_db=[0.0] + gains)
    got = ag.augment_numpy(chunks, plan)
    t = torch.from_numpy(x.copy())
    assert np.array_equal(_bits(got[0]), _bits(torch.neg(t).numpy()))
    for k, g in enumerate(gains):
        ratio = 10 ** (g / 20)                       # F.gain: a Python float
        want = torch.clamp(t * ratio, -1, 1)         # Vol.forward
        assert plan.ratio32[k + 1] == np.float32(ratio)
        assert np.array_equal(_bits(got[k + 1]), _bits(want.numpy())), g
    assert np.isnan(got[1][10]) and got[1][1] == 0 and np.signbit(got[1][1]) and got[1][12] == -1.0
    assert np.array_equal(_bits(chunks[0]), _bits(x))      # the input is not changed


def test_polarity_equals_the_recorded_reference():
    for name in GOLD["noise_cases"]:
        x = GOLD[f"noise/{name}/x"]
        got = ag.augment_numpy(x[None], ag.make_plan([ag.KIND_POLARITY]))
        assert np.array_equal(_bits(got[0]), _bits(GOLD[f"polarity/{name}/out"]))


# ------------------------------------------------------------------------------------------------ 4
def _ulp_apart(a, b) -> int:
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 2 ** 31
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_white_noise_reproduces_the_reference_from_its_draw():
    lo, hi = float(GOLD["min_snr"]), float(GOLD["max_snr"])
    for name in GOLD["noise_cases"]:
        x, u = GOLD[f"noise/{name}/x"], float(GOLD[f"noise/{name}/u"])
        plan = ag.make_plan([ag.KIND_NOISE], u=[u], min_snr=lo, max_snr=hi)
        got = ag.augment_numpy(x[None], plan, noise=GOLD[f"noise/{name}/noise"][None])
        assert np.array_equal(_bits(got[0]), _bits(GOLD[f"noise/{name}/out"])), name
        std = ag.std32_numpy(x)
        apart = _ulp_apart(std, GOLD[f"noise/{name}/std"])
        print(f"white noise {name}: std32 {std!r}, torch.std {GOLD[f'noise/{name}/std']!r}, {apart} ulp apart")
        assert apart <= 1, name
        # random.uniform spelled out, from the reference's own std.  The statement is float64 (a Python float times the 0-d
        # float32 array `std` under numpy 1.x, which the reference was written for); the fixture was recorded under numpy 2, whose
        # promotion keeps that product, and with it a + (b - a) * u, in float32: three float32 roundings apart at most
        want = float(GOLD[f"noise/{name}/noise_std"])
        mine = ag.noise_std_numpy(GOLD[f"noise/{name}/std"], u, lo, hi)
        assert abs(mine - want) <= 3 * 2.0 ** -24 * abs(want) or (np.isnan(mine) and np.isnan(want)), name
    assert np.isnan(ag.std32_numpy(GOLD["noise/one/x"])) and ag.std32_numpy(GOLD["noise/zeros/x"]) == 0


def test_white_noise_from_the_generator():
    rng = np.random.default_rng(3)
    x = (0.1 * rng.standard_normal((3, 257))).astype(np.float32)
    x[1] = 0.0
    x[2, 5] = np.nan
    plan = ag.make_plan([2, 2, 2], u=[0.25, 0.5, 0.75], key=[7, 8, 9])
    got = ag.augment_numpy(x, plan)
    s = ag.noise_std_numpy(ag.std32_numpy(x[0]), 0.25, 1e-4, 5e-3)
    want = x[0] + (s * ag.normal_stream(7, 257).astype(np.float64)).astype(np.float32)
    assert np.array_equal(_bits(got[0]), _bits(want)) and not np.array_equal(got[0], x[0])
    assert not got[1].any() and np.isnan(got[2]).all()
    one = ag.augment_numpy(np.asarray([[0.25]], np.float32), ag.make_plan([2], u=[0.5], key=[1]))
    assert np.isnan(one).all()


# ------------------------------------------------------------------------------------------------ 5
def _vad():
    files = [str(f) for f in GOLD["meld/vad_files"]]
    vad = {f: [] for f in files}
    for j, a, b in GOLD["meld/vad_segments"]:
        vad[files[j]].append({"start": int(a), "end": int(b)})
    return vad


@pytest.mark.parametrize("classes", [8, 7, 6])
def test_meld_windows_against_the_reference(tmp_path, classes):
    path = tmp_path / "train_sent_emo.csv"
    path.write_text(str(GOLD["meld/csv"]))
    vad = _vad()
    labels = ac.read_meld_labels(str(path), vad)
    assert len(labels) == 9 and "dia125_utt3.wav" in vad and all(fn != "dia125_utt3.wav" and fn != "dia9_utt9.wav" for fn, _ in labels)
    with_windows = []
    for fn, emotion in labels:
        tab = ac.meld_windows(vad[fn], emotion, num_classes=classes)
        assert tab.kind == "meld"
        if len(tab):
            with_windows.append(fn)
            t, f = GOLD[f"meld{classes}/{fn}/t"], GOLD[f"meld{classes}/{fn}/f"]
            got = sorted(zip(tab.start_t, tab.end_t, tab.start_f, tab.end_f, tab.expr))
            want = sorted(zip(t[:, 0], t[:, 1], f[:, 0], f[:, 1], f[:, 2]))
            assert got == want, fn
            assert list(zip(tab.start_f, tab.end_f)) == sorted(zip(tab.start_f, tab.end_f))
    assert with_windows == [str(f) for f in GOLD[f"meld{classes}/files"]]
    if classes == 8:
        assert "dia0_utt0.wav" not in with_windows                                       # 31999 samples: shorter than min_w_len
        assert ac.meld_windows(vad["dia0_utt1.wav"], "anger").start_f.tolist() == [1000]  # exactly min_w_len
        dup = ac.meld_windows(vad["dia0_utt2.wav"], "joy")                                # the fallback to the start repeats window 0
        assert list(zip(dup.start_f, dup.end_f)) == [(0, 50000)]
        tail = ac.meld_windows(vad["dia1_utt0.wav"], "sadness")                           # 150000: the tail falls back to end - max
        assert (152500 - 64000, 152500) in list(zip(tail.start_f, tail.end_f)) and len(tail) == 5
    if classes == 6:
        assert "dia1_utt1.wav" not in with_windows                                        # surprise = 6 > 5


def test_meld_tables_are_cut_by_the_plain_rule():
    assert ac.meld_label("joy") == 4 and ac.meld_label(3) == 3
    assert ac.TABLE_CUTS["meld"] == "cexpr"
    tab = ac.meld_windows([{"start": 5, "end": 64006}], "joy")
    a, b = ac.window_samples(float(tab.start_t[0]), float(tab.end_t[0]), 16000, 4, ac.TABLE_CUTS[tab.kind])
    assert (a, b) == (round(16000 * (5 / 16000)), round(16000 * (64005 / 16000))) == (5, 64005)


# ------------------------------------------------------------------------------------------------ 6
def test_draw_plan_is_a_function_of_seed_and_window():
    spec = ag.AugmentSpec(seed=12)
    whole = ag.draw_plan(spec, 10)
    assert len(whole) == 10 and whole.kind.dtype == np.int32 and whole.key.dtype == np.uint64 and whole.ratio32.dtype == np.float32
    for i in range(10):
        one = ag.draw_plan(spec, 1, first=i)
        assert one.records().tobytes() == whole.records()[i:i + 1].tobytes() and one.gain_db[0] == whole.gain_db[i]
    assert ag.draw_plan(spec, 4, first=3).records().tobytes() == whole.rows(3, 7).records().tobytes()
    big = ag.draw_plan(spec, 300)
    assert set(big.kind.tolist()) == {1, 2, 3} and ((big.u >= 0) & (big.u < 1)).all() and len(set(big.key.tolist())) == 300
    assert (big.gain_db >= -20).all() and (big.gain_db <= -1).all()
    assert np.array_equal(big.ratio32, np.asarray([np.float32(10 ** (g / 20)) for g in big.gain_db.tolist()]))
    assert ag.draw_plan(ag.AugmentSpec(seed=13), 10).records().tobytes() != whole.records().tobytes()
    assert set(ag.draw_plan(ag.AugmentSpec(seed=1, choices=("gain",)), 20).kind.tolist()) == {3}
    assert ag.REC.itemsize == 24 and len(ag.draw_plan(spec, 0)) == 0


# ------------------------------------------------------------------------------------------------ 7
def _view_case():
    feats, targets, runs, _ = cases.inputs("f64_c7", n=10, bsz=4)
    rng = np.random.default_rng(17)
    other = (feats + 0.05 * rng.standard_normal(feats.shape)).astype(np.float32)
    return feats, other, targets, runs


def _same_runs(a, b):
    return all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_head_fit_numpy_views():
    feats, other, targets, runs = _view_case()
    rl = list(runs.values())
    one = hf.head_fit_numpy(feats, targets, rl, 3, 4)
    assert _same_runs(hf.head_fit_numpy(feats[None], targets, rl, 3, 4), one)
    assert _same_runs(hf.head_fit_numpy(np.stack([feats, feats]), targets, rl, 3, 4), one)
    two = np.stack([feats, other])
    mixed = hf.head_fit_numpy(two, targets, rl, 3, 4)           # default view: e % 2 = 0, 1, 0
    # every epoch, Adam's moments and all, against the reference's iteration in torch float64 reading view 0, 1, 0: the figure of
    # tests/test_head_fit_cpu.py for statement against torch float64
    for k, r in enumerate(rl):
        dev = cases.deviation(aug_cases.torch_fit_views(two, targets, r, [0, 1, 0], 4, torch.float64, 3), mixed[k])
        wrong = cases.deviation(aug_cases.torch_fit_views(two, targets, r, [0, 0, 0], 4, torch.float64, 3), mixed[k])
        print(f"head_fit_numpy views run {k}: against torch float64 {dev:.3e} (view 0 throughout: {wrong:.3e})")
        assert dev <= 1e-12 < wrong, (k, dev, wrong)
    for r in rl:
        r.view = np.asarray([0, 1, 0])
    assert _same_runs(hf.head_fit_numpy(two, targets, rl, 3, 4), mixed)
    for k, (name, r) in enumerate(runs.items()):
        assert np.array_equal(mixed[k].batch_loss[0], one[k].batch_loss[0]) and not np.array_equal(mixed[k].batch_loss[1], one[k].batch_loss[1])
    # epoch 1 continues from epoch 0's state on view 1.  A one-view call can be started from epoch 0's W and b but not from Adam's
    # moments and step count, which no call takes; a batch loss is computed BEFORE its step, so the first batch of epoch 1 is what a
    # one-view call from (W, b) on view 1 must reproduce (W and b pass through float32, hence 1e-6 relative):
    k, r = 0, rl[0]
    cont = hf.HeadRun(w0=mixed[k].w_hist[0].astype(np.float32), b0=mixed[k].b_hist[0].astype(np.float32), order=r.order[1:2], kind=r.kind,
                      weights=r.weights, gamma=r.gamma, lr=r.lr, eta_min=r.eta_min, t0=r.t0)
    first = hf.head_fit_numpy(other, targets, [cont], 1, 4, first_epoch=2)[0].batch_loss[0, 0]
    assert abs(first - mixed[k].batch_loss[1, 0]) <= 1e-6 * abs(first)     # w_hist rounded to float32 on its way through
    # and every epoch, moments and all: three tables under the default view e % 3 are the two tables under view = [0, 1, 0]
    for k, r in enumerate(rl):
        r.view = None
    by_hand = hf.head_fit_numpy(np.stack([feats, other, feats]), targets, rl, 3, 4)        # e % 3 = 0, 1, 2 -> feats, other, feats
    assert _same_runs(by_hand, mixed)
    for r in rl:
        r.view = np.asarray([0, 2, 0])
        with pytest.raises(ValueError, match="view"):
            hf.head_fit_numpy(two, targets, [r], 3, 4)
        r.view = np.asarray([0, 1])
        with pytest.raises(ValueError, match="view"):
            hf.head_fit_numpy(two, targets, [r], 3, 4)
        r.view = np.asarray([0, 0, 0])
        with pytest.raises(ValueError, match="view"):
            hf.head_fit_numpy(feats, targets, [r], 3, 4)
        r.view = None


# ------------------------------------------------------------------------------------------------ 8
def test_refusals_come_before_any_work():
    for bad in (dict(choices=("polarity", "sox")), dict(choices=("SoxEffect",)), dict(choices=("resample",)), dict(choices=("echo",)),
                dict(choices=()), dict(choices="noise"), dict(min_snr=1e-2, max_snr=1e-3), dict(min_gain=-1.0, max_gain=-2.0),
                dict(min_snr=float("nan")), dict(max_snr=float("inf")), dict(min_gain=float("-inf")), dict(max_gain=float("nan")),
                dict(seed=-1), dict(seed=1.5), dict(seed=True)):
        args = dict(seed=0)
        args.update(bad)
        with pytest.raises(ValueError):
            ag.AugmentSpec(**args)
    with pytest.raises(ValueError, match="libsox"):
        ag.AugmentSpec(seed=0, choices=("sox",))
    with pytest.raises(ValueError, match="Engine.resample"):
        ag.AugmentSpec(seed=0, choices=("ResampleAudio",))
    spec = ag.AugmentSpec(seed=0)
    for n, first in ((-1, 0), (2, -1), (1.5, 0), (True, 0)):
        with pytest.raises(ValueError):
            ag.draw_plan(spec, n, first)
    with pytest.raises(ValueError):
        ag.draw_plan("polarity", 3)
    x = np.zeros((2, 8), np.float32)
    for bad in (lambda: ag.augment_numpy(x, ag.make_plan([1])), lambda: ag.augment_numpy(x[0], ag.make_plan([1, 1])),
                lambda: ag.augment_numpy(x, ag.make_plan([2, 2]), noise=x[:, :4]), lambda: ag.augment_numpy(x[:, :0], ag.make_plan([1, 1])),
                lambda: ag.make_plan([4]), lambda: ag.make_plan([1], u=[1.0]), lambda: ag.make_plan([1, 1], u=[0.5]),
                lambda: ag.make_plan([3], gain_db=[np.nan]), lambda: ag.make_plan([2], min_snr=1.0, max_snr=0.5),
                lambda: ag.normal_stream(-1, 4), lambda: ag.normal_stream(2 ** 64, 4)):
        with pytest.raises(ValueError):
            bad()

    class NoEngine:          # any attribute access would be work
        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} touched")

    with pytest.raises(ValueError, match="AugmentSpec"):
        ac.run_corpus(NoEngine(), [("a", np.zeros(8, np.float32))], [None], transform="noise")
    with pytest.raises(ValueError):
        hf.augmented_views(NoEngine(), [], [], 0, spec)
    with pytest.raises(ValueError):
        hf.augmented_views(NoEngine(), [], [], 2, "noise")
    for bad in ([{"start": 0.5, "end": 40000}], [{"start": 10, "end": 5}], [{"start": -1, "end": 5}]):
        with pytest.raises(ValueError):
            ac.meld_windows(bad, "joy")
    with pytest.raises(ValueError):
        ac.meld_windows([], "happy")
    with pytest.raises(ValueError):
        ac.meld_windows([], "joy", sr=0)
