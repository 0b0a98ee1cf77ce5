"""The audio model over a corpus on the device (avcer_amd/audio_corpus.py, csrc/votes.hip), synthetic audio weights.

1. run_corpus on three files of 3 s, 5 s and 9.3 s at 16 kHz -- one table of each kind, 12 windows, passes of 5 so that a pass ends
   inside a file: every window's logits and features equal, bit for bit, a one-window Engine.audio_forward call on the same cut.
   Both head kinds (ExprModelV3 and ExprModelV1).
2. avcer_window_votes against audio_corpus.votes_numpy, exact on every integer output, inside guard bands (tests/guard_band.py).
3. extract_features on the three files: the keys, the types and the pickle round trip."""
import pickle

import numpy as np
import pytest
import torch

from avcer_amd import audio_corpus as ac
from avcer_amd import synth
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine, _ptr
from guard_band import Band, check

pytestmark = pytest.mark.gpu

SR, MAX_W = 16000, 4


@pytest.fixture(scope="module")
def corpus():
    """(files, tables): 3 s as an AFEW file, 5 s as an ABAW video at 29.97 fps, 9.3 s as a C-EXPR video at 25 fps whose windows
    start every second; the last windows of the two videos are cut past the end of their files."""
    lens = (48000, 80000, 148800)
    wavs = [synth.waveforms(70 + k, 1, n)[0] for k, n in enumerate(lens)]
    rs = np.random.RandomState(5)
    mouth = np.ones(240)
    mouth[100:110] = 0                                             # 10 closed frames < 12.5: kept, one sequence
    tables = [ac.afew_windows(lens[0], "Happy", vad_info=[{"start": 1000, "end": 40000}]),
              ac.abaw_windows(rs.randint(0, 8, 150), (rs.rand(150) > 0.4).astype(float), 29.97),
              ac.cexpr_windows(np.repeat(rs.randint(0, 7, 24), 10), mouth, 25.0, shift=1)]
    assert [len(t) for t in tables] == [1, 2, 9]
    files = [("c_afew.wav", wavs[0]), ("a_abaw.txt", wavs[1]), ("b_cexpr.txt", wavs[2])]
    return files, tables


def _engine(kind):
    eng = Engine(0)
    eng.load_audio(synth.to_torch(synth.audio_state_dict(42) if kind == "v3" else synth.audio_v1_state_dict(44)))
    assert (eng.audio_head_kind == 1) == (kind == "v1")
    return eng


@pytest.fixture(scope="module", params=["v3", "v1"])
def eng(request, engine):   # `engine`: the session's fixture skips where there is no GPU
    e = _engine(request.param)
    yield e
    e.close()


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("mode", [MODE_F16X3, MODE_FP32])
def test_every_window_row_is_its_one_window_forward(eng, corpus, mode):
    files, tables = corpus
    res = ac.run_corpus(eng, files, tables, SR, MAX_W, mode=mode, windows_per_pass=5, features=True)
    n = 12
    assert res.passes == (5, 5, 2) and res.file_off.tolist() == [0, 1, 3, 12]     # a pass ends inside the third file
    assert eng.x3_fallbacks == 0                                                  # the mode asked for is the mode that ran
    width = 256 if eng.audio_head_kind == 1 else 1024
    assert tuple(res.logits.shape) == (n, eng.audio_classes) and tuple(res.features.shape) == (n, width)
    assert int((res.ends - res.starts).max()) == MAX_W * SR and int((res.ends - res.starts).min()) < MAX_W * SR
    logits, feats = _bits(res.logits), _bits(res.features)
    for f, (_, wav) in enumerate(files):
        for i in range(int(res.file_off[f]), int(res.file_off[f + 1])):
            cut = np.zeros((1, MAX_W * SR), np.float32)
            cut[0, :res.ends[i] - res.starts[i]] = wav[res.starts[i]:res.ends[i]]
            one_l, one_f = eng.audio_forward(torch.from_numpy(cut), normalize=True, mode=mode, return_features=True)
            assert np.array_equal(_bits(one_l)[0], logits[i]), (f, i)
            assert np.array_equal(_bits(one_f)[0], feats[i]), (f, i)
    assert np.isfinite(res.logits.cpu().numpy()).all()
    # the votes behind the pass are those of the statement on the same logits
    probs, pred, file_pred, file_target, onehot = ac.votes_numpy(res.logits.cpu().numpy(), res.targets, res.file_off)
    assert np.array_equal(res.pred.cpu().numpy(), pred) and np.array_equal(res.file_pred.cpu().numpy(), file_pred)
    assert np.array_equal(res.file_target.cpu().numpy(), file_target) and np.array_equal(res.file_onehot.cpu().numpy(), onehot)
    # the public call: files come back in sorted-name order
    t, p, names = ac.majority_voting(eng, res.logits, res.targets, res.file_off, names=res.names)
    assert names == ["a_abaw.txt", "b_cexpr.txt", "c_afew.wav"]
    order = [1, 2, 0]
    assert t == [int(file_target[f]) for f in order] and all(np.array_equal(a, onehot[f]) and a.dtype == np.int64 for a, f in zip(p, order))


# ----------------------------------------------------------------------------- the vote kernel
def _vote_case(name, c):
    """(logits f32 [n, c], targets i32 [n], file_off)"""
    rng = np.random.default_rng([c, sum(map(ord, name))])
    if name == "one_file":
        counts = [37]
    elif name == "seventy_files":                                   # more files than the 4 waves of a block, 18 blocks
        counts = rng.integers(1, 9, 70).tolist()
    else:                                                           # 1 window, none, 200 (a wave strides 4 times), none at the end
        counts = [1, 0, 200, 5, 0]
    n = int(sum(counts))
    logits = (rng.standard_normal((n, c)) * 3).astype(np.float32)
    ties = rng.random(n) < 0.3
    logits[ties] = np.round(logits[ties])                           # small integers: exact ties of the maximum are common
    logits[:: 7] = logits[:: 7, :1]                                 # rows of equal logits
    if name == "edge_files":
        logits[1:201:2] = np.round(logits[1:201:2] / 4)             # few distinct classes win: ties between the file's class counts
        logits[3, 2] = np.nan                                       # np.argmax: a NaN counts as the maximum; its row of probs is NaN
        logits[[201, 202, 204, 205]] = 0                            # the file of 5 windows: classes 4, 4, 0 (equal logits), 2, 2
        logits[[201, 202], 4] = logits[[204, 205], 2] = 5
    targets = rng.integers(ac.VOTES_TARGET_MIN, c, n).astype(np.int32)
    if name == "edge_files":
        targets[201:206] = [3, 3, 0, -1, -1]
    return logits, targets, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("c", [7, 8])
@pytest.mark.parametrize("name", ["one_file", "seventy_files", "edge_files"])
def test_window_votes_against_the_numpy_statement(engine, name, c):
    """Integer outputs: exact.  probs: the statement's float32 exp is numpy's, the kernel's is the device's expf, and the two may
    differ in the last place, so tolerance zero against the statement is not available; the kernel is held to a float64 softmax
    instead.  Per element, relative to the float64 value: x - max is exact or rounds once (0.5 ulp of a magnitude d <= dmax, i.e.
    d * 2^-24 relative in the exponential), expf is within 1 ulp by its specification and is given 2, in the element and in each
    term of the sum; the c - 1 additions and the quotient round once each:
        |p - p64| <= (2 * (dmax + 4) + c) * 2^-24 * p64          (eps = 2^-24 = half a float32 ulp)
    with dmax the largest max - x of the case (14 to 18 here: a bound of 44 to 51 * 2^-24).  Measured on MI355X (printed with
    -s): the worst |p - p64| / p64 of the six cases is 8.5 to 14.5 * 2^-24, in the smallest probabilities, where the rounding of
    x - max weighs most; against the numpy statement the largest absolute difference is 1.2e-7 (one ulp of a probability near 1)."""
    dev = engine.device
    logits, targets, off = _vote_case(name, c)
    n, nf = logits.shape[0], off.shape[0] - 1
    lg, tg = torch.from_numpy(logits).to(dev), torch.from_numpy(targets).to(dev)
    off_d = torch.from_numpy(off.astype(np.int32)).to(dev)

    def run(outs):
        engine._check(engine.lib.avcer_window_votes(engine.ctx, _ptr(lg), _ptr(tg), _ptr(off_d), n, c, nf, *(_ptr(o) for o in outs),
                                                    engine._stream()))

    bands = [Band("probs", (n, c), torch.float32), Band("pred", (n,), torch.int32, row_bytes=4 * c),
             Band("file_pred", (nf,), torch.int32, row_bytes=4 * c), Band("file_target", (nf,), torch.int32, row_bytes=4 * c),
             Band("file_onehot", (nf, c), torch.int32)]
    probs, pred, file_pred, file_target, onehot = (t.numpy() for t in check(run, bands, [lg, tg, off_d], device=dev))
    w_probs, w_pred, w_file_pred, w_file_target, w_onehot = ac.votes_numpy(logits, targets, off)
    assert np.array_equal(pred, w_pred) and np.array_equal(pred, np.argmax(logits, axis=1))
    assert np.array_equal(file_pred, w_file_pred) and np.array_equal(file_target, w_file_target) and np.array_equal(onehot, w_onehot)
    # the cases hold what they are for
    ok = ~np.isnan(logits).any(axis=1)
    assert ok.all() == (name != "edge_files") and np.isnan(probs[~ok]).all() and np.isfinite(probs[ok]).all()
    top = logits.max(axis=1, keepdims=True)
    assert ((logits == top).sum(axis=1) > 1).sum() > n // 10            # exact ties of the maximum, rows of equal logits among them
    counts = np.diff(off)
    if name == "edge_files":
        assert file_pred[1] == -1 and file_target[4] == -1 and not onehot[1].any() and not onehot[4].any() and counts.max() == 200
        assert file_pred[3] == 2 and file_target[3] == -1                # 2 and 4, -1 and 3 tie: the smallest wins
    hist = [np.bincount(w_pred[off[f]:off[f + 1]], minlength=c) for f in range(nf) if counts[f]]
    if name != "one_file":
        assert any((h == h.max()).sum() > 1 for h in hist)              # a tie between class counts
    p64 = _softmax64(logits[ok])
    dmax = float((top - logits)[ok].max())
    bound = (2 * (dmax + 4) + c) * 2.0 ** -24
    ratio = np.abs(probs[ok].astype(np.float64) - p64) / p64
    print(f"window votes {name} c={c}: worst |p - p64| / p64 = {ratio.max() / 2.0 ** -24:.2f} * 2^-24 (bound {bound / 2.0 ** -24:.1f}), "
          f"against the numpy statement {np.abs(probs[ok] - w_probs[ok]).max():.3e} absolute")
    assert ratio.max() <= bound, (ratio.max(), bound)
    assert np.array_equal(probs[::7][:, 0], np.full(len(probs[::7]), np.float32(1) / np.float32(c)))   # equal logits: exactly 1 / c


def test_window_votes_refuses_what_it_cannot_take(engine):
    lg = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        engine.window_votes(lg, torch.zeros(3, dtype=torch.int32), [0, 4])
    with pytest.raises(ValueError):
        engine.window_votes(lg, torch.zeros(4, dtype=torch.int32), [0, 3])
    with pytest.raises(ValueError):
        engine.window_votes(lg, torch.zeros(4, dtype=torch.int32), [0, 3, 2, 4])
    with pytest.raises(ValueError):
        ac.majority_voting(engine, lg, [0, 1, 8, 2], [0, 4])
    with pytest.raises(Exception, match="classes"):
        engine.window_votes(torch.zeros(4, 9), torch.zeros(4, dtype=torch.int32), [0, 4])
    out = engine.window_votes(torch.zeros(0, 7), torch.zeros(0, dtype=torch.int32), [0, 0, 0])   # files, no windows
    assert out[2].tolist() == [-1, -1] and out[3].tolist() == [-1, -1] and not out[4].any()


# ----------------------------------------------------------------------------- the per-file dict
def test_extract_features_keys_types_and_pickle(eng, corpus, tmp_path):
    files, tables = corpus
    d = ac.extract_features(eng, files, tables, SR, MAX_W, windows_per_pass=5)
    res = ac.run_corpus(eng, files, tables, SR, MAX_W, windows_per_pass=128, features=True)
    width = 256 if eng.audio_head_kind == 1 else 1024
    assert list(d) == [name for name, _ in files]
    common = {"targets", "predicts", "features", "frame_start", "frame_end", "timestep_start", "timestep_end"}
    assert set(d["c_afew.wav"]) == common | {"vad_info"} and set(d["a_abaw.txt"]) == common | {"fps", "mouth_open"}
    assert set(d["b_cexpr.txt"]) == common
    probs, feats = res.probs.cpu().numpy(), res.features.cpu().numpy()
    for f, ((name, _), tab) in enumerate(zip(files, tables)):
        e, a = d[name], int(res.file_off[f])
        assert all(len(v) == len(tab) for v in e.values())
        for i in range(len(tab)):
            assert type(e["targets"][i]) is np.int64 and e["targets"][i] == tab.expr[i]
            assert e["predicts"][i].dtype == np.float32 and e["predicts"][i].shape == (8,)
            assert e["features"][i].dtype == np.float32 and e["features"][i].shape == (width,)
            assert np.array_equal(e["predicts"][i], probs[a + i]) and np.array_equal(e["features"][i], feats[a + i])   # one pass or three
            assert type(e["frame_start"][i]) is int and type(e["frame_end"][i]) is int
            assert type(e["timestep_start"][i]) is float and type(e["timestep_end"][i]) is float
            assert (e["frame_start"][i], e["frame_end"][i]) == (tab.start_f[i], tab.end_f[i])
            assert (e["timestep_start"][i], e["timestep_end"][i]) == (tab.start_t[i], tab.end_t[i])
    assert all(type(v) is float and v == 29.97 for v in d["a_abaw.txt"]["fps"])
    assert all(isinstance(m, np.ndarray) and m.shape == (4,) for m in d["a_abaw.txt"]["mouth_open"])
    assert d["c_afew.wav"]["vad_info"] == ['[{"start": 1000, "end": 40000}]']
    path = ac.write_pickle(str(tmp_path / "out" / "features.pickle"), d)
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:2] == bytes([0x80, pickle.HIGHEST_PROTOCOL])
    back = pickle.loads(raw)
    assert list(back) == list(d)
    for name in d:
        assert list(back[name]) == list(d[name])
        for k, v in d[name].items():
            assert len(back[name][k]) == len(v)
            for x, y in zip(back[name][k], v):
                assert type(x) is type(y) and (np.array_equal(x, y) if isinstance(y, np.ndarray) else x == y)
