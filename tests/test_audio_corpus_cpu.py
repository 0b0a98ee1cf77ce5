"""Host side of the audio model over a corpus (avcer_amd/audio_corpus.py) against what the reference's own planners and its
majority vote returned (tests/golden/audio_corpus.npz, written by tests/golden/make_audio_corpus_golden.py).  No GPU."""
import pickle
import types

import numpy as np
import pytest

from avcer_amd import audio_corpus as ac


@pytest.fixture(scope="module")
def gold(golden):
    return golden("audio_corpus")


def _frame_cases(gold):
    return [str(n) for n in gold["frame_cases"]]


def _same_table(tab, t, f, where):
    assert len(tab) == len(f), (where, len(tab), len(f))
    assert tab.start_f.dtype == tab.end_f.dtype == tab.expr.dtype == np.int64
    assert np.array_equal(tab.start_f, f[:, 0]) and np.array_equal(tab.end_f, f[:, 1]), where
    assert np.array_equal(tab.expr, f[:, 2]), where
    assert tab.start_t.dtype == tab.end_t.dtype == np.float64
    assert np.array_equal(tab.start_t, t[:, 0]) and np.array_equal(tab.end_t, t[:, 1]), where   # equal as float64


def test_round_math_matches_the_reference_on_both_sides_of_a_half(gold):
    for name in _frame_cases(gold):
        assert ac.round_math(float(gold[f"{name}/fps"])) == int(gold[f"{name}/round_math"]), name
    assert ac.round_math(24.5) == 25 and round(24.5) == 24        # the case that tells it from Python's round
    assert ac.round_math(24.49) == 24 and ac.round_math(29.97) == 30 and ac.round_math(-2.5) == -3


def test_cexpr_windows_equal_the_reference(gold):
    seen = 0
    for name in _frame_cases(gold):
        tab = ac.cexpr_windows(gold[f"{name}/expr"], gold[f"{name}/mouth"], float(gold[f"{name}/fps"]))
        _same_table(tab, gold[f"{name}/cexpr_t"], gold[f"{name}/cexpr_f"], name)
        assert tab.kind == "cexpr" and tab.mouth_open is None
        order = np.lexsort((tab.end_f, tab.start_f))
        assert np.array_equal(order, np.arange(len(tab))), name   # sorted by (start_f, end_f), as documented
        seen += len(tab)
    assert seen > 60
    # the cases do what they are named for
    assert len(gold["dup76/cexpr_f"]) == 1 and tuple(gold["dup76/cexpr_f"][0]) == (1, 76, 3)
    assert len(gold["all_unlabelled/cexpr_f"]) == 0 and len(gold["empty/cexpr_f"]) == 0
    assert gold["short_seq/cexpr_f"][:, 0].min() == 54            # the 50-frame sequence left no window
    assert set(gold["tie_1_3/cexpr_f"][:, 2]) >= {1} and gold["tie_5_2/cexpr_f"][0, 2] == 2 and gold["tie_m2_7/cexpr_f"][0, 2] == -2


@pytest.mark.parametrize("classes", [8, 7])
def test_abaw_windows_equal_the_reference(gold, classes):
    seen = 0
    for name in _frame_cases(gold):
        if f"{name}/abaw{classes}_f" not in gold.files:
            assert name == "empty"
            assert len(ac.abaw_windows(gold[f"{name}/expr"], gold[f"{name}/mouth"], 25.0, num_classes=classes)) == 0
            continue
        fps = float(gold[f"{name}/fps"])
        tab = ac.abaw_windows(gold[f"{name}/expr"], gold[f"{name}/mouth"], fps, num_classes=classes)
        _same_table(tab, gold[f"{name}/abaw{classes}_t"], gold[f"{name}/abaw{classes}_f"], name)
        want = gold[f"{name}/abaw{classes}_mouth"]
        assert tab.mouth_open.dtype == np.int64 and tab.mouth_open.shape[0] == len(tab)
        assert np.array_equal(tab.mouth_open, want.reshape(len(tab), -1) if len(tab) else tab.mouth_open), name
        assert tab.fps == fps and tab.kind == "abaw"
        assert (np.diff(tab.start_t) > 0).all(), name               # sorted by start_t, and no two windows share a start
        seen += len(tab)
    assert seen > 50
    assert gold[f"above_classes/abaw{classes}_f"][:, 2].max() == (7 if classes == 8 else 2)   # 8, 9 (and 7 of 7 classes) were dropped
    assert len(gold["above_classes/abaw8_f"]) > len(gold["above_classes/abaw7_f"]) > 0


@pytest.mark.parametrize("classes", [8, 6])
def test_afew_windows_equal_the_reference(gold, classes):
    seen = 0
    for fn, label, dur in zip(gold["afew_files"], gold["afew_labels"], gold["afew_durations"]):
        vad = [{"start": 0, "end": int(dur)}]
        tab = ac.afew_windows(int(dur), str(label), num_classes=classes, vad_info=vad)
        _same_table(tab, gold[f"afew{classes}/{fn}/t"], gold[f"afew{classes}/{fn}/f"], str(fn))
        assert tab.kind == "afew" and tab.vad_info == vad
        seen += len(tab)
    assert seen > 10
    assert len(gold["afew6/u_max.wav/f"]) == 0 and len(gold["afew8/u_max.wav/f"]) > 0   # Surprise = 6 > 6 - 1
    assert ac.afew_label("Angry") == 1 and ac.afew_label(4) == 4
    with pytest.raises(ValueError):
        ac.afew_label("Other")


def test_window_samples_use_pythons_round():
    sr = 16000
    # sr * t lands on .5 exactly: Python's round goes to the even neighbour, round_math would go up
    for t in (1 / 256, 3 / 256, 5 / 256, 257 / 256, 1283 / 256):   # 16000 / 256 = 62.5: exact in binary
        x = sr * t
        assert x - int(x) == 0.5, t
        a, b = ac.window_samples(t, t + 4, sr, 4, "cexpr")
        assert (a, b) == (round(x), round(sr * (t + 4)))
        assert a == (int(x) if int(x) % 2 == 0 else int(x) + 1)
        assert ac.window_samples(t, t + 4, sr, 4, "afew") == (a, b)
        a2, b2 = ac.window_samples(t, t + 4, sr, 4, "abaw")
        assert (a2, b2) == (a, min(round(sr * (t + 4)), sr * (t + 4 + 4))) and isinstance(b2, int)
    assert ac.window_samples(1 / 30, 121 / 30, sr, 4, "cexpr") == (round(sr * (1 / 30)), round(sr * (121 / 30)))
    with pytest.raises(ValueError):
        ac.window_samples(0.0, 1.0, sr, 4, "meld")


@pytest.mark.parametrize("classes", [7, 8])
def test_votes_numpy_equals_the_references_majority_voting(gold, classes):
    predicts, targets = gold[f"vote{classes}/predicts"], gold[f"vote{classes}/targets"]
    files = [str(f) for f in gold[f"vote{classes}/files"]]
    # the kernel's layout: the windows of a file are neighbours; here in the order the files first appear (NOT sorted)
    names = list(dict.fromkeys(files))
    rows = np.concatenate([[i for i, f in enumerate(files) if f == name] for name in names])
    off = np.concatenate([[0], np.cumsum([files.count(name) for name in names])])
    probs, pred, file_pred, file_target, onehot = ac.votes_numpy(predicts[rows], targets[rows], off)
    assert np.array_equal(pred, np.argmax(predicts[rows], axis=1))
    order = np.argsort(names)                                     # the reference's groupby sorts the names
    assert [names[i] for i in order] == [str(f) for f in gold[f"vote{classes}/out_files"]]
    assert np.array_equal(file_target[order], gold[f"vote{classes}/out_targets"])
    assert np.array_equal(onehot[order], gold[f"vote{classes}/out_preds"])
    assert np.array_equal(np.argmax(onehot, axis=1), file_pred) and (onehot.sum(axis=1) == 1).all()
    assert probs.dtype == np.float32 and np.allclose(probs.sum(axis=1), 1, atol=1e-6)
    by_name = dict(zip([names[i] for i in order], gold[f"vote{classes}/out_preds"].argmax(axis=1)))
    assert by_name["mid.wav"] == 0 and by_name["zeta.wav"] == 5 and by_name["alpha.wav"] == classes - 1   # ties -> smallest; first maximum


def test_votes_numpy_edges():
    logits = np.asarray([[0, 1, 1], [2, 2, 2], [np.nan, 5, 1], [0, 0, 7]], dtype=np.float32)
    probs, pred, file_pred, file_target, onehot = ac.votes_numpy(logits, [-2, -2, 1, 9], [0, 0, 3, 3, 4])
    assert pred.tolist() == [1, 0, 0, 2]                          # first maximum; a NaN counts as the maximum
    assert file_pred.tolist() == [-1, 0, -1, 2] and file_target.tolist() == [-1, -2, -1, -1]   # 9 is counted nowhere
    assert onehot.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1]]
    assert np.isnan(probs[2]).all() and np.array_equal(probs[1], np.full(3, np.float32(1) / np.float32(3)))


def _stub_engine(max_tokens=256, classes=8):
    return types.SimpleNamespace(audio_max_tokens=max_tokens, audio_classes=classes)


def test_planner_input_checks():
    e, m = np.zeros(100, np.int64), np.ones(100)
    for fn in (ac.cexpr_windows, ac.abaw_windows):
        for fps in (0, -25.0, float("nan"), 0.3, None):
            with pytest.raises(ValueError):
                fn(e, m, fps)
        with pytest.raises(ValueError):
            fn(e, m[:-1], 25.0)
        for kw in ({"shift": 0}, {"shift": -1}, {"shift": 1.5}, {"min_w_len": 0}, {"max_w_len": 0}):
            with pytest.raises(ValueError):
                fn(e, m, 25.0, **kw)
    with pytest.raises(ValueError):
        ac.afew_windows(-1, "Happy")
    with pytest.raises(ValueError):
        ac.afew_windows(1000, "Happy", shift=0)


def test_corpus_plan_checks_before_any_work():
    tab = ac.afew_windows(48000, "Happy")
    wav = np.zeros(48000, np.float32)
    ok = ac.plan_corpus(_stub_engine(), [("a", wav)], [tab])
    assert ok[2].tolist() == [0, len(tab)] and ok[3].tolist() == [0] and ok[4].tolist() == [47999]
    with pytest.raises(ValueError, match="max_tokens"):           # 6 s at 16 kHz is 299 tokens
        ac.plan_corpus(_stub_engine(256), [("a", wav)], [tab], max_w_len=6)
    with pytest.raises(ValueError, match="windows_per_pass"):
        ac.plan_corpus(_stub_engine(), [("a", wav)], [tab], windows_per_pass=0)
    with pytest.raises(ValueError, match="window tables"):
        ac.plan_corpus(_stub_engine(), [("a", wav)], [tab, tab])
    with pytest.raises(ValueError, match="distinct"):
        ac.plan_corpus(_stub_engine(), [("a", wav), ("a", wav)], [tab, tab])
    with pytest.raises(ValueError, match="no files"):
        ac.plan_corpus(_stub_engine(), [], [])
    with pytest.raises(ValueError, match="more than"):            # a 4 s window against max_w_len = 2
        ac.plan_corpus(_stub_engine(), [("a", np.zeros(100000, np.float32))], [ac.afew_windows(100000, "Happy")], max_w_len=2)
    with pytest.raises(ValueError, match="targets"):              # class 7 against a 7-class model
        ac.plan_corpus(_stub_engine(classes=7), [("a", wav)], [ac.afew_windows(48000, 7)])
    big = np.broadcast_to(np.float32(0), (2 ** 30 + 1,))           # no memory behind it: only its length is read
    none = ac.afew_windows(0, "Happy")
    with pytest.raises(ValueError, match=r"2\^31 - 1"):
        ac.plan_corpus(_stub_engine(), [("a", big), ("b", big)], [none, none])


def test_windows_past_the_end_of_a_file_are_clipped():
    tab = ac.cexpr_windows(np.full(100, 3), np.ones(100), 25.0)    # frames 1 .. 100 and 51 .. 100: 1/25 s and 51/25 s to 4 s
    names, s_off, file_off, starts, ends, targets = ac.plan_corpus(_stub_engine(), [("v", np.zeros(50000, np.float32))], [tab])
    assert starts.tolist() == [640, 32640] and ends.tolist() == [50000, 50000] and targets.tolist() == [3, 3]


def test_readers_and_pickle(tmp_path):
    lab = tmp_path / "v.txt"
    lab.write_text("Neutral,Anger,Disgust,Fear,Happiness,Sadness,Surprise,Other\n3\n3\n-1\n7\n")
    assert ac.read_labels(str(lab)).tolist() == [3, 3, -1, 7]
    csv = tmp_path / "v.csv"
    csv.write_text(",frame,surface_area_mouth,mouth_open\n0,1,10.5,1.0\n1,2,0.2,0.0\n2,4,3.0,1.0\n3,9,3.0,1.0\n")
    assert ac.read_mouth_open(str(csv), 5).tolist() == [1.0, 0.0, 0.0, 1.0, 0.0]   # frame 3 missing -> 0.0, frame 9 has no label
    csv.write_text(",frame,surface_area_mouth,mouth_open\n0,1,10.5,1.0\n1,1,0.2,0.0\n")
    with pytest.raises(ValueError):
        ac.read_mouth_open(str(csv), 5)
    vad = {"a.wav": [{"start": 0, "end": 16000}]}
    p = ac.write_pickle(str(tmp_path / "sub" / "vad.pickle"), vad)
    assert ac.read_vad(p) == vad
    with open(p, "rb") as f:
        assert f.read(2) == bytes([0x80, pickle.HIGHEST_PROTOCOL])
