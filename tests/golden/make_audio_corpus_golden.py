#!/usr/bin/env python
"""Generate tests/golden/audio_corpus.npz by running the REFERENCE's own window planners and its majority vote (imported from
/root/reference/src/audio) on small synthetic label and mouth-open arrays; only the inputs and what the reference returned are kept.

Run in the build container only (`python tests/golden/make_audio_corpus_golden.py`, needs pandas); /root/reference does not exist
anywhere else, and no test imports this file.

What is called, unmodified and unbound, on a stub object that carries only the attributes the method reads:
  CExprDataset.parse_features      src/audio/data/c_expr_dataset.py:72-179
  AbawFEDataset.parse_features     src/audio/data/abaw_fe_dataset.py:82-202
  AfewFEDataset.prepare_data       src/audio/data/afew_fe_dataset.py:94-170, over a temporary folder tree of empty files whose durations
                                   the stand-in `torchaudio.info` below reports
  common_utils.majority_voting     src/audio/utils/common_utils.py:74-108
The dataset modules import cv2, torchaudio, torchvision, transformers and a `config` module at their top; none of the four methods
uses them (torchaudio.info apart), and only some are installed here, so empty stand-in modules are put into sys.modules first.

The C-EXPR planner returns its windows in the order of a Python set; they are stored sorted by (start_f, end_f), which is the
order avcer_amd.audio_corpus.cexpr_windows documents.

Cases (the names are the npz key prefixes):
  frame rates 25, 30, 29.97, 24.5 and 24.49 (round_math on both sides of .5 -- Python's round sends 24.5 to 24);
  a sequence shorter than min_w_len, one between min_w_len and max_w_len, a tail shorter than min_w_len, the 76-frame duplicate
  of the reference's own comment, gaps in lab_id (from expr == -1 rows and from dropped mouth-closed runs), mouth-closed runs one
  frame under and exactly at the threshold, labels above num_classes - 1 (ABAW, 8 and 7 classes), two-way ties of the window label
  (between 1 and 3, between 5 and 2 inserted in that order, between -2 and 7).
  Voting: a two-way tie of predictions and one of targets, a file with one window, names given out of order, 7 and 8 classes."""
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REF_AUDIO = "/root/reference/src/audio"

DURATIONS = {}  # wav base name -> samples, what the stand-in torchaudio.info reports


def _stand_ins():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    module("cv2")
    module("torchaudio", info=lambda path: types.SimpleNamespace(num_frames=DURATIONS[os.path.basename(path)]))
    tv = module("torchvision")
    tv.transforms = module("torchvision.transforms")
    tv.transforms.transforms = module("torchvision.transforms.transforms", Compose=object)
    module("transformers", Wav2Vec2Processor=object)
    module("config", c_config={}, afew_config={})
    sys.path.insert(0, REF_AUDIO)


def frame_cases():
    """name -> (fps, expr int64 [n], mouth_open float64 [n])"""
    rs = np.random.RandomState(20240302)
    cases = {}

    def runs(*pairs):
        return np.concatenate([np.full(k, v, dtype=np.int64) for v, k in pairs])

    for tag, fps in (("fps25", 25.0), ("fps30", 30.0), ("fps2997", 29.97), ("fps245", 24.5), ("fps2449", 24.49)):
        n = 410
        expr = np.repeat(rs.randint(0, 8, size=n // 10 + 1), 10)[:n].astype(np.int64)
        cases[tag] = (fps, expr, np.ones(n))
    # 30 fps: min 60, max 120, shift 60, threshold 15
    cases["short_seq"] = (30.0, runs((2, 50), (-1, 3), (4, 200)), np.ones(253))            # 50 < 60 frames, then a long one
    cases["mid_seq"] = (30.0, runs((1, 90), (-1, 2), (3, 100)), np.ones(192))               # 90 and 100: between min and max
    cases["short_tail"] = (30.0, runs((0, 100), (6, 100), (5, 30)), np.ones(230))           # tail of 50 < 60 behind seg 180
    cases["dup76"] = (30.0, runs((3, 76)), np.ones(76))                                      # the reference's comment
    cases["all_unlabelled"] = (30.0, runs((-1, 150)), np.ones(150))
    cases["no_labels_minus2"] = (25.0, runs((-2, 260)), np.ones(260))                        # a corpus without label files
    mouth = np.ones(400)
    mouth[100:114] = 0   # 14 closed frames: under the threshold of 15, kept
    mouth[250:265] = 0   # 15: at the threshold, dropped -> a gap in lab_id
    cases["mouth_runs30"] = (30.0, runs((2, 200), (5, 200)), mouth)
    mouth = np.ones(330)
    mouth[60:72] = 0     # 12 < 12.5, kept
    mouth[200:213] = 0   # 13 >= 12.5, dropped
    mouth[300:330] = 0   # a closed tail
    cases["mouth_runs25"] = (25.0, runs((1, 165), (4, 165)), mouth)
    mouth = (rs.rand(500) > 0.3).astype(np.float64)
    expr = np.repeat(rs.randint(-1, 8, size=50), 10).astype(np.int64)
    cases["random_mouth"] = (30.0, expr, mouth)
    mouth = np.repeat((rs.rand(60) > 0.35).astype(np.float64), 10)
    cases["random_runs2997"] = (29.97, np.repeat(rs.randint(-1, 8, size=40), 15).astype(np.int64), mouth)
    cases["tie_1_3"] = (30.0, runs((3, 60), (1, 60), (3, 30), (1, 30)), np.ones(180))
    cases["tie_5_2"] = (30.0, runs((5, 60), (2, 60)), np.ones(120))
    cases["tie_m2_7"] = (25.0, runs((7, 50), (-2, 50)), np.ones(100))
    cases["above_classes"] = (30.0, runs((8, 130), (7, 130), (2, 100), (9, 60)), np.ones(420))
    cases["single_frame"] = (25.0, runs((4, 1)), np.ones(1))
    cases["empty"] = (25.0, np.zeros(0, np.int64), np.zeros(0))
    return cases


def frame_df(expr, mouth):
    df = pd.DataFrame({"expr": expr})
    df["lab_id"] = df.index + 1
    df["mouth_open"] = mouth
    return df


def timings_arrays(timings, sort_cexpr):
    if sort_cexpr:
        timings = sorted(timings, key=lambda d: (d["start_f"], d["end_f"]))
    t = np.asarray([[d["start_t"], d["end_t"]] for d in timings], dtype=np.float64).reshape(-1, 2)
    f = np.asarray([[d["start_f"], d["end_f"], int(d["expr"])] for d in timings], dtype=np.int64).reshape(-1, 3)
    return t, f


def main():
    _stand_ins()
    from data.abaw_fe_dataset import AbawFEDataset
    from data.afew_fe_dataset import AfewFEDataset
    from data.c_expr_dataset import CExprDataset
    from utils.common_utils import majority_voting, round_math

    out = {}
    names = []
    for name, (fps, expr, mouth) in frame_cases().items():
        names.append(name)
        out[f"{name}/fps"] = np.float64(fps)
        out[f"{name}/round_math"] = np.int64(round_math(fps))
        out[f"{name}/expr"] = expr
        out[f"{name}/mouth"] = mouth
        stub = types.SimpleNamespace(shift=2, min_w_len=2, max_w_len=4, threshold=0.5)
        timings, labels = CExprDataset.parse_features(stub, frame_df(expr, mouth), name + ".txt", fps)
        assert [t["expr"] for t in timings] == labels
        out[f"{name}/cexpr_t"], out[f"{name}/cexpr_f"] = timings_arrays(timings, True)
        for classes in (8, 7):
            if len(expr) == 0:
                continue  # no frame, no window: nothing to record (the C-EXPR record above states the empty result)
            stub = types.SimpleNamespace(shift=2, min_w_len=2, max_w_len=4, new_fps=5, num_classes=classes)
            timings, labels = AbawFEDataset.parse_features(stub, frame_df(expr, mouth), name + ".txt", fps)
            assert all(t["fps"] == fps for t in timings)
            out[f"{name}/abaw{classes}_t"], out[f"{name}/abaw{classes}_f"] = timings_arrays(timings, False)
            out[f"{name}/abaw{classes}_mouth"] = np.asarray([t["mouth_open"] for t in timings], dtype=np.int64).reshape(len(timings), -1)
    out["frame_cases"] = np.asarray(names)

    # ---- AFEW: durations in samples at 16 kHz
    afew = {"Happy": {"h_short.wav": 20000, "h_mid.wav": 50000, "h_exact.wav": 96000, "h_long.wav": 148800},
            "Sad": {"s_one.wav": 1, "s_tail.wav": 100001}, "Surprise": {"u_min.wav": 32001, "u_max.wav": 64001}}
    a_names, a_rows = [], {}
    for classes in (8, 6):
        with tempfile.TemporaryDirectory() as root:
            vad = {}
            for label, files in afew.items():
                os.makedirs(os.path.join(root, "wavs", label))
                for fn, dur in files.items():
                    open(os.path.join(root, "wavs", label, fn), "wb").close()
                    DURATIONS[fn] = dur
                    vad[fn] = [{"start": 0, "end": dur}]
            with open(os.path.join(root, "vad.pickle"), "wb") as f:
                pickle.dump(vad, f)
            stub = types.SimpleNamespace(shift=2, min_w_len=2, max_w_len=4, sr=16000, num_classes=classes, meta=[], expr_labels=[],
                                         audio_root=os.path.join(root, "wavs"), vad_file_path=os.path.join(root, "vad.pickle"))
            stub.afew_to_abaw_labels = types.MethodType(AfewFEDataset.afew_to_abaw_labels, stub)
            AfewFEDataset.prepare_data(stub)
            for label, files in afew.items():
                for fn, dur in files.items():
                    mine = [d for d in stub.meta if os.path.basename(d["wav_filename"]) == fn]  # in the dataset's order
                    assert all(d["vad_info"] == vad[fn] for d in mine)
                    key = f"afew{classes}/{fn}"
                    out[key + "/t"], out[key + "/f"] = timings_arrays(mine, False)
                    if classes == 8:
                        a_names.append(fn)
                        a_rows[fn] = (label, dur)
    out["afew_files"] = np.asarray(a_names)
    out["afew_labels"] = np.asarray([a_rows[fn][0] for fn in a_names])
    out["afew_durations"] = np.asarray([a_rows[fn][1] for fn in a_names], dtype=np.int64)

    # ---- majority voting
    rs = np.random.RandomState(7)
    for classes in (7, 8):
        files = ["zeta.wav"] * 6 + ["alpha.wav"] * 1 + ["mid.wav"] * 4 + ["beta.wav"] * 9
        n = len(files)
        order = rs.permutation(n)  # the windows of a file need not be neighbours in the reference's lists
        predicts = rs.rand(n, classes).astype(np.float32)
        predicts /= predicts.sum(axis=1, keepdims=True)
        want = np.asarray([5, 5, 5, 2, 2, 2] + [classes - 1] + [0, 3, 3, 0] + [1] * 4 + [4] * 3 + [6, 0], dtype=np.int64)
        predicts[np.arange(n), want] = 2.0  # zeta: 5 and 2 tie -> 2; mid: 0 and 3 tie -> 0
        predicts[3, 1] = 2.0                # window 3: classes 1 and 2 both hold the maximum -> the first, 1; zeta's vote becomes 5
        targets = np.asarray([3, 1, 3, 1, 0, 0] + [6] + [2, 2, 5, 5] + [classes - 1] * 9, dtype=np.int64)  # zeta: 0, 1, 3 tie -> 0
        files = [files[i] for i in order]
        predicts, targets = predicts[order], targets[order]
        info = [{"a_filename": files[a:a + 8]} for a in range(0, n, 8)]  # batches of 8, as a dataloader collates them
        t, p, fn = majority_voting(list(targets), predicts, info)
        out[f"vote{classes}/predicts"] = predicts
        out[f"vote{classes}/targets"] = targets
        out[f"vote{classes}/files"] = np.asarray(files)
        out[f"vote{classes}/out_targets"] = np.asarray(t, dtype=np.int64)
        out[f"vote{classes}/out_preds"] = np.stack(p).astype(np.int64)
        out[f"vote{classes}/out_files"] = np.asarray(fn)
    path = os.path.join(HERE, "audio_corpus.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
