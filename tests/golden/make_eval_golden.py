#!/usr/bin/env python3
"""Generate tests/golden/eval_golden.npz and eval_audio_submission_{False,True}.txt by running the REFERENCE's unmodified
get_abaw_pred, get_afew_pred, get_metrics and get_pred_audio.get_c_expr_db_pred (get_pred_av.py, get_pred_video.py,
get_pred_audio.py) with pandas and sklearn on a synthetic folder of three videos.

Run in the build container only (`python tests/golden/make_eval_golden.py`), like make_golden.py, whose stubs it reuses (that file is
unchanged).  Harness-side shims, none of which touches the arithmetic:
  * `plot_conf_matrix` (a matplotlib PDF) is replaced by a recorder of the `cm` it is given; `metrics` and get_pred_audio's
    `get_metrics` are wrapped by recorders that call the original;
  * `pd.read_csv` serves the one hard-coded path (D:/work/ABAW2024/AFEW_data.csv) from the synthetic folder;
  * get_pred_audio.get_c_expr_db_pred calls get_compound_expression without its fifth argument `ce_mask` (a TypeError as the
    function stands): the module's name is bound to the same function with ce_mask=False;
  * the scripts write pickles and txt files under ./src/pred_results: the generator works in a temporary directory.

The folder (every file is stored in the archive, byte for byte, so the tests rebuild it and parse it themselves):
  ann/<video>.txt                 one label per frame under the challenge's header; -1 and 7 among them; class 0 never occurs, as a
                                  label or as any model's prediction (classes 1..6 all do: get_metrics_for_fusion needs them)
  video/static__<video>.csv       probabilities, video/dynamic__<video>.csv logits, the video models' column order
  audio/model/<video>.csv         8 logit columns + `frames`, one row per (window, frame), windows overlapping, rows not in frame order
    va  40 labelled frames; visual tables 40 rows; audio covers frames 0..33 (tail repeat of 6 .. fewer after the label filter)
    vb  25 labelled frames; visual tables 22 rows (a different deficit than the audio's); audio frames 0..9 and 14..22: group
        number != frame value behind the gap
    vc  12 labelled frames; visual tables 12 rows; audio windows written last to first (keys descending), one row all NaN
    vq  the static table one row LONGER than the dynamic one, both shorter than the labels: the static table grows by the dynamic
        table's deficit (get_pred_av.py:124-125).  Its lists differ in length, so it is run on its own and only its tables are kept.
Condition on the inputs, asserted below on the reference's own tables: in every row that reaches an argmax the two largest values
differ by more than 1e-6, so no integer output hinges on the last bits."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository root and the reference on sys.path)
from make_golden_weight_search import save_npz  # noqa: E402

VIDEO_COLS = ("Neutral", "Happiness", "Sadness", "Surprise", "Fear", "Disgust", "Anger")
AUDIO_COLS = ("Neutral", "Anger", "Disgust", "Fear", "Happiness", "Sadness", "Surprise", "Other")
HEADER = ",".join(AUDIO_COLS)
VIDEOS = {"va": (40, 40, 40), "vb": (25, 22, 22), "vc": (12, 12, 12), "vq": (20, 17, 16)}  # labels, static rows, dynamic rows
MAIN = ("va", "vb", "vc")
AFEW = (("va.mp4", "Happy"), ("vb.avi", "Sad"), ("vc.mp4", "Angry"))
W2 = (0.11, 0.26, 0.06)
MARGIN = 1e-6


def top2_gap(t):
    s = np.sort(np.asarray(t, dtype=np.float64), axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


def logits(rng, n, c, order):
    x = rng.normal(0.0, 3.0, size=(n, c))
    x[:, order.index("Neutral")] -= 12.0  # class 0 is never anyone's prediction
    return x


def write_folder(root):
    import pandas as pd

    rng = np.random.default_rng(20240304)
    os.makedirs(os.path.join(root, "ann"))
    os.makedirs(os.path.join(root, "video"))
    os.makedirs(os.path.join(root, "audio", "model"))
    for vi, (video, (n_lab, n_stat, n_dyn)) in enumerate(VIDEOS.items()):
        lab = 1 + (np.arange(n_lab) * 5 + vi) % 6
        lab[rng.choice(n_lab, 3, replace=False)] = -1
        lab[rng.choice(np.nonzero(lab > 0)[0], 2, replace=False)] = 7
        with open(os.path.join(root, "ann", video + ".txt"), "w") as f:
            f.write(HEADER + "\n" + "".join(f"{int(v)}\n" for v in lab))
        s = logits(rng, n_stat, 7, VIDEO_COLS)
        s = np.exp(s - s.max(1, keepdims=True))
        s = (s / s.sum(1, keepdims=True)).astype(np.float32)  # the files hold float32 values, as write_visual_csvs writes them
        d = logits(rng, n_dyn, 7, VIDEO_COLS).astype(np.float32)
        pd.DataFrame(s, columns=list(VIDEO_COLS)).to_csv(os.path.join(root, "video", f"static__{video}.csv"), index=False)
        pd.DataFrame(d, columns=list(VIDEO_COLS)).to_csv(os.path.join(root, "video", f"dynamic__{video}.csv"), index=False)
        # audio: windows of 8 frames every 4, each row one (window, frame) pair
        frames = {"va": list(range(34)), "vb": list(range(10)) + list(range(14, 23)), "vc": list(range(12)), "vq": list(range(15))}[video]
        windows = [[f for f in frames if w <= f < w + 8] for w in range(0, max(frames) + 1, 4)]
        if video == "vc":
            windows = windows[::-1]
        pairs = [(wi, f) for wi, win in enumerate(windows) for f in win]
        base = logits(rng, len(windows), 8, AUDIO_COLS)
        a = np.stack([base[wi] + rng.normal(0.0, 0.3, size=8) for wi, _ in pairs]).astype(np.float32).astype(np.float64)
        if video == "vc":
            a[5] = np.nan
        df = pd.DataFrame(a, columns=list(AUDIO_COLS))
        df["frames"] = [str(f).zfill(6) + ".jpg" for _, f in pairs]
        df.to_csv(os.path.join(root, "audio", "model", f"{video}.csv"), index=False)
    with open(os.path.join(root, "AFEW_data.csv"), "w") as f:
        f.write("name_video,emotion\n" + "".join(f"{n},{e}\n" for n, e in AFEW))
    # the challenge's prediction file: some frames of each video, in part behind the audio's last frame, in part not covered
    with open(os.path.join(root, "format.txt"), "w") as f:
        f.write("image_location,Fearfully_Surprised,Happily_Surprised,Sadly_Surprised,Disgustedly_Surprised,Angrily_Surprised,"
                "Sadly_Fearful,Sadly_Angry\n")
        for video, listed in (("va", list(range(3, 40, 2))), ("vb", list(range(0, 25))), ("vc", [1, 2, 3, 7, 11])):
            f.write("".join(f"{video}/{str(fr + 1).zfill(5)}.jpg\n" for fr in listed))


def main():
    mg.install_stubs()
    import pandas as pd

    captured = {"cm": [], "metrics": [], "audio": []}
    vis = sys.modules["visualization.visualize"]
    vis.plot_conf_matrix = lambda cm, **kw: captured["cm"].append(np.asarray(cm).copy())
    import data.utils as du

    original_metrics = du.metrics

    def metrics(true, pred):
        out = original_metrics(true, pred)
        captured["metrics"].append(np.array(out, dtype=np.float64))
        return out

    du.metrics = metrics
    import get_pred_audio as ga
    import get_pred_av as gav
    import get_pred_video as gv

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "data")
        write_folder(root)
        real_read_csv = pd.read_csv
        pd.read_csv = lambda p, *a, **k: real_read_csv(os.path.join(root, "AFEW_data.csv") if str(p) == "D:/work/ABAW2024/AFEW_data.csv" else p, *a, **k)
        original_get_metrics = ga.get_metrics
        ga.get_metrics = lambda trues, preds, *a: (captured["audio"].append((np.array(trues), np.array(preds))), original_get_metrics(trues, preds, *a))[1]
        compound = ga.get_compound_expression
        ga.get_compound_expression = lambda pred, com_emo, dict_weights, ce_weights_type: compound(pred, com_emo, dict_weights, ce_weights_type, False)
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            ann = os.path.join(root, "ann") + "/"
            ann_files = [v + ".txt" for v in MAIN]
            path_preds = ["video", "audio", "model"]
            rng = np.random.default_rng(7)
            w1 = rng.dirichlet(np.ones(3), size=7).T

            def take(prefix, names, lists):
                for n, l in zip(names, lists):
                    out[f"{prefix}_{n}"] = np.asarray(l, dtype=np.int32 if n == "trues" else np.float64)

            def metrics_since(prefix, n_cm, n_m):
                out[f"{prefix}_cm"] = np.stack(captured["cm"][n_cm:]).astype(np.int64)
                out[f"{prefix}_metrics"] = np.stack(captured["metrics"][n_m:])

            # audio + video
            abaw = gav.get_abaw_pred(ann, root + "/", path_preds, ann_files)
            take("av_abaw", ("stat", "dyn", "audio", "trues"), abaw)
            afew = gav.get_afew_pred(root + "/", path_preds)
            take("av_afew", ("stat", "dyn", "audio", "trues"), afew)
            quirk = gav.get_abaw_pred(ann, root + "/", path_preds, ["vq.txt"])
            take("av_quirk", ("stat", "dyn", "audio", "trues"), quirk)
            assert len(quirk[0]) != len(quirk[1]), "the quirk case must show the static table's odd extension"
            out["w1"], out["w2"] = w1, np.array(W2)
            for prefix, (ps, pd_, pa, tr) in (("av_abaw", abaw), ("av_afew", afew)):
                tabs = [np.array(ps), np.array(pd_), np.array(pa)]
                fused = sum(t * w1[i] * W2[i] for i, t in enumerate(tabs))
                assert min(top2_gap(t) for t in tabs + [fused]) > MARGIN, prefix
                n_cm, n_m = len(captured["cm"]), len(captured["metrics"])
                gav.get_metrics(tr, [np.array(ps), np.array(pd_), np.array(pa)], w1, list(W2), "X", "AV", "double")
                metrics_since(prefix, n_cm, n_m)
            # the chain into the weight search (data/utils.py:138-163) on the reference's own tables
            np.random.seed(42)
            out["chain_best"] = np.asarray(du.get_weights_prob_model(abaw[3], [abaw[0], abaw[1], abaw[2]], 200, 7), dtype=np.float64)
            # video
            vdir = os.path.join(root, "video") + "/"
            for prefix, res in (("video_abaw", gv.get_abaw_pred(ann, vdir, ann_files)), ("video_afew", gv.get_afew_pred(vdir))):
                take(prefix, ("stat", "dyn", "trues"), res)
                tabs = [np.array(res[0]), np.array(res[1])]
                fused = sum(t * w1[i] * W2[i] for i, t in enumerate(tabs))
                assert min(top2_gap(t) for t in tabs + [fused]) > MARGIN, prefix
                n_cm, n_m = len(captured["cm"]), len(captured["metrics"])
                gv.get_metrics(res[2], [np.array(res[0]), np.array(res[1])], w1[:2], list(W2[:2]), "X", "V", "double")
                metrics_since(prefix, n_cm, n_m)  # fused, static, dynamic, in this order
            # audio
            adir = os.path.join(root, "audio", "model")
            for prefix, call in (("audio_abaw", lambda: ga.get_abaw_pred(ann, adir, ann_files, "X", "model", "A")),
                                 ("audio_afew", lambda: ga.get_afew_pred(adir, "X", "model", "A"))):
                n_cm, n_m = len(captured["cm"]), len(captured["metrics"])
                call()
                trues, preds = captured["audio"][-1]
                assert top2_gap(preds) > MARGIN, prefix
                take(prefix, ("audio", "trues"), (preds, trues))
                metrics_since(prefix, n_cm, n_m)
            for ce in (False, True):
                ga.get_c_expr_db_pred(os.path.join(root, "format.txt"), adir, list(MAIN), "model", "A", ce)
                txt = os.path.join(tmp, "src/pred_results/DF_C_EXPR_DB", f"C_EXPR_DB_A_model_ce_type_{ce}.txt")
                with open(txt, "rb") as f:
                    data = f.read()
                with open(os.path.join(HERE, f"eval_audio_submission_{ce}.txt"), "wb") as f:
                    f.write(data)
        finally:
            os.chdir(cwd)
            pd.read_csv = real_read_csv
        paths = []
        for d, _, files in sorted(os.walk(root)):
            for name in sorted(files):
                rel = os.path.relpath(os.path.join(d, name), root)
                with open(os.path.join(d, name), "rb") as f:
                    out[f"file_{len(paths):03d}"] = np.frombuffer(f.read(), dtype=np.uint8)
                paths.append(rel)
        out["paths"] = np.array(paths)
    for k in sorted(out):
        if not k.startswith("file_"):
            print(k, out[k].shape, out[k].dtype)
    assert not (out["av_abaw_trues"] == 0).any() and (out["av_abaw_cm"][0][:, 0] == 0).all(), "class 0 must never occur"
    path = os.path.join(HERE, "eval_golden.npz")
    save_npz(path, out)
    print("size", os.path.getsize(path))


if __name__ == "__main__":
    main()
