"""The matrix figures on the device (avcer_amd/figures.py render, write_conf_matrices; evaluate.score(save_path=), score_models;
weight_search.write_weight_figures): host-built item lists through the existing avcer_annotate_frames and the existing JPEG
encoder, against `matrix_numpy` -- which tests/test_figures_cpu.py holds to PIL -- and `PIL.Image.save`, at tolerance zero."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import eval_cases as ec
import figure_item_cases as fi
from avcer_amd import annotate as an
from avcer_amd import evaluate as ev
from avcer_amd import figures as fg
from avcer_amd import weight_search as ws

pytestmark = pytest.mark.gpu
COMMON = ("conf7", "w3x7", "w16")  # the figures of 800 x 600


@pytest.fixture(scope="module")
def g():
    return ec.load()


@pytest.fixture(scope="module")
def tables(engine, g, tmp_path_factory):
    root = ec.write_folder(g, str(tmp_path_factory.mktemp("eval")))
    return {prefix: ev.run_job(engine, job) for prefix, (job, _) in ec.jobs(root).items()}


def test_one_confusion_matrix_is_the_statement(engine):
    values, plan, want = fi.gpu_cases()["conf7"]
    assert (plan.width, plan.height) == (800, 600)
    out = fg.render(engine, [values], [plan])
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (1, 600, 800, 3)
    np.testing.assert_array_equal(out.cpu().numpy()[0], want)


def test_a_mixed_batch_is_each_figures_statement(engine):
    """Three figures of one size in ONE call; the 16 x 16 grid at the smallest picture its plan accepts is of another size, which
    one call refuses, so it has a call of its own."""
    cases = fi.gpu_cases()
    out = fg.render(engine, [cases[k][0] for k in COMMON], [cases[k][1] for k in COMMON]).cpu().numpy()
    for i, k in enumerate(COMMON):
        np.testing.assert_array_equal(out[i], cases[k][2], err_msg=k)
    values, plan, want = cases["w16_small"]
    assert (plan.width, plan.height) != (800, 600) and fi.accepts(16, 16, "weights", plan.width - 1, plan.height) is None
    with pytest.raises(ValueError, match="one picture size"):
        fg.render(engine, [cases["conf7"][0], values], [cases["conf7"][1], plan])
    np.testing.assert_array_equal(fg.render(engine, [values], [plan]).cpu().numpy()[0], want)


def test_a_forced_split_changes_nothing(engine, monkeypatch):
    cases = fi.gpu_cases()
    values, plans = [cases[k][0] for k in COMMON], [cases[k][1] for k in COMMON]
    calls, draw = [], an.draw
    monkeypatch.setattr(an, "draw", lambda eng, frames, *a: calls.append(int(frames.shape[0])) or draw(eng, frames, *a))
    whole = fg.render(engine, values, plans)
    assert calls == [3]
    for per, want in ((1, [1, 1, 1]), (2, [2, 1])):
        del calls[:]
        assert torch.equal(fg.render(engine, values, plans, max_figures_per_call=per), whole)
        assert calls == want


@pytest.mark.parametrize("entropy", ["device", "host"])
def test_files_are_pils(engine, tmp_path, entropy):
    cms = [fi.conf_7(), np.array([[5, 0, 1], [0, 0, 0], [2, 2, 6]], dtype=np.int64)]
    labels = [None, None]
    paths = [tmp_path / "a.jpg", tmp_path / "deep" / "b.jpeg"]
    titles = ["Static video model. ABAW. UAR = 41.23%", "three"]
    plans = [fg.matrix_plan(len(cm), len(cm), "conf", title=t) for cm, t in zip(cms, titles)]
    for quality, subsampling in ((95, 2), (80, 0)):
        got = fg.write_conf_matrices(engine, cms, labels[0], paths, titles, quality=quality, subsampling=subsampling, entropy=entropy)
        assert got == [str(p) for p in paths]
        for path, cm, plan in zip(paths, cms, plans):
            assert path.read_bytes() == fi.pil_file(fg.matrix_numpy(cm, plan), quality, subsampling), (path.name, quality)
            with Image.open(path) as im:
                assert im.size == (800, 600) and np.asarray(im.convert("RGB")).shape == (600, 800, 3)


def test_weight_figures_are_the_scripts(engine, tmp_path):
    """get_weights_matrices.py: three files under its stems, the two sizes in a call each; one fitted set gives its one file."""
    from avcer_amd import fusion

    paths = ws.write_weight_figures(engine, save_dir=tmp_path)
    assert [os.path.basename(p) for p in paths] == ["weights1_video.jpg", "weights1_av_7.jpg", "weights1_av_8.jpg"]
    sets = ((fusion.WEIGHTS_V_1, fusion.WEIGHTS_V_2, (2, None)), (fusion.WEIGHTS_AV7_1, fusion.WEIGHTS_AV7_2, (3, 7)),
            (fusion.WEIGHTS_AV_1, fusion.WEIGHTS_AV_2, (3, 8)))
    for path, (w1, w2, key) in zip(paths, sets):
        stem, title, (fw, fh), x_labels = ws.WEIGHT_FIGURES[key]
        m = ws.weight_figure_matrix(w1, w2)
        plan = fg.matrix_plan(len(m), 8, "weights", 100 * fw, 100 * fh, (ws.WEIGHT_FIGURE_LABELS[0][:len(m)], ws.WEIGHT_FIGURE_LABELS[1]),
                              title, None, True, x_labels)
        with open(path, "rb") as f:
            assert f.read() == fi.pil_file(fg.matrix_numpy(m, plan)), stem
    one = ws.write_weight_figures(engine, fusion.WEIGHTS_AV7_1, fusion.WEIGHTS_AV7_2, tmp_path / "fit", audio_classes=7)
    assert one == [str(tmp_path / "fit" / "weights1_av_7.jpg")]
    with open(one[0], "rb") as a, open(paths[1], "rb") as b:
        assert a.read() == b.read()


def test_score_with_a_path_draws_its_matrix(engine, g, tables, tmp_path):
    stat, dyn, audio, trues = tables["av_abaw"]
    plain = ev.score(engine, trues, [stat, dyn, audio], g["w1"], g["w2"])
    got = ev.score(engine, trues, [stat, dyn, audio], g["w1"], g["w2"], save_path=tmp_path / "cm.jpg", title="Audio-Video fusion")
    assert list(got) == list(plain) + ["plot_conf"] and got["plot_conf"] == str(tmp_path / "cm.jpg")
    assert all(np.array_equal(got[k], plain[k]) for k in plain)
    ec.check_score(g, "av_abaw", 0, got)
    fg.write_conf_matrices(engine, [plain["cm"]], ev.EMO, [tmp_path / "same.jpg"], ["Audio-Video fusion"])
    assert (tmp_path / "cm.jpg").read_bytes() == (tmp_path / "same.jpg").read_bytes()
    plan = fg.matrix_plan(7, 7, "conf", labels=ev.EMO, title="Audio-Video fusion")
    assert (tmp_path / "cm.jpg").read_bytes() == fi.pil_file(fg.matrix_numpy(plain["cm"], plan))


def test_score_models_writes_the_references_names_in_one_draw_call(engine, g, tables, tmp_path, monkeypatch):
    """The launch profile of the engine does not count avcer_annotate_frames, so annotate.draw is counted."""
    calls, draw = [], an.draw
    monkeypatch.setattr(an, "draw", lambda eng, frames, *a: calls.append(int(frames.shape[0])) or draw(eng, frames, *a))
    stat, dyn, trues = tables["video_abaw"]
    got = ev.score_models(engine, trues, {"stat": stat, "dyn": dyn}, g["w1"][:2], g["w2"][:2], save_dir=tmp_path / "v", corpus="ABAW",
                          modality="V", weight_type="double")
    assert calls == [3]
    assert list(got) == ["fusion", "stat", "dyn"]
    assert sorted(os.listdir(tmp_path / "v")) == ["ABAW_V_dynamic_double.jpg", "ABAW_V_sd_double.jpg", "ABAW_V_static_double.jpg"]
    heads = {"fusion": "Video fusion", "stat": "Static video model", "dyn": "Dynamic video model"}
    for index, (key, m) in enumerate(got.items()):
        ec.check_score(g, "video_abaw", index, m)
        title = "{0}. {1}. UAR = {2:.2f}%".format(heads[key], "ABAW", m["uar"] * 100)  # get_pred_video.py:51,64,79
        plan = fg.matrix_plan(7, 7, "conf", labels=ev.EMO, title=title)
        with open(m["plot_conf"], "rb") as f:
            assert f.read() == fi.pil_file(fg.matrix_numpy(m["cm"], plan)), key
    del calls[:]
    stat, dyn, audio, trues = tables["av_afew"]
    av = ev.score_models(engine, trues, {"stat": stat, "dyn": dyn, "audio": audio}, g["w1"], g["w2"], save_dir=tmp_path / "av", corpus="AFEW")
    assert calls == [4] and sorted(os.listdir(tmp_path / "av")) == ["AFEW_AV_audio_single.jpg", "AFEW_AV_dynamic_single.jpg",
                                                                     "AFEW_AV_sd_single.jpg", "AFEW_AV_static_single.jpg"]
    ec.check_score(g, "av_afew", 0, av["fusion"])
    del calls[:]
    audio, trues = tables["audio_abaw"]
    a = ev.score_models(engine, trues, {"audio": audio}, save_dir=tmp_path / "a", modality="audio_mean_0.5", name_model="ExprModelV3")
    assert calls == [1] and os.listdir(tmp_path / "a") == ["ABAW_audio_mean_0.5_ExprModelV3.jpg"] and list(a) == ["audio"]
    ec.check_score(g, "audio_abaw", 0, a["audio"])
