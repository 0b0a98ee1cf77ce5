"""Host side of the dataset evaluation (avcer_amd/evaluate.py, io_formats.dataset_fusion_audio) against
tests/golden/eval_golden.npz: the reference's unmodified get_abaw_pred / get_afew_pred / get_metrics of all three scripts and
get_pred_audio.get_c_expr_db_pred, run with pandas and sklearn on a synthetic folder (tests/golden/make_eval_golden.py).

The folder is written back from the archive and parsed by the host code under test; the two kernel entries are answered by their
numpy statements (evaluate_numpy), which tests/test_gpu_evaluate.py then uses as the referee of the kernels.  Tables are compared
at 1e-12 absolute, labels and confusion matrices exactly, metrics at 1e-15 (tests/eval_cases.py)."""
import os

import numpy as np
import pytest

import eval_cases as ec
from avcer_amd import evaluate as ev
from avcer_amd import io_formats


@pytest.fixture(scope="module")
def g():
    return ec.load()


@pytest.fixture(scope="module")
def folder(g, tmp_path_factory):
    return ec.write_folder(g, str(tmp_path_factory.mktemp("eval")))


@pytest.fixture(scope="module")
def tables(folder):
    return {prefix: (ev.evaluate_numpy.job(job), names) for prefix, (job, names) in ec.jobs(folder).items()}


@pytest.mark.parametrize("prefix", ["av_abaw", "av_afew", "video_abaw", "video_afew", "audio_abaw", "audio_afew", "av_quirk"])
def test_tables_match_reference(g, tables, prefix):
    got, names = tables[prefix]
    ec.check_tables(g, prefix, names, got)


def test_quirk_static_grows_by_dynamic_deficit(g, tables):
    (stat, dyn, audio, trues), _ = tables["av_quirk"]
    assert len(stat) == len(trues) + 1 and len(dyn) == len(trues) == len(audio)


@pytest.mark.parametrize("prefix", ["av_abaw", "av_afew"])
def test_score_fusion_av(g, tables, prefix):
    (stat, dyn, audio, trues), _ = tables[prefix]
    ec.check_score(g, prefix, 0, ev.score(ev.NumpyEngine(), trues, [stat, dyn, audio], g["w1"], g["w2"]))


@pytest.mark.parametrize("prefix", ["video_abaw", "video_afew"])
def test_score_video(g, tables, prefix):
    (stat, dyn, trues), _ = tables[prefix]
    eng = ev.NumpyEngine()
    ec.check_score(g, prefix, 0, ev.score(eng, trues, [stat, dyn], g["w1"][:2], g["w2"][:2]))
    ec.check_score(g, prefix, 1, ev.score(eng, trues, [stat]))
    ec.check_score(g, prefix, 2, ev.score(eng, trues, [dyn]))


@pytest.mark.parametrize("prefix", ["audio_abaw", "audio_afew"])
def test_score_audio(g, tables, prefix):
    (audio, trues), _ = tables[prefix]
    ec.check_score(g, prefix, 0, ev.score(ev.NumpyEngine(), trues, audio))


def test_absent_class_left_out_of_macro_average(g):
    cm = g["av_abaw_cm"][0]
    assert cm[0].sum() == 0 and cm[:, 0].sum() == 0      # class 0: never a label, never predicted
    m = ev.metrics_from_cm(cm)
    recall = np.diag(cm)[1:] / cm.sum(axis=1)[1:]
    assert m["uar"] == pytest.approx(recall.mean(), abs=1e-15) and m["uar"] != pytest.approx(np.append(recall, 0.0).mean())


def test_metrics_zero_division_is_zero():
    cm = np.zeros((7, 7), dtype=np.int64)
    cm[1, 2] = 3   # class 1 never predicted (precision 0 / 0 -> 0), class 2 never a label (recall 0 / 0 -> 0)
    cm[3, 3] = 1
    m = ev.metrics_from_cm(cm)
    assert m["uar"] == pytest.approx(1 / 3) and m["precision"] == pytest.approx(1 / 3) and m["f1"] == pytest.approx(1 / 3)
    assert m["acc"] == 0.25


def test_score_refuses_labels_outside_the_matrix(tables):
    (audio, trues), _ = tables["audio_abaw"]
    bad = np.array(trues).copy()
    bad[0] = 9
    with pytest.raises(ValueError, match="outside 0..6"):
        ev.score(ev.NumpyEngine(), bad, audio)


def test_group_number_is_not_frame_value(folder):
    """vb's audio has no frames 10..13: a kept position p >= 10 is the group of frame p + 4."""
    job = ev.abaw_job(os.path.join(folder, "ann"), folder, ec.PATH_PREDS, ["vb.txt"], "audio")
    t = job.tables[0]
    groups = ev._group_means(t.rows[:, :7], t.keys)
    uniq = np.unique(t.keys)
    out = ev.evaluate_numpy.job(job)[0]
    j = int(np.nonzero((job.need >= 10) & (job.need < len(uniq)))[0][0])
    p = int(job.need[j])
    assert uniq[p] == p + 4
    assert np.array_equal(out[j], ev._softmax(groups[p:p + 1])[0])


@pytest.mark.parametrize("ce_weights_type", [False, True])
def test_dataset_fusion_audio_file(folder, tmp_path, ce_weights_type):
    locs, pred, txt = io_formats.dataset_fusion_audio(ev.NumpyEngine(), os.path.join(folder, "format.txt"), os.path.join(folder, "audio", "model"),
                                                      list(ec.MAIN), "model", "A", ce_weights_type, save_path=str(tmp_path))
    assert os.path.basename(txt) == f"C_EXPR_DB_A_model_ce_type_{ce_weights_type}.txt"
    with open(txt, "rb") as f, open(os.path.join(ec.GOLDEN, f"eval_audio_submission_{ce_weights_type}.txt"), "rb") as w:
        assert f.read() == w.read()
    assert len(locs) == len(pred)
