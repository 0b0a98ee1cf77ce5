"""video_corpus.corpus_plan / list_corpus on hand-made folder trees of empty files: the present masks are read_face_dir's, every
folder's ClipPlan is plan_clip's, the static passes are the cuts of the concatenated tile list, and every refusal is raised with its
message.  No GPU, no decode: the files are never opened."""
import os

import numpy as np
import pytest

from avcer_amd import video_corpus as vc
from avcer_amd.video_corpus import FaceFolder, corpus_plan, list_corpus
from avcer_amd.video_pipeline import plan_clip, read_face_dir

# name -> (file numbers, total_frames, fps)
TREES = {"seven": (range(7), 7, 25), "lone": ([3], 8, 25), "gaps": ([0, 1, 5, 6, 11], 12, 30)}


def make(root, name, numbers, track="00", extra=()):
    folder = os.path.join(str(root), name, track)
    os.makedirs(folder, exist_ok=True)
    for i in numbers:
        open(os.path.join(folder, str(i).zfill(6) + ".jpg"), "wb").close()
    for other in extra:
        open(os.path.join(folder, other), "wb").close()
    return os.path.join(str(root), name)


@pytest.fixture()
def corpus(tmp_path):
    out = []
    for name, (numbers, total, fps) in TREES.items():
        # files at and past total_frames, and names the rule never asks for, are not tiles
        extra = ("12.jpg", "000001.png", "notes.txt") if name == "gaps" else ()
        path = make(tmp_path, name, list(numbers) + ([12, 40] if name == "gaps" else []), extra=extra)
        out.append(FaceFolder(name, path, fps, total))
    return out


def mask_of(folder):
    """read_face_dir's mask, by read_face_dir's lines over the folder's listing (the files are empty: nothing can be decoded)."""
    names = set(os.listdir(os.path.join(folder.path, folder.track)))
    return np.array([str(i).zfill(6) + ".jpg" in names for i in range(folder.total_frames)], dtype=bool)


def test_read_face_dirs_own_mask_on_a_folder_it_can_read(tmp_path):
    """The rule mask_of restates is read_face_dir's: checked on a folder of real files."""
    from PIL import Image

    folder = os.path.join(str(tmp_path), "real", "00")
    os.makedirs(folder)
    for i in (1, 2, 6):
        Image.fromarray(np.full((9, 7, 3), 40 * i, dtype=np.uint8)).save(os.path.join(folder, str(i).zfill(6) + ".jpg"))
    f = FaceFolder("real", os.path.join(str(tmp_path), "real"), 25, 5)
    want = read_face_dir(f.path, 5)[1]
    assert want.tolist() == [False, True, True, False, False]
    np.testing.assert_array_equal(mask_of(f), want)
    np.testing.assert_array_equal(corpus_plan([f]).presents[0], want)


def test_present_masks_are_read_face_dirs(corpus):
    plan = corpus_plan(corpus, 1000)
    assert plan.ok == [0, 1, 2] and plan.errors == {}
    for f, got in zip(corpus, plan.presents):
        np.testing.assert_array_equal(got, mask_of(f))
    assert [int(p.sum()) for p in plan.presents] == [7, 1, 5]
    assert plan.presents[2].tolist() == [i in (0, 1, 5, 6, 11) for i in range(12)]
    assert plan.frame_off.tolist() == [0, 7, 15, 27]


def test_clip_plans_are_plan_clips(corpus):
    plan = corpus_plan(corpus, 1000)
    f_off, w_off = plan.host[3], plan.host[4]
    assert f_off.tolist() == [0, 7, 8, 13]
    for k, f in enumerate(corpus):
        want = plan_clip(mask_of(f), f.fps, int(f_off[k]), int(w_off[k]))
        got = plan.clip(k)
        assert got.static_src == want.static_src and got.dyn_src == want.dyn_src and got.windows == want.windows
    # fps 25 steps by 5, fps 30 by 6: frames 0 and 5 of `seven`, none of `lone` (frame 3), frames 0 and 6 of `gaps`
    assert w_off.tolist() == [0, 2, 2, 4]
    # `lone` never starts a window, so nothing is held behind its one crop (get_prob_video.py:175-178): zero rows, its own row 7 once
    assert plan.clip(1).dyn_src == [-1] * 8 and plan.clip(1).static_src == [-1] * 3 + [7] + [-1] * 4


@pytest.mark.parametrize("per", [1, 5, 1000])
def test_pass_cuts_are_those_of_the_concatenated_list(corpus, per):
    plan = corpus_plan(corpus, per)
    tiles = [os.path.join(f.path, "00", str(i).zfill(6) + ".jpg") for f in corpus for i in np.flatnonzero(mask_of(f))]
    assert plan.files == tiles and plan.n_tiles == 13
    cuts = [tiles[a:a + per] for a in range(0, len(tiles), per)]
    assert plan.passes == [len(c) for c in cuts] == {1: [1] * 13, 5: [5, 5, 3], 1000: [13]}[per]
    at = 0
    for n, want in zip(plan.passes, cuts):
        assert plan.files[at:at + n] == want
        at += n
    assert all(os.path.exists(p) for p in plan.files)


def test_refusals_and_their_messages(corpus, tmp_path):
    beyond = FaceFolder("beyond", make(tmp_path, "beyond", [4, 9]), 25, 4)          # every file at or past total_frames
    bare = FaceFolder("bare", make(tmp_path, "bare", [0], track="01"), 25, 3)       # no track directory 00
    gone = FaceFolder("gone", os.path.join(str(tmp_path), "gone"), 25, 3)           # no folder at all
    with pytest.raises(FileNotFoundError, match=r"folder beyond: no file below total_frames=4"):
        corpus_plan(corpus + [beyond], 5)
    for f in (bare, gone):
        with pytest.raises(FileNotFoundError, match=rf"folder {f.name}: no track directory .*{f.name}.00"):
            corpus_plan(corpus + [f], 5)
    for fps in (0, -25.0, float("nan")):
        with pytest.raises(ValueError, match=r"folder seven: fps must be a positive number"):
            corpus_plan([FaceFolder("seven", corpus[0].path, fps, 7)] + corpus[1:], 5)
    for total in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match=r"folder lone: total_frames must be an integer >= 1"):
            corpus_plan([corpus[0], FaceFolder("lone", corpus[1].path, 25, total)], 5)
    with pytest.raises(ValueError, match=r"folder names must be distinct: 'gaps' is given twice"):
        corpus_plan(corpus + [corpus[2]], 5)
    with pytest.raises(ValueError, match=r"folder names must be distinct"):
        corpus_plan(corpus + [corpus[2]], 5, skip_failed=True)
    for per in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match=r"max_frames_per_pass must be an integer >= 1"):
            corpus_plan(corpus, per)
    with pytest.raises(ZeroDivisionError, match=r"folder seven: integer division or modulo by zero"):
        corpus_plan([FaceFolder("seven", corpus[0].path, 2.0, 7)], 5)


def test_skip_failed_plans_the_rest_as_if_alone(corpus, tmp_path):
    bad = [FaceFolder("beyond", make(tmp_path, "beyond", [4, 9]), 25, 4), FaceFolder("gone", os.path.join(str(tmp_path), "gone"), 25, 3),
           FaceFolder("still", corpus[0].path, 0, 7)]
    mixed = [bad[0], corpus[0], bad[1], corpus[1], corpus[2], bad[2]]
    got, want = corpus_plan(mixed, 5, skip_failed=True), corpus_plan(corpus, 5)
    assert got.ok == [1, 3, 4] and sorted(got.errors) == [0, 2, 5]
    assert isinstance(got.errors[0], FileNotFoundError) and "beyond" in str(got.errors[0])
    assert isinstance(got.errors[2], FileNotFoundError) and "gone" in str(got.errors[2])
    assert isinstance(got.errors[5], ValueError) and "still" in str(got.errors[5])
    assert got.files == want.files and got.passes == want.passes and got.frame_off.tolist() == want.frame_off.tolist()
    for a, b in zip(got.host, want.host):
        np.testing.assert_array_equal(a, b)
    none = corpus_plan(bad, 5, skip_failed=True)
    assert none.ok == [] and none.passes == [] and none.n_tiles == 0


def test_refusals_of_the_call_come_before_the_engine_is_touched(corpus, tmp_path):
    """run_video_corpus with no engine at all: every refusal is raised before the first use of it."""
    for kw, what in ((dict(decode="cv2"), "decode must be"), (dict(entropy="gpu"), "entropy must be"), (dict(max_frames_per_pass=0), "max_frames_per_pass"),
                     (dict(max_windows_per_pass=0), "max_windows_per_pass"), (dict(flag_save_prob=True), "save_path")):
        with pytest.raises(ValueError, match=what):
            vc.run_video_corpus(None, corpus, **kw)
    with pytest.raises(FileNotFoundError, match="folder gone"):
        vc.run_video_corpus(None, corpus + [FaceFolder("gone", os.path.join(str(tmp_path), "gone"), 25, 3)])
    out = vc.run_video_corpus(None, [FaceFolder("gone", os.path.join(str(tmp_path), "gone"), 25, 3)], skip_failed=True)
    assert set(out[0]) == {"name", "error"} and out[0]["name"] == "gone" and out.passes == {"static": [], "lstm": []}


def test_list_corpus_with_and_without_the_frames_column(corpus, tmp_path):
    root = str(tmp_path)
    with_frames = os.path.join(root, "with.csv")
    with open(with_frames, "w") as f:
        f.write("name_video,frame_rate,total_frame\nseven.avi,25,7\nlone.mp4,25.0,8\ngaps.avi,29.97,12\nnowhere.avi,25,3\n")
    got = list_corpus(root, with_frames)
    assert [(g.name, g.fps, g.total_frames, g.track) for g in got] == [("seven", 25.0, 7, "00"), ("lone", 25.0, 8, "00"),
                                                                         ("gaps", 29.97, 12, "00"), ("nowhere", 25.0, 3, "00")]
    assert [g.path for g in got[:3]] == [c.path for c in corpus] and got[3].path == os.path.join(root, "nowhere")
    assert all(isinstance(g.total_frames, int) for g in got)
    with pytest.raises(FileNotFoundError, match="folder nowhere"):
        corpus_plan(got)
    assert corpus_plan(got, skip_failed=True).ok == [0, 1, 2]
    # without the column: the last file's number + 1 -- the files past the reference's count are counted here (`gaps` has 000040.jpg)
    without = os.path.join(root, "without.csv")
    with open(without, "w") as f:
        f.write("name_video,frame_rate\nseven.avi,25\nlone.mp4,25\ngaps.avi,30\n")
    got = list_corpus(root, without)
    assert [(g.name, g.total_frames) for g in got] == [("seven", 7), ("lone", 4), ("gaps", 41)]
    assert [int(p.sum()) for p in corpus_plan(got).presents] == [7, 1, 7]
    # the rows themselves, mixed; and a row that needs a listing it cannot have
    got = list_corpus(root, [("seven.avi", 25, 5), ("lone.mp4", 30)])
    assert [(g.name, g.fps, g.total_frames) for g in got] == [("seven", 25.0, 5), ("lone", 30.0, 4)]
    with pytest.raises(FileNotFoundError):
        list_corpus(root, [("nowhere.avi", 25)])
    make(tmp_path, "unnumbered", [], extra=("face.jpg",))
    with pytest.raises(FileNotFoundError, match="folder unnumbered: no NNNNNN.jpg"):
        list_corpus(root, [("unnumbered.avi", 25)])
    with pytest.raises(ValueError, match="frame_rate"):
        bad = os.path.join(root, "bad.csv")
        with open(bad, "w") as f:
            f.write("name_video,fps\nseven.avi,25\n")
        list_corpus(root, bad)
    # AFEW keeps its folders one level down, under the emotion
    make(os.path.join(root, "Happy"), "clip9", [0, 1])
    deep = list_corpus(root, [("clip9.avi", 25, 2)])[0]
    assert deep.path == os.path.join(root, "Happy", "clip9") and corpus_plan([deep]).n_tiles == 2
