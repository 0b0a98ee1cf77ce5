"""The `tracks=` option without a GPU: what is refused before any work, the per-track plan, and the per-track labels of the result
video (annotate.layout with dicts, annotate.draw_numpy as the CPU statement of the drawing)."""
import numpy as np
import pytest
import torch

from avcer_amd import annotate as an
from avcer_amd import run as arun
from avcer_amd.face_tiles import check_tracks, select_tracks, track_clip
from avcer_amd.video_pipeline import clips_plan, plan_clip, tracks_plan


class NoEngine:
    """An engine nothing may touch: every attribute read is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was used")


BAD = ("00", "ALL", "", [], (), [0, 0], [2, 1, 2], [-1], [True], [1.5], ["1"], 3, 0, True, 2.0, {0}, {0: 1}, np.array([[0, 1]]), np.array(1),
       [None])


# ---------------------------------------------------------------------------------------------------- selection
def test_check_tracks_accepts_none_all_and_lists_of_distinct_track_numbers():
    assert check_tracks(None) is None and check_tracks(None, flag_heatmaps=True) is None
    assert check_tracks("all") == "all"
    assert check_tracks([2, 0]) == (2, 0) and check_tracks((1,)) == (1,)
    got = check_tracks(np.array([3, 1], dtype=np.int32))
    assert got == (3, 1) and all(type(k) is int for k in got)
    for bad in BAD:
        with pytest.raises(ValueError, match="tracks"):
            check_tracks(bad)


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_a_bad_selection_is_refused_before_any_work(bad, tmp_path):
    frames, wav, dets = np.zeros((2, 8, 8, 3), dtype=np.uint8), np.zeros(1600, dtype=np.float32), [np.zeros((0, 15), dtype=np.float32)] * 2
    with pytest.raises(ValueError, match="tracks"):
        arun.run_inference(NoEngine(), frames, wav, 25, detections=dets, tracks=bad)
    # the file is never opened: a path that does not exist is not looked at (in memory and streamed)
    for more in ({}, {"stream_frames": 5}):
        with pytest.raises(ValueError, match="tracks"):
            arun.run_inference_file(NoEngine(), tmp_path / "missing.avi", detections=dets, tracks=bad, **more)
    with pytest.raises(ValueError, match="tracks"):
        an.write_result_video(NoEngine(), frames, np.zeros((0, 6), dtype=np.int64), {0: [0, 0]}, {0: np.ones((2, 7)) / 7}, tmp_path / "no.avi", 25,
                              tracks=bad)
    assert not (tmp_path / "no.avi").exists()


@pytest.mark.parametrize("tracks", ["all", [0], [1, 0]], ids=repr)
def test_heat_maps_and_tracks_together_are_refused_naming_both(tracks, tmp_path):
    frames, wav, dets = np.zeros((2, 8, 8, 3), dtype=np.uint8), np.zeros(1600, dtype=np.float32), [np.zeros((0, 15), dtype=np.float32)] * 2
    for call in (lambda: arun.run_inference(NoEngine(), frames, wav, 25, detections=dets, tracks=tracks, flag_heatmaps=True),
                 lambda: arun.run_inference_file(NoEngine(), tmp_path / "missing.avi", detections=dets, tracks=tracks, flag_heatmaps=True),
                 lambda: arun.run_inference_file(NoEngine(), tmp_path / "missing.avi", detections=dets, tracks=tracks, flag_heatmaps=True,
                                                 stream_frames=4)):
        with pytest.raises(ValueError) as e:
            call()
        assert "flag_heatmaps" in str(e.value) and "tracks" in str(e.value)


def test_result_video_refuses_a_track_without_a_prediction(tmp_path):
    frames = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    pred, prob = {0: [0, 0]}, {0: np.ones((2, 7)) / 7}
    with pytest.raises(ValueError, match="track 01"):
        an.write_result_video(NoEngine(), frames, np.zeros((0, 6), dtype=np.int64), pred, prob, tmp_path / "no.avi", 25, tracks=[0, 1])
    with pytest.raises(ValueError, match="dicts"):
        an.write_result_video(NoEngine(), frames, np.zeros((0, 6), dtype=np.int64), pred[0], prob[0], tmp_path / "no.avi", 25, tracks="all")
    assert not (tmp_path / "no.avi").exists()


def records_of(spans):
    """records int64 [n,6] in the tracker's order (by frame, then by track) for {track: frames}."""
    rows = sorted((t, k) for k, frames in spans.items() for t in frames)
    return np.array([[t, k, 1 + k, 2, 9 + k, 12] for t, k in rows], dtype=np.int64).reshape(-1, 6)


def test_select_tracks_names_what_is_missing():
    rec = records_of({0: range(3), 2: [1], 5: [2]})
    assert select_tracks(rec, "all") == (0, 2, 5)
    assert select_tracks(rec, (5, 0)) == (5, 0)
    with pytest.raises(FileNotFoundError, match="no face track 03"):
        select_tracks(rec, (0, 3))
    with pytest.raises(FileNotFoundError, match="no face track 01"):
        select_tracks(rec, (1,))
    empty = np.zeros((0, 6), dtype=np.int64)
    with pytest.raises(FileNotFoundError, match="no face track"):
        select_tracks(empty, "all")
    with pytest.raises(FileNotFoundError, match="no face track 00"):
        select_tracks(empty, (0,))


# ---------------------------------------------------------------------------------------------------- the plan
T = 23
SPANS = {0: [t for t in range(17) if t not in (5, 6, 7)],   # a gap: the window restarts behind it
         1: [10],                                           # a single frame, on the LSTM's stride at 25 fps and off it at 30
         2: list(range(8, T))}                              # starts late: zero rows in front


@pytest.mark.parametrize("fps", [25, 30])
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1), (1,), (2, 1)])
def test_plan_of_the_selected_tracks_is_plan_clip_per_track_laid_end_to_end(fps, order):
    rec = records_of(SPANS)
    tp = tracks_plan(rec, order, T, fps)
    assert tp.tracks == order and tp.present.shape == (len(order), T)
    tiles = torch.arange(len(rec), dtype=torch.uint8)[:, None, None, None].expand(len(rec), 224, 224, 3)
    f_off, w_off = [0], [0]
    for i, k in enumerate(order):
        clip, present = track_clip(rec, tiles, k, T)                                  # what the code as it stands feeds visual_forward
        np.testing.assert_array_equal(tp.present[i], present)
        assert present.tolist() == [t in SPANS[k] for t in range(T)]
        want = plan_clip(present, fps, f_off[-1], w_off[-1])
        f_off.append(f_off[-1] + int(present.sum()))
        w_off.append(w_off[-1] + len(want.windows))
        assert tp.static_src[i * T:(i + 1) * T].tolist() == want.static_src
        assert tp.dyn_src[i * T:(i + 1) * T].tolist() == want.dyn_src
        assert tp.windows[w_off[i]:w_off[i + 1]].tolist() == want.windows
        # the compact tile list: the track's tiles in frame order, and nothing else
        rows = tp.rows[f_off[i]:f_off[i + 1]]
        assert (rec[rows, 1] == k).all() and rec[rows, 0].tolist() == SPANS[k]
        assert torch.equal(tiles[torch.from_numpy(rows)], clip[torch.from_numpy(present)])
        # a track's rows never point outside its own features and windows (or at the zero row)
        s, d = tp.static_src[i * T:(i + 1) * T], tp.dyn_src[i * T:(i + 1) * T]
        assert ((s == -1) | ((s >= f_off[i]) & (s < f_off[i + 1]))).all() and ((d == -1) | ((d >= w_off[i]) & (d < w_off[i + 1]))).all()
        w = tp.windows[w_off[i]:w_off[i + 1]]
        assert w.size == 0 or (w.min() >= f_off[i] and w.max() < f_off[i + 1])
    assert tp.feat_off.tolist() == f_off and tp.win_off.tolist() == w_off              # the offsets tile the concatenation
    assert len(tp.rows) == f_off[-1] == sum(len(SPANS[k]) for k in order) and len(tp.windows) == w_off[-1]
    assert len(tp.static_src) == len(tp.dyn_src) == len(order) * T
    for a, b in zip(clips_plan(tp.present, fps), (tp.static_src, tp.dyn_src, tp.windows, tp.feat_off, tp.win_off)):
        np.testing.assert_array_equal(a, b)


def test_plan_cases_reach_every_rule():
    """The hand-written tracks do what their comments say at both frame rates."""
    for fps, step in ((25, 5), (30, 6)):
        gap = plan_clip(tracks_plan(records_of(SPANS), (0,), T, fps).present[0], fps)
        assert gap.static_src[5:8] == [4, 4, 4] and gap.static_src[17:] == [13] * 6      # hold-last in the gap and behind the end
        assert any(len(set(w)) == 1 for w in gap.windows[1:])                            # a window restarted behind the gap
        one = plan_clip(tracks_plan(records_of(SPANS), (1,), T, fps).present[0], fps)
        assert len(one.windows) == (1 if 10 % step == 0 else 0) and one.static_src[:10] == [-1] * 10
        late = plan_clip(tracks_plan(records_of(SPANS), (2,), T, fps).present[0], fps)
        assert late.dyn_src[:8] == [-1] * 8 and late.windows[0] == [late.windows[0][0]] * 10


# ---------------------------------------------------------------------------------------------------- labels
H, W, N = 48, 64, 3


def label_case():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    # two boxes that overlap (and whose labels overlap): the later item wins, so order matters
    rec = np.array([[0, 0, 6, 20, 40, 44], [0, 1, 14, 24, 60, 46], [1, 0, 7, 20, 41, 44], [1, 1, 15, 24, 61, 46], [2, 1, 16, 24, 62, 46],
                    [2, 2, 2, 2, 12, 12]], dtype=np.int64)
    prob = {k: rng.dirichlet(np.ones(7), size=N) for k in (0, 1, 2)}
    pred = {k: p.argmax(axis=1) for k, p in prob.items()}
    return frames, rec, pred, prob


class BoxFont:
    """A font whose metrics are written down here: every character is 3 pixels wide, a text's mask is 7 rows of coverage 200 that
    start 2 rows below its origin, and its advance is 3 * len + 0.4 (rounded: 3 * len)."""

    class Mask:
        def __init__(self, w, h):
            self.size = (w, h)

        def __array__(self, dtype=None, copy=None):
            return np.full(self.size[0] * self.size[1], 200, dtype=dtype or np.uint8)

    def getmask(self, text, mode):
        assert mode == "L"
        return self.Mask(3 * len(text), 7)

    def getbbox(self, text):
        return (0, 2, 3 * len(text), 9)

    def getlength(self, text):
        return 3 * len(text) + 0.4


def test_items_of_a_labelled_record_written_out_by_hand():
    """60 x 200 frames: lw = max(round((60 + 200 + 3) / 2 * 0.003), 2) = 2.  With BoxFont "Happily Surprised: " (19 characters)
    advances 57 and "50.00%" is 18 wide: tw = 75, th = 9, the backdrop is 79 x 13.  Frame 1, box (100, 20, 140, 44): bx = 100 + 41 // 2
    - 79 // 2 = 81, by = 20 - 13 = 7.  Frame 2, box (100, 5, 140, 30), "Fearfully Surprised: " (21 characters, advance 63) and
    "25.00%": the backdrop is 85 x 13, bx = 100 + 20 - 42 = 78, and 5 - 13 < 0 puts it inside the box at by = 5 + lw = 7.  The seven
    names are masks 0..6, the numbers follow in the order of their first use."""
    h, w = 60, 200
    rec = np.array([[1, 0, 100, 20, 140, 44], [1, 1, 10, 30, 50, 58], [2, 0, 100, 5, 140, 30]], dtype=np.int64)
    pred = np.array([3, 1, 0])
    prob = np.zeros((3, 7))
    prob[1, 1], prob[2, 0] = 0.5, 0.25
    magenta, black = (255, 0, 255), (0, 0, 0)
    want = [(1, an.OUTLINE, 100, 20, 140, 44, 2, 0, magenta, 0),
            (1, an.FILL, 81, 7, 159, 19, 160, 0, black, 0),
            (1, an.MASK, 83, 11, 0, 0, 1, 1, magenta, 0),
            (1, an.MASK, 140, 11, 0, 0, 1, 7, magenta, 0),
            (1, an.OUTLINE, 10, 30, 50, 58, 2, 0, magenta, 0),                         # track 01: a bare box
            (2, an.OUTLINE, 100, 5, 140, 30, 2, 0, magenta, 0),
            (2, an.FILL, 78, 7, 162, 19, 160, 0, black, 0),
            (2, an.MASK, 80, 11, 0, 0, 1, 0, magenta, 0),
            (2, an.MASK, 143, 11, 0, 0, 1, 8, magenta, 0)]
    font = BoxFont()
    for form in ((pred, prob), ({0: pred}, {0: prob})):
        items, masks = an.layout(rec, *form, h, w, font=font)
        np.testing.assert_array_equal(items, an.as_items(want))
        assert [m.shape for m in masks] == [(7, 3 * len(n + ": ")) for n in an.COMPOUND_NAMES] + [(7, 18), (7, 18)]
        assert all((m == 200).all() for m in masks)
    # the dict form on track 01 instead: its box (10, 30, 50, 58) carries the label, "Happily Surprised: " + "50.00%" on frame 1:
    # bx = 10 + 41 // 2 - 39 = -9 -> 0, by = 30 - 13 = 17; track 00 keeps bare boxes
    items, _ = an.layout(rec, {1: pred}, {1: prob}, h, w, font=font)
    np.testing.assert_array_equal(items, an.as_items([want[0], want[4], (1, an.FILL, 0, 17, 78, 29, 160, 0, black, 0),
                                                      (1, an.MASK, 2, 21, 0, 0, 1, 1, magenta, 0), (1, an.MASK, 59, 21, 0, 0, 1, 7, magenta, 0),
                                                      want[5]]))


def test_layout_of_track_00_alone_is_the_positional_call():
    _, rec, pred, prob = label_case()
    for panel in (False, True):
        old_items, old_masks = an.layout(rec, pred[0], prob[0], H, W, panel=panel)
        new_items, new_masks = an.layout(rec, {0: pred[0]}, {0: prob[0]}, H, W, panel=panel)
        np.testing.assert_array_equal(new_items, old_items)
        assert len(new_masks) == len(old_masks) and all(np.array_equal(a, b) for a, b in zip(new_masks, old_masks))
    # and within the full list, track 00's items are the same records
    full, full_masks = an.layout(rec, pred, prob, H, W)
    alone, alone_masks = an.layout(rec[rec[:, 1] == 0], pred[0], prob[0], H, W)

    def told(items, masks):
        return [(tuple(int(it[f]) for f in ("frame", "kind", "x0", "y0", "x1", "y1", "arg")), tuple(it["colour"].tolist()),
                 masks[int(it["mask"])].tobytes() if it["kind"] == an.MASK else None) for it in items]

    assert [x for x in told(alone, alone_masks) if x in told(full, full_masks)] == told(alone, alone_masks)
    assert len(full) == len(rec) + 3 * len(rec)                                       # every box, and a label (3 items) on each
    with pytest.raises(ValueError, match="layout"):
        an.layout(rec, pred, prob[0], H, W)
    with pytest.raises(ValueError, match="layout"):
        an.layout(rec, {0: pred[0], 1: pred[1]}, {1: prob[1], 0: prob[0]}, H, W)


@pytest.mark.parametrize("flip", [False, True])
def test_drawing_all_tracks_is_drawing_them_one_after_the_other(flip):
    frames, rec, pred, prob = label_case()
    if flip:  # track 01 in front of track 00 within every frame: the items follow the records
        rec = rec[np.lexsort((-rec[:, 1], rec[:, 0]))]
    sel = (0, 1)
    items, masks = an.layout(rec, {k: pred[k] for k in sel}, {k: prob[k] for k in sel}, H, W)
    got = an.draw_numpy(frames.copy(), items, masks)
    want = frames.copy()
    for t in range(N):  # per frame, in record order: a track's box and label, then the next track's
        for r in rec[rec[:, 0] == t]:
            k = int(r[1])
            one = an.layout(r[None], {k: pred[k]}, {k: prob[k]}, H, W) if k in sel else an.layout(r[None], {9: pred[0]}, {9: prob[0]}, H, W)
            an.draw_numpy(want, *one)
    np.testing.assert_array_equal(got, want)
    assert (items["kind"] == an.OUTLINE).sum() == len(rec) and (items["kind"] == an.FILL).sum() == 5   # track 02: a bare box
    # the labels of track 01 are there: the positional call draws another picture
    old = an.draw_numpy(frames.copy(), *an.layout(rec, pred[0], prob[0], H, W))
    assert not np.array_equal(got, old)
    # and the order within a frame matters in this case, or the test would show nothing
    other = an.draw_numpy(frames.copy(), *an.layout(rec[np.lexsort(((1 if flip else -1) * rec[:, 1], rec[:, 0]))],
                                                  {k: pred[k] for k in sel}, {k: prob[k] for k in sel}, H, W))
    assert not np.array_equal(got, other)


def test_the_panel_shows_the_first_track_of_the_dict():
    _, rec, pred, prob = label_case()
    none = np.zeros((0, 6), dtype=np.int64)
    want, want_masks = an.layout(none, pred[1], prob[1], H, W, panel=True)
    got, got_masks = an.layout(none, {1: pred[1], 0: pred[0]}, {1: prob[1], 0: prob[0]}, H, W, panel=True)
    np.testing.assert_array_equal(got, want)
    assert all(np.array_equal(a, b) for a, b in zip(got_masks, want_masks))
    other, _ = an.layout(none, {0: pred[0], 1: pred[1]}, {0: prob[0], 1: prob[1]}, H, W, panel=True)
    assert not np.array_equal(other, want)
