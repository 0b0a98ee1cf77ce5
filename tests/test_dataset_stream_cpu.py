"""The host code of run_dataset(stream_frames=N) (avcer_amd/dataset.py), without a GPU: how known records are dealt out to the frame
passes (pass_rows), the checks on what VideoJob.open hands out (checked_passes), the argument check, and VideoJob's new field.  The
first two are held to a brute-force statement over every video length 0..70 and every pass size 1..80."""
import numpy as np
import pytest

from avcer_amd.dataset import VideoJob, check_stream_frames, checked_passes, pass_rows, run_dataset

LENGTHS, SIZES = range(0, 71), range(1, 81)


def job(n, h=2, w=3, **kw):
    return VideoJob("clip", n, h, w, 25, 1600, **kw)


def frame_column(n, seed):
    """The frame column of a video's records in frame order: frames 0..n-1, each with 0 to 3 records (faces come and go)."""
    return np.repeat(np.arange(n), np.random.default_rng(seed).integers(0, 4, n))


def test_pass_rows_deals_every_row_to_the_pass_of_its_frame():
    for n in LENGTHS:
        col = frame_column(n, n)
        for per in SIZES:
            dealt = []
            for a in range(0, n, per):
                b = min(a + per, n)
                lo, hi = pass_rows(col, a, b)
                assert list(range(lo, hi)) == [r for r, f in enumerate(col) if a <= f < b], (n, per, a)
                dealt.extend(range(lo, hi))
            assert dealt == list(range(len(col))), (n, per)                   # every row once, in order


def test_checked_passes_yields_every_frame_once_at_its_offset():
    for n in LENGTHS:
        clip = np.arange(n * 18, dtype=np.int64).astype(np.uint8).reshape(n, 2, 3, 3)
        for per in SIZES:
            got = list(checked_passes(job(n), (clip[a:a + per] for a in range(0, n, per)), per))
            assert [a for a, _ in got] == list(range(0, n, per)), (n, per)
            assert all(1 <= f.shape[0] <= per for _, f in got) and sum(f.shape[0] for _, f in got) == n
            assert np.array_equal(np.concatenate([f.numpy() for _, f in got] or [clip[:0]]), clip), (n, per)


def test_checked_passes_takes_uneven_and_empty_batches():
    clip = np.zeros((10, 2, 3, 3), dtype=np.uint8)
    got = list(checked_passes(job(10), [clip[:3], clip[:0], clip[3:4], clip[4:10]], 6))
    assert [(a, f.shape[0]) for a, f in got] == [(0, 3), (3, 1), (4, 6)]


@pytest.mark.parametrize("n", [0, 1, 7, 70])
@pytest.mark.parametrize("per", [1, 7, 16, 80])
def test_checked_passes_refuses_what_the_metadata_does_not_say(n, per):
    clip = np.zeros((n + per + 1, 2, 3, 3), dtype=np.uint8)

    def run(batches):
        return list(checked_passes(job(n), batches, per))

    whole = [clip[a:min(a + per, n)] for a in range(0, n, per)]
    run(whole)
    with pytest.raises(ValueError, match="clip"):                             # a batch larger than asked
        run([clip[:per + 1]] + whole)
    with pytest.raises(ValueError, match="clip"):                             # more frames than the job says
        run(whole + [clip[:1]])
    if n:
        with pytest.raises(ValueError, match="clip"):                         # fewer
            run(whole[:-1] + [whole[-1][:-1]])
        for bad in (np.zeros((1, 3, 3, 3), np.uint8), np.zeros((1, 2, 4, 3), np.uint8), np.zeros((1, 2, 3, 4), np.uint8), np.zeros((2, 3, 3), np.uint8)):
            with pytest.raises(ValueError, match="clip"):                     # another frame size, no batch axis
                run([bad] + whole)


def test_checked_passes_holds_no_batch_once_the_next_is_asked_for():
    import weakref

    alive = []

    def batches():
        for _ in range(4):
            assert not any(r() is not None for r in alive)                    # every earlier batch is gone
            b = np.zeros((2, 2, 3, 3), dtype=np.uint8)
            alive.append(weakref.ref(b))
            yield b
            del b

    for _, frames in checked_passes(job(8), batches(), 2):
        del frames
    assert len(alive) == 4


def test_stream_frames_values():
    assert check_stream_frames(None) is None and check_stream_frames(1) == 1 and check_stream_frames(np.int64(64)) == 64
    for bad in (0, -3, 2.5, True, "64", np.bool_(True)):
        with pytest.raises(ValueError, match="stream_frames"):
            check_stream_frames(bad)


def test_video_job_keeps_its_positional_fields_and_open_comes_last():
    j = VideoJob("v", 2, 8, 9, 25, 1600, 44100, len, [1, 2])
    assert (j.wav_sr, j.load, j.detections, j.open) == (44100, len, [1, 2], None)
    assert VideoJob("v", 2, 8, 9, 25, 1600, open=len).open is len


def test_run_dataset_refuses_before_any_work():
    calls = []
    dets = [np.zeros((0, 15), dtype=np.float32)] * 2

    def never(*a):
        calls.append(a)
        raise AssertionError("a job was touched")

    both = VideoJob("v", 2, 8, 8, 25, 1600, detections=dets, load=never, open=never)
    for bad in (0, -3, 2.5, True, "64"):
        with pytest.raises(ValueError, match="stream_frames"):
            run_dataset(object(), [both], stream_frames=bad)
    with pytest.raises(ValueError, match="only_load"):
        run_dataset(object(), [both, VideoJob("only_load", 2, 8, 8, 25, 1600, detections=dets, load=never)], stream_frames=8)
    assert calls == []
