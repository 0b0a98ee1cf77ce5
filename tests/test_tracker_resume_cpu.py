"""The resumable face tracker (include/avcer_hip.h avcer_tracker_*, engine.FaceTracker): a video pushed in pieces of any size gives the
records of avcer_track_faces on the whole, and an error names the frame of the whole video.  Host code only: no device."""
import ctypes

import numpy as np
import pytest

FRAMES, W, H = 60, 640, 360


def _lib():
    from avcer_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(build.LIB)
    for name in ("avcer_track_faces", "avcer_tracker_create", "avcer_tracker_push", "avcer_tracker_last_error", "avcer_tracker_destroy"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def _whole(lib, dets, iou=0.4, min_size=0.0):
    from avcer_amd.engine import _pack_detections

    boxes, counts, rec = _pack_detections(dets)
    n = ctypes.c_int64(0)
    rc = lib.avcer_track_faces(None, boxes.ctypes.data_as(ctypes.c_void_p), 4, counts.ctypes.data_as(ctypes.c_void_p), len(counts), W, H,
                               iou, min_size, rec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
    assert rc == 0
    return rec[:n.value].copy()


def _pushed(lib, dets, cuts, iou=0.4, min_size=0.0):
    from avcer_amd.engine import FaceTracker

    tr = FaceTracker(lib, iou, min_size)
    parts = [tr.push(dets[a:b], W, H).copy() for a, b in zip([0] + list(cuts), list(cuts) + [len(dets)])]
    assert tr.frames == len(dets)
    tr.close()
    return np.concatenate(parts)


def _video(seed):
    """60 frames of 0..4 boxes: faces that drift, are missed, JUMP (the track dies and a new one is born), and frames without any
    box (every tracklet is dropped; the counter runs on)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform([60, 60], [W - 60, H - 60], (4, 2))
    size = rng.uniform(45, 90, 4)                                      # above the minimum face size of the second run
    dets = []
    for t in range(FRAMES):
        centres += rng.normal(0, 3, centres.shape)
        rows = []
        for f in range(4):
            if rng.uniform() < 0.1:
                centres[f] = rng.uniform([60, 60], [W - 60, H - 60])     # a jump: no overlap with the tracklet it left
            if rng.uniform() < 0.25:
                continue                                                  # missed
            (cx, cy), s = centres[f], size[f]
            rows.append([cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2, 0.9] + [0.0] * 10)
        if rng.uniform() < 0.12 or t in (17, 18):
            rows = []                                                     # a frame without faces (two in a row at 17, 18)
        order = rng.permutation(len(rows))
        dets.append(np.array([rows[i] for i in order], np.float32).reshape(-1, 15))
    return dets


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_split_of_the_video_gives_the_records_of_the_whole(seed):
    lib = _lib()
    dets = _video(seed)
    counts = [len(d) for d in dets]
    assert 0 in counts and max(counts) >= 3
    for min_size in (0.0, 40.0):
        want = _whole(lib, dets, min_size=min_size)
        assert len(want) and want[:, 1].max() >= 4, "tracks must die and be reborn in this video"
        np.testing.assert_array_equal(_pushed(lib, dets, [], min_size=min_size), want)          # one piece
        for cut in range(1, FRAMES):                                                            # every single frame border
            np.testing.assert_array_equal(_pushed(lib, dets, [cut], min_size=min_size), want, err_msg=f"cut at {cut}")
        for chunk in (1, 7, 16):
            np.testing.assert_array_equal(_pushed(lib, dets, list(range(chunk, FRAMES, chunk)), min_size=min_size), want, err_msg=f"chunks of {chunk}")


def test_an_empty_push_and_a_push_of_empty_frames_change_nothing_they_should_not():
    lib = _lib()
    dets = _video(3)
    want = _whole(lib, dets)
    from avcer_amd.engine import FaceTracker

    tr = FaceTracker(lib)
    got = [tr.push(dets[:20], W, H).copy(), tr.push([], W, H).copy(), tr.push(dets[20:], W, H).copy()]
    assert len(got[1]) == 0 and got[1].shape == (0, 6)
    np.testing.assert_array_equal(np.concatenate(got), want)


def test_errors_name_the_frame_of_the_whole_video():
    lib = _lib()
    from avcer_amd.engine import FaceTracker

    good = [np.array([[10, 10, 60, 60, 0.9] + [0] * 10], np.float32)] * 7
    tr = FaceTracker(lib)
    tr.push(good, W, H)
    tr.push(good, W, H)
    third = list(good)
    third[3] = np.array([[10, 10, 10, 50, 0.9] + [0] * 10], np.float32)                          # zero area: frame 14 + 3
    with pytest.raises(ValueError, match=r"^frame 17: a zero-area detection has no track id \(TypeError in the reference\)$"):
        tr.push(third, W, H)
    with pytest.raises(ValueError, match="frame 17"):                                            # and takes no further push
        tr.push(good, W, H)
    tr = FaceTracker(lib)
    tr.push(good, W, H)
    outside = [good[0], np.array([[700, 10, 760, 50, 0.9] + [0] * 10], np.float32)]
    with pytest.raises(ValueError, match=r"^frame 8: empty crop \(640, 10, 640, 50\) \(cv2.imwrite fails in the reference\)$"):
        tr.push(outside, W, H)
    # the whole-video call keeps its text: the same sentence, counted from its own frame 0
    from avcer_amd.engine import _pack_detections

    boxes, counts, rec = _pack_detections(good[:2] + [third[3]])
    n = ctypes.c_int64(0)
    assert lib.avcer_track_faces(None, boxes.ctypes.data_as(ctypes.c_void_p), 4, counts.ctypes.data_as(ctypes.c_void_p), 3, W, H, 0.4, 0.0,
                                 rec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)) == -1
