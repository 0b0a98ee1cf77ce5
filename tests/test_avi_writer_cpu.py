"""avi.AviWriter: frames appended as they come, the header patched at close -- byte for byte the file avi.write_avi writes from the
same blobs and PCM (and the bytes avi.build_avi states on its own), however the frames were cut into calls; open_avi reads every
file back; the 4 GiB refusal, tested through the module's limit."""
import numpy as np
import pytest

from avcer_amd import avi
from test_avi_cpu import blobs_of, pcm_of

W = H = 16


def written(tmp_path, name, blobs, chunk, rate, scale, pcm, audio_rate, by_set_pcm=False):
    path = tmp_path / name
    ch = None if pcm is None else (1 if pcm.ndim == 1 else pcm.shape[1])
    w = avi.AviWriter(path, W, H, rate, scale, audio_rate=audio_rate, channels=ch, pcm=None if by_set_pcm else pcm)
    if by_set_pcm and pcm is not None:
        w.set_pcm(pcm)
    for a in range(0, len(blobs), chunk):
        assert w.add_frames(blobs[a:a + chunk]) is w
    assert w.n_frames == len(blobs)
    assert w.close() == path and w.close() == path
    return path.read_bytes()


CASES = {
    "mute": dict(rate=25, scale=1, pcm=None, audio_rate=44100),
    "stereo": dict(rate=25, scale=1, pcm=pcm_of(44100 * 13 // 25 + 77, 2), audio_rate=44100),
    "mono_ntsc": dict(rate=30000, scale=1001, pcm=pcm_of(9001, 1), audio_rate=16000),                 # scale != 1
    "short_sound": dict(rate=24000, scale=1001, pcm=pcm_of(1500, 2), audio_rate=48000),                # the sound ends before the picture
}


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_writer_equals_write_avi_however_the_frames_are_cut(tmp_path, case, dropped):
    c = CASES[case]
    blobs = blobs_of(13, W, H)
    if dropped:
        blobs[4] = blobs[5] = blobs[12] = b""                                                         # repeated frames, the last one too
    want = avi.build_avi(blobs, c["rate"], c["scale"], c["pcm"], c["audio_rate"])
    assert (tmp_path / "ref.avi") == avi.write_avi(tmp_path / "ref.avi", blobs, c["rate"], c["scale"], c["pcm"], c["audio_rate"])
    assert (tmp_path / "ref.avi").read_bytes() == want
    for chunk in (1, 5, 13):
        for by_set_pcm in (False, True):
            got = written(tmp_path, f"w{chunk}.avi", blobs, chunk, c["rate"], c["scale"], c["pcm"], c["audio_rate"], by_set_pcm)
            assert got == want, (case, dropped, chunk, by_set_pcm)
    with avi.open_avi(tmp_path / "w5.avi") as a:
        assert (a.n_frames, a.width, a.height, a.rate, a.scale) == (13, W, H, c["rate"], c["scale"])
        shown = [b if b else None for b in blobs]
        for k in range(13):
            shown[k] = shown[k] if shown[k] is not None else shown[k - 1]
        assert [bytes(f) for f in a.frames] == shown
        if c["pcm"] is None:
            assert a.pcm is None
        else:
            np.testing.assert_array_equal(a.pcm, c["pcm"].reshape(len(c["pcm"]), -1))
            assert a.audio_rate == c["audio_rate"]


def test_writer_without_index_and_as_a_context(tmp_path):
    blobs, pcm = blobs_of(6, W, H), pcm_of(4000, 2)
    with avi.AviWriter(tmp_path / "n.avi", W, H, 25, pcm=pcm, index=False) as w:
        w.add_frames(memoryview(b) for b in blobs)
    assert (tmp_path / "n.avi").read_bytes() == avi.build_avi(blobs, 25, 1, pcm, index=False)
    with pytest.raises(RuntimeError, match="boom"):                                                    # an exception in the block: no partial file
        with avi.AviWriter(tmp_path / "gone.avi", W, H, 25) as w:
            w.add_frames(blobs[:2])
            assert (tmp_path / "gone.avi").exists()
            raise RuntimeError("boom")
    assert not (tmp_path / "gone.avi").exists()


def test_writer_refusals(tmp_path):
    blobs = blobs_of(3, W, H)
    with pytest.raises(ValueError, match="rate and scale"):
        avi.AviWriter(tmp_path / "x.avi", W, H, 0)
    with pytest.raises(ValueError, match="pcm int16"):
        avi.AviWriter(tmp_path / "x.avi", W, H, 25, pcm=np.zeros(10, dtype=np.float32))
    with pytest.raises(ValueError, match="2 channels"):
        avi.AviWriter(tmp_path / "x.avi", W, H, 25, channels=1, pcm=pcm_of(10, 2))
    w = avi.AviWriter(tmp_path / "late.avi", W, H, 25)
    w.add_frames(blobs[:1])
    with pytest.raises(ValueError, match="before the first frame"):
        w.set_pcm(pcm_of(10, 2))
    w.close()
    with pytest.raises(ValueError, match="closed"):
        w.add_frames(blobs[1:])
    w = avi.AviWriter(tmp_path / "none.avi", W, H, 25)                                                 # no frame, or dropped frames alone
    w.add_frames([b"", b""])
    with pytest.raises(ValueError, match="no frame"):
        w.close()
    assert not (tmp_path / "none.avi").exists() and not (tmp_path / "x.avi").exists()
    with pytest.raises(ValueError, match="no frame"):
        avi.write_avi(tmp_path / "none.avi", [], 25)
    assert not (tmp_path / "none.avi").exists()


@pytest.mark.parametrize("sound", [False, True])
def test_the_4_gib_limit_through_the_module_constant(tmp_path, monkeypatch, sound):
    blobs = blobs_of(8, W, H)
    pcm = pcm_of(8 * 1764, 2) if sound else None
    whole = len(avi.build_avi(blobs, 25, 1, pcm))
    monkeypatch.setattr(avi, "AVI_MAX_BYTES", whole + 64)                                              # the whole file fits (a few bytes of slack) ...
    assert len(written(tmp_path, "fits.avi", blobs, 3, 25, 1, pcm, 44100)) == whole
    # ... and one that does not is refused at the append that would cross the limit -- the last frame's -- and the partial file removed
    monkeypatch.setattr(avi, "AVI_MAX_BYTES", whole - len(blobs[-1]) // 2)
    w = avi.AviWriter(tmp_path / "big.avi", W, H, 25, pcm=pcm)
    with pytest.raises(OSError, match=r"4 GiB") as e:
        for k, b in enumerate(blobs):
            w.add_frames([b])
            assert (tmp_path / "big.avi").exists()
    assert str(whole - len(blobs[-1]) // 2) in str(e.value)
    assert not isinstance(e.value, ValueError) and k == 7
    assert not (tmp_path / "big.avi").exists()
    with pytest.raises(ValueError, match="closed"):
        w.add_frames(blobs[:1])
    with pytest.raises(OSError, match="4 GiB"):
        avi.write_avi(tmp_path / "big2.avi", blobs, 25, 1, pcm)
    assert not (tmp_path / "big2.avi").exists()
