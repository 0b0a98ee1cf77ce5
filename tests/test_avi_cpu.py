"""Motion-JPEG AVI files on the host (avcer_amd/avi.py) and the annex-K default Huffman tables of the header pass
(AVCER_JPEG_STD_TABLES, csrc/jpeg_decode.hip): write_avi -> open_avi round trips, every refusal of the reader by name, truncation at
every byte, and frames whose DHT segments were cut out against the untouched files -- through the host entropy pass and through
the host form of the device decoder, tolerance zero.  No device."""
import ctypes
import io
import struct

import numpy as np
import pytest
from PIL import Image

from avcer_amd import avi, jpeg

SIZES = ((50, 38), (16, 16))                                     # (w, h)
KINDS = (("420", 2), ("422", 1), ("444", 0), ("grey", None))     # PIL's subsampling; None: mode L


def picture(w, h, seed, grey=False):
    """A smooth picture with some noise: every coefficient band is used, no file is trivial."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(5 * x + 3 * y) % 256, (7 * y + 40) % 256, (3 * x * y // 8 + 90) % 256], axis=-1)
    img = np.clip(base + rng.integers(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    return img[..., 0] if grey else img


def jpeg_file(w, h, seed, subsampling, quality=88, **kw):
    buf = io.BytesIO()
    if subsampling is None:
        Image.fromarray(picture(w, h, seed, True), "L").save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(picture(w, h, seed)).save(buf, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def segments(blob):
    """[(marker, start, end)] of the header segments of a JPEG file up to and including SOS."""
    out, p = [], 2
    while True:
        assert blob[p] == 0xFF
        m = blob[p + 1]
        n = (blob[p + 2] << 8) | blob[p + 3]
        out.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def cut_dht(blob, keep=()):
    """`blob` without its DHT segments, but those whose (class, id) byte is in `keep` (PIL writes one table per segment)."""
    drop = [(a, b) for m, a, b in segments(blob) if m == 0xC4 and blob[a + 4] not in keep]
    assert drop
    out, at = b"", 0
    for a, b in drop:
        out += blob[at:a]
        at = b
    return out + blob[at:]


@pytest.fixture(scope="module")
def lib():
    from avcer_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(build.LIB)
    for name in ("avcer_jpeg_probe", "avcer_jpeg_entropy_batch", "avcer_jpeg_entropy_batch_ex", "avcer_jpeg_scan_batch",
                 "avcer_jpeg_scan_batch_ex", "avcer_jpeg_unpack_host"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def files():
    """[(name, untouched file, the file without DHT)]"""
    out = []
    for w, h in SIZES:
        for k, (name, sub) in enumerate(KINDS):
            blob = jpeg_file(w, h, 100 * w + k, sub)
            out.append((f"{name}_{w}x{h}", blob, cut_dht(blob)))
    return out


def entropy(lib, blobs, **kw):
    desc = np.zeros(len(blobs), dtype=jpeg.DESC)
    coeffs = np.zeros(64 * 4096, dtype=np.int16)
    jpeg.entropy_batch(lib, blobs, coeffs, desc, 2, **kw)
    return coeffs.reshape(-1, 64), desc


def scan(lib, blobs, **kw):
    n = len(blobs)
    data = np.zeros(sum(len(b) for b in blobs) + 16 * n, dtype=np.uint8)
    desc, sc, tabs = np.zeros(n, dtype=jpeg.DESC), np.zeros(n, dtype=jpeg.SCAN), np.zeros(4 * n + 4, dtype=jpeg.TAB)
    n_tabs, _, blocks = jpeg.scan_batch(lib, blobs, data, desc, sc, tabs, 2, **kw)
    return data, desc, sc, tabs[:n_tabs], blocks


# ---------------------------------------------------------------------------------------------------- annex-K default tables
def test_the_library_exports_the_new_calls():
    from avcer_amd import _lib, build

    build.build()
    for name in ("avcer_jpeg_frames", "avcer_jpeg_entropy_batch_ex", "avcer_jpeg_scan_batch_ex"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(build.LIB), name)


def test_frames_without_dht_decode_to_the_coefficients_of_the_untouched_files(lib, files):
    whole, cut = [b for _, b, _ in files], [c for _, _, c in files]
    wc, wd = entropy(lib, whole)
    assert (wd["status"] == jpeg.OK).all()
    for blobs in (cut, [memoryview(c) for c in cut]):  # bytes, and buffers as a mapped AVI file hands them out
        gc, gd = entropy(lib, blobs, std_tables=True)
        assert (gd["status"] == jpeg.OK).all(), gd["reason"]
        for f in ("width", "height", "ncomp", "hs", "vs", "bw", "bh", "coef_block", "n_blocks", "qt"):
            np.testing.assert_array_equal(gd[f], wd[f], err_msg=f)
        used = int((wd["coef_block"] + wd["n_blocks"]).max())
        np.testing.assert_array_equal(gc[:used], wc[:used])
    # the untouched files are the same with the flag as without
    gc, gd = entropy(lib, whole, std_tables=True)
    np.testing.assert_array_equal(gc, wc)
    np.testing.assert_array_equal(gd, wd)


def test_the_existing_entry_points_still_refuse_them(lib, files):
    cut = [c for _, _, c in files]
    _, d = entropy(lib, cut)
    assert (d["status"] == jpeg.NOT_HANDLED).all() and (d["reason"] == 8).all()  # R_TABLE, as before
    _, d, _, tabs, blocks = scan(lib, cut)
    assert (d["status"] == jpeg.NOT_HANDLED).all() and (d["reason"] == 8).all() and len(tabs) == 0 and blocks == 0
    for c in cut:
        info = jpeg.probe(lib, c)
        assert info["status"] == jpeg.NOT_HANDLED and info["reason"] == 8


def test_unpack_host_gives_the_same_coefficients(lib, files):
    whole, cut = [b for _, b, _ in files], [c for _, _, c in files]
    wc, wd = entropy(lib, whole)
    data, desc, sc, tabs, blocks = scan(lib, cut, std_tables=True)
    assert (desc["status"] == jpeg.OK).all() and len(tabs) == 4  # the four tables of annex K, once for the batch
    gc, status = jpeg.unpack_host(lib, data, sc, tabs, desc, blocks)
    assert (status == jpeg.OK).all()
    np.testing.assert_array_equal(desc["coef_block"], wd["coef_block"])
    np.testing.assert_array_equal(gc, wc[:blocks])


def test_a_file_that_defines_some_tables_gets_only_the_omitted_ones(lib):
    blob = jpeg_file(50, 38, 7, 2)
    # its DC table 0, restated with the symbols 10 and 11 swapped: categories no 8-bit picture of this size reaches, so the
    # coefficients are the same -- and the table is recognisably the file's own
    (a, b), = [(a, b) for m, a, b in segments(blob) if m == 0xC4 and blob[a + 4] == 0x00]
    seg = bytearray(blob[a:b])
    assert seg[5 + 16 + 10] == 10 and seg[5 + 16 + 11] == 11
    seg[5 + 16 + 10], seg[5 + 16 + 11] = 11, 10
    own = cut_dht(blob[:a] + bytes(seg) + blob[b:], keep=(0x00,))
    wc, wd = entropy(lib, [blob])
    gc, gd = entropy(lib, [own], std_tables=True)
    assert gd["status"][0] == jpeg.OK
    np.testing.assert_array_equal(gc, wc)
    _, d, sc, tabs, _ = scan(lib, [own], std_tables=True)
    assert d["status"][0] == jpeg.OK
    dc0 = tabs[sc["dc"][0][0]]
    assert list(dc0["vals"][10:12]) == [11, 10]                       # the file's table, not the standard's
    std = scan(lib, [cut_dht(blob)], std_tables=True)
    assert list(std[3][std[2]["dc"][0][0]]["vals"][10:12]) == [10, 11]  # ... which an omitted table 0 is
    # ids 2 and 3 have no standard table: a scan that names table 2 and no DHT stays refused
    sos = [(a, b) for m, a, b in segments(own) if m == 0xDA][0][0]
    bad = bytearray(own)
    bad[sos + 4 + 1 + 1] = 0x22
    assert entropy(lib, [bytes(bad)], std_tables=True)[1]["reason"][0] == 8
    # and an unknown flag bit is an error of the call
    desc = np.zeros(1, dtype=jpeg.DESC)
    rc = lib.avcer_jpeg_entropy_batch_ex(None, None, None, 0, None, 0, desc.ctypes.data_as(ctypes.c_void_p), 1, 2, None)
    assert rc != 0


# ---------------------------------------------------------------------------------------------------- the container
def blobs_of(n, w=16, h=16, quality=50):
    return [jpeg_file(w, h, 900 + k, 2, quality=quality) for k in range(n)]


def pcm_of(n, ch, seed=3):
    p = np.random.default_rng(seed).integers(-20000, 20000, (n, ch)).astype(np.int16)
    return p[:, 0] if ch == 1 else p


def opened(tmp_path, data, name="clip.avi"):
    path = tmp_path / name
    path.write_bytes(data)
    return avi.open_avi(path)


def same_frames(a, blobs):
    return a.n_frames == len(blobs) and all(bytes(f) == b for f, b in zip(a.frames, blobs))


@pytest.mark.parametrize("index", [True, False])
@pytest.mark.parametrize("ch", [1, 2])
def test_round_trip(tmp_path, index, ch):
    blobs = blobs_of(5)
    blobs[1] += b"\0" * (len(blobs[1]) & 1)                           # an even-length frame
    blobs[2] += b"\0" * (1 - (len(blobs[2]) & 1))                     # ... beside an odd one: padding
    pcm = pcm_of(7351, ch)
    path = avi.write_avi(tmp_path / "rt.avi", blobs, 25, pcm=pcm, audio_rate=44100, index=index)
    raw = (tmp_path / "rt.avi").read_bytes()
    assert (b"idx1" in raw) == index
    with avi.open_avi(path) as a:
        assert (a.width, a.height, a.rate, a.scale, a.fps, a.n_frames) == (16, 16, 25, 1, 25.0, 5)
        assert (a.audio_rate, a.audio_channels) == (44100, ch) and a.pcm.dtype == np.int16 and a.pcm.shape == (7351, ch)
        assert same_frames(a, blobs) and all(isinstance(f, memoryview) for f in a.frames)
        np.testing.assert_array_equal(a.pcm, pcm.reshape(7351, ch))
    # no audio stream
    with avi.open_avi(avi.write_avi(tmp_path / "mute.avi", blobs, 25)) as a:
        assert a.pcm is None and a.audio_rate is None and a.audio_channels is None and same_frames(a, blobs)


def test_odd_frames_junk_info_and_swapped_streams(tmp_path):
    blobs = [b + b"\0" * (1 - (len(b) & 1)) for b in blobs_of(4)]     # every frame of odd length
    assert all(len(b) & 1 for b in blobs)
    pcm = pcm_of(4000, 2)
    junk = avi._chunk(b"JUNK", b"\x55" * 13)
    info = avi._list(b"INFO", avi._chunk(b"ISFT", b"some muxer\0"))
    rec = avi._list(b"rec ", avi._chunk(b"09xx", b"abc"))              # an unknown stream inside a rec list
    vprp = avi._chunk(b"vprp", b"\0" * 68) + avi._chunk(b"JUNK", b"\0" * 6) + avi._chunk(b"strn", b"name\0")
    for audio_first in (False, True):
        data = avi.build_avi(blobs, 30000, 1001, pcm, 48000, True, audio_first=audio_first,
                             movi_extra=[(0, junk), (2, info), (2, junk), (3, rec), (4, junk)], strl_extra=vprp)
        assert (b"01dc" in data) == audio_first and (b"00wb" in data) == audio_first
        with opened(tmp_path, data, f"x{int(audio_first)}.avi") as a:
            assert same_frames(a, blobs) and (a.rate, a.scale) == (30000, 1001) and a.audio_rate == 48000
            assert abs(a.fps - 29.97002997) < 1e-6 and int(a.rate / a.scale) == 29
            np.testing.assert_array_equal(a.pcm, pcm)


def test_a_zero_length_chunk_repeats_its_predecessor(tmp_path):
    blobs = blobs_of(3)
    with opened(tmp_path, avi.build_avi([blobs[0], b"", blobs[1], b"", b"", blobs[2]], 25, pcm=pcm_of(2000, 2))) as a:
        assert same_frames(a, [blobs[0], blobs[0], blobs[1], blobs[1], blobs[1], blobs[2]])
    with pytest.raises(ValueError, match="first video chunk is empty"):
        opened(tmp_path, avi.build_avi([b"", blobs[0]], 25))


def patched(data, at, new):
    return data[:at] + new + data[at + len(new):]


def test_every_refusal_names_the_file_and_the_reason(tmp_path):
    blobs, pcm = blobs_of(3), pcm_of(3000, 2)
    vprp = avi._chunk(b"vprp", b"\0" * 68)
    good = avi.build_avi(blobs, 25, pcm=pcm, strl_extra=vprp, movi_extra=[(1, avi._chunk(b"JUNK", b"\0" * 8))])
    with opened(tmp_path, good) as a:
        assert same_frames(a, blobs)
    with opened(tmp_path, good.replace(b"vidsMJPG", b"vidsmjpg").replace(b"MJPG", b"mJpG")) as a:  # any letter case
        assert same_frames(a, blobs)
    strh_v, strh_a = good.index(b"vidsMJPG"), good.index(b"auds")
    comp = good.index(b"MJPG", strh_v + 8)
    wave = good.index(b"strf", strh_a) + 8
    first = good.index(b"00dc")
    cases = {
        "not a RIFF AVI": patched(good, 0, b"RIFX"),
        "not a RIFF AVI file": patched(good, 8, b"WAVE"),
        "video handler": patched(good, strh_v + 4, b"H264"),
        "biCompression": patched(good, comp, b"XVID"),
        "audio format tag 85": patched(good, wave, struct.pack("<H", 0x55)),
        "with 8 bits": patched(good, wave + 14, struct.pack("<H", 8)),
        "2 video streams": patched(good, strh_a, b"vids"),
        "AVIX": good + avi._list(b"AVIX", avi._list(b"movi", b""), b"RIFF"),
        "indx chunk": good.replace(b"vprp", b"indx"),
        "ix## index": good.replace(b"JUNK", b"ix00"),
        "runs past the end": patched(good, first + 4, struct.pack("<I", len(good))),
        "no movi list": good.replace(b"movi", b"movx"),
        "RIFF form .* runs past the end": good[:-10],
        "no video stream": patched(good, strh_v, b"txts"),
    }
    for reason, data in cases.items():
        with pytest.raises(ValueError, match=reason) as e:
            opened(tmp_path, data, "bad.avi")
        assert "bad.avi" in str(e.value), reason
    (tmp_path / "empty.avi").write_bytes(b"")
    with pytest.raises(ValueError, match="empty.avi"):
        avi.open_avi(tmp_path / "empty.avi")


def test_a_truncated_file_raises_valueerror_or_reads_what_is_whole(tmp_path):
    blobs = blobs_of(3)
    good = avi.build_avi(blobs, 25, pcm=pcm_of(300, 2), movi_extra=[(1, avi._chunk(b"JUNK", b"\0" * 7))],
                         strl_extra=avi._chunk(b"vprp", b"\0" * 20))
    assert len(good) < 8192
    path = tmp_path / "cut.avi"
    read = refused = 0
    for n in range(len(good)):                                        # every chunk boundary and every byte between them
        # as it is cut, and with the RIFF size set to what is left -- so that the walk inside is what meets the cut
        for data in (good[:n], (good[:4] + struct.pack("<I", max(n - 8, 0)) + good[8:n]) if n >= 8 else None):
            if data is None:
                continue
            path.write_bytes(data)
            try:
                a = avi.open_avi(path)
            except ValueError as e:
                assert "cut.avi" in str(e)
                refused += 1
                continue
            with a:                                                   # what it reads is whole frames of the good file, in order
                assert a.n_frames <= 3 and all(bytes(f) == b for f, b in zip(a.frames, blobs))
                assert a.pcm is None or a.pcm.shape[1] == 2
            read += 1
    assert refused > len(good) and read > 0                           # (cuts at list ends with a fitting RIFF size are whole files)


def test_jpeg_size_and_the_writer_refuse_what_they_cannot_state():
    assert avi.jpeg_size(jpeg_file(50, 38, 1, 2)) == (50, 38)
    assert avi.jpeg_size(jpeg_file(33, 17, 1, None, progressive=True)) == (33, 17)
    with pytest.raises(ValueError):
        avi.jpeg_size(b"not a jpeg")
    with pytest.raises(ValueError):
        avi.build_avi([], 25)
    with pytest.raises(ValueError):
        avi.build_avi(blobs_of(1), 0)
    with pytest.raises(ValueError):
        avi.build_avi(blobs_of(1), 25, pcm=np.zeros(10, dtype=np.float32))
