"""Uncompressed BGR video on the host: dib.unpack_numpy against PIL's BMP reader (a DIB frame behind a BITMAPFILEHEADER and a
BITMAPINFOHEADER is a BMP file), tolerance zero; the raw AVI container through build_avi_raw -> open_avi; what is refused, by name.
No device."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

from avcer_amd import avi, dib
from test_avi_cpu import blobs_of, patched, pcm_of

WIDTHS, HEIGHTS = (1, 2, 3, 5, 16, 17, 22), (1, 3)


def bmp_file(chunk, w, h, bits, bottom_up):
    info = struct.pack("<IiiHHIIiiII", 40, w, h if bottom_up else -h, 1, bits, 0, len(chunk), 0, 0, 0, 0)
    return b"BM" + struct.pack("<IHHI", 14 + 40 + len(chunk), 0, 0, 14 + 40) + info + bytes(chunk)


def test_pil_reads_32_bit_bi_rgb_as_bgrx():
    """The premise of the 32-bit claim: PIL takes bytes 0, 1, 2 of a pixel as B, G, R and drops byte 3."""
    img = Image.open(io.BytesIO(bmp_file(bytes([10, 20, 30, 99]), 1, 1, 32, True)))
    assert np.asarray(img.convert("RGB")).tolist() == [[[30, 20, 10]]]


@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("bottom_up", [True, False])
def test_unpack_numpy_is_pils_bmp_reader(bits, bottom_up):
    rng = np.random.default_rng(bits + bottom_up)
    for w in WIDTHS:
        for h in HEIGHTS:
            size = dib.stride_of(w, bits) * h
            chunks = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(2)]   # random padding and fourth bytes too
            want = np.stack([np.asarray(Image.open(io.BytesIO(bmp_file(c, w, h, bits, bottom_up))).convert("RGB")) for c in chunks])
            for bgr in (True, False):
                got = dib.unpack_numpy(chunks, h, w, bits, bottom_up, bgr=bgr)
                assert got.dtype == np.uint8 and got.shape == (2, h, w, 3)
                np.testing.assert_array_equal(got, want[..., ::-1] if bgr else want, err_msg=f"{w} x {h} bgr={bgr}")
    assert dib.stride_of(5, 24) == 16 and dib.stride_of(5, 32) == 20 and dib.stride_of(1, 24) == 4
    with pytest.raises(ValueError, match="frame 1"):
        dib.unpack_numpy([bytes(8), bytes(7)], 2, 1, 24, True)
    with pytest.raises(ValueError, match="16 bits"):
        dib.unpack_numpy([bytes(8)], 2, 1, 16, True)


def frames_of(n, h, w, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("bits,bottom_up", [(24, True), (24, False), (32, True), (32, False)])
def test_the_raw_container_round_trip(tmp_path, bits, bottom_up):
    frames, pcm = frames_of(4, 5, 7), pcm_of(4 * 1764, 2)
    path = avi.write_avi_raw(tmp_path / "raw.avi", [frames[0], None, frames[1], frames[2], frames[3]], 25, pcm=pcm, bits=bits, bottom_up=bottom_up)
    assert (tmp_path / "raw.avi").read_bytes() == avi.build_avi_raw([frames[0], None, frames[1], frames[2], frames[3]], 25, pcm=pcm, bits=bits,
                                                                    bottom_up=bottom_up)
    with avi.open_avi(path) as a:
        assert (a.codec, a.bits, a.bottom_up, a.width, a.height, a.n_frames, a.rate, a.scale) == ("DIB", bits, bottom_up, 7, 5, 5, 25, 1)
        assert all(len(f) == dib.stride_of(7, bits) * 5 for f in a.frames)
        chunks, _, _ = avi.raw_chunks(frames, bits, bottom_up)
        assert [bytes(f) for f in a.frames] == [chunks[0], chunks[0], chunks[1], chunks[2], chunks[3]]   # the empty chunk repeats
        np.testing.assert_array_equal(dib.unpack_numpy(a.frames, 5, 7, bits, bottom_up), frames[[0, 0, 1, 2, 3]])
        np.testing.assert_array_equal(a.pcm, pcm)
    # and in OpenDML segments (a frame is 120 or 140 bytes)
    data = avi.build_avi_raw(frames, 25, pcm=pcm, audio_rate=2000, bits=bits, bottom_up=bottom_up, opendml=True, segment_bytes=1500, index_segments=8)
    assert data.count(b"AVIX") >= 2
    (tmp_path / "odml.avi").write_bytes(data)
    with avi.open_avi(tmp_path / "odml.avi", opendml=True) as a:
        np.testing.assert_array_equal(dib.unpack_numpy(a.frames, 5, 7, a.bits, a.bottom_up), frames)
        np.testing.assert_array_equal(a.pcm, pcm)
    with avi.open_avi(avi.write_avi(tmp_path / "mjpg.avi", blobs_of(2), 25)) as a:              # a Motion-JPEG file says so
        assert (a.codec, a.bits, a.bottom_up) == ("MJPG", 24, False)


def test_what_is_refused_is_refused_by_name(tmp_path):
    frames = frames_of(3, 4, 6)
    good = avi.build_avi_raw(frames, 25, pcm=pcm_of(300, 2))
    strh = good.index(b"vidsDIB ")
    strf = good.index(b"strf", strh) + 8
    first = good.index(b"00dc")
    size = dib.stride_of(6, 24) * 4
    assert struct.unpack_from("<I", good, first + 4)[0] == size
    short = good[:first + 4] + struct.pack("<I", size - 2) + good[first + 8:first + 8 + size - 2] + good[first + 8 + size:]
    short = short[:4] + struct.pack("<I", len(short) - 8) + short[8:]
    movi = short.index(b"movi") - 4
    short = short[:movi] + struct.pack("<I", struct.unpack_from("<I", good, movi)[0] - 2) + short[movi + 4:]
    cases = {
        "16 bits a pixel": patched(good, strf + 14, struct.pack("<H", 16)),
        "8 bits a pixel .palettised": patched(good, strf + 14, struct.pack("<H", 8)),
        "YUY2.*YUV": patched(good, strf + 16, b"YUY2"),
        "I420.*YUV": patched(good, strf + 16, b"I420"),
        "BI_BITFIELDS": patched(good, strf + 16, struct.pack("<I", 3)),
        "BI_RLE8": patched(good, strf + 16, struct.pack("<I", 1)),
        "video frame 0: a chunk of 78 bytes": short,
        "video handler b'MJPG' beside biCompression 0": patched(good, strh + 4, b"MJPG"),
        # today's messages for what was refused before
        "video biCompression b'XVID': only MJPG": patched(good, strf + 16, b"XVID"),
        "video biCompression b'H264': only MJPG": patched(good, strf + 16, b"H264"),
    }
    for reason, data in cases.items():
        path = tmp_path / "bad.avi"
        path.write_bytes(data)
        with pytest.raises(ValueError, match=reason) as e:
            avi.open_avi(path)
        assert "bad.avi" in str(e.value), reason
    for handler in (b"RGB ", b"RAW ", b"dib ", b"\0\0\0\0"):                                     # the handlers a raw stream may name
        path = tmp_path / "ok.avi"
        path.write_bytes(patched(good, strh + 4, handler))
        with avi.open_avi(path) as a:
            assert a.codec == "DIB" and a.n_frames == 3
    mjpg = avi.build_avi(blobs_of(2), 25)
    path = tmp_path / "h264.avi"
    path.write_bytes(patched(mjpg, mjpg.index(b"vidsMJPG") + 4, b"H264"))
    with pytest.raises(ValueError, match="video handler b'H264': only MJPG"):
        avi.open_avi(path)
    with pytest.raises(ValueError, match="frame 1"):
        avi.build_avi_raw([frames[0], frames[1][:, :5]], 25)
