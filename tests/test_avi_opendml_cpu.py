"""OpenDML AVI files on the host (avcer_amd/avi.py): open_avi(opendml=True) reads what build_avi / AviWriter(opendml=True) write
and returns the frames and sound of the plain file; a reader written here from the OpenDML 1.02 struct layouts checks every index
the writer leaves; a sparse file past 4 GiB is walked; the refusals name the file.  No device."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from avcer_amd import avi
from test_avi_cpu import blobs_of, pcm_of

SEGMENT, CAPACITY, RATE, AUDIO_RATE = 4096, 16, 25, 8000


def inputs():
    """9 small frames, two of them empty (frames 3 and 6), 320 stereo samples a frame."""
    blobs = blobs_of(9)
    blobs[3] = blobs[6] = b""
    return blobs, pcm_of(9 * AUDIO_RATE // RATE + 77, 2)


def built(**kw):
    blobs, pcm = inputs()
    return avi.build_avi(blobs, RATE, pcm=pcm, audio_rate=AUDIO_RATE, opendml=True, segment_bytes=SEGMENT, index_segments=CAPACITY, **kw)


# ---------------------------------------------------------------------------------------------------- a reader of its own
def chunks(data, at, end):
    """[(fourcc, list type or None, data offset, size)] of data[at:end)."""
    out = []
    while at < end:
        cc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        out.append((cc, data[at + 8:at + 12] if cc in (b"LIST", b"RIFF") else None, at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end
    return out


def forms(data):
    """Per RIFF form: (type, offset of the header, size, {stream fourcc: [(data offset, size)]} of its movi walk, (movi fourcc offset,
    its chunks))."""
    out = []
    for cc, kind, at, size in chunks(data, 0, len(data)):
        assert cc == b"RIFF"
        movi = [c for c in chunks(data, at + 4, at + size) if c[1] == b"movi"]
        assert len(movi) == 1
        inner = chunks(data, movi[0][2] + 4, movi[0][2] + movi[0][3])
        walk = {}
        for c in inner:
            if c[0][:2].isdigit():
                walk.setdefault(c[0], []).append((c[2], c[3]))
        out.append((kind, at - 8, size, walk, (movi[0][2], inner)))
    return out


def test_every_index_the_writer_leaves_is_right():
    data = built()
    fs = forms(data)
    assert len(fs) >= 3 and [f[0] for f in fs] == [b"AVI "] + [b"AVIX"] * (len(fs) - 1)
    biggest = max(size for f in fs for rows in f[3].values() for _, size in rows) + 8 + 1   # the largest chunk of the file
    for kind, at, size, walk, _ in fs:
        assert size % 2 == 0 and 8 + size < SEGMENT + biggest
    # an empty frame first in its segment
    firsts = [f[3][b"00dc"][0][1] for f in fs if b"00dc" in f[3]]
    assert 0 in firsts[1:]
    # the header: avih, the super indexes, dmlh
    head = {c[1] if c[0] == b"LIST" else c[0]: c for c in chunks(data, 12, 8 + fs[0][2])}
    hdrl = chunks(data, head[b"hdrl"][2] + 4, head[b"hdrl"][2] + head[b"hdrl"][3])
    avih = next(c for c in hdrl if c[0] == b"avih")
    assert struct.unpack_from("<I", data, avih[2] + 16)[0] == len(fs[0][3][b"00dc"])          # dwTotalFrames: the first segment
    odml = next(c for c in hdrl if c[1] == b"odml")
    dmlh, = chunks(data, odml[2] + 4, odml[2] + odml[3])
    assert dmlh[0] == b"dmlh" and struct.unpack_from("<I", data, dmlh[2])[0] == 9
    strls = [c for c in hdrl if c[1] == b"strl"]
    assert len(strls) == 2
    for strl, stream, per_tick in zip(strls, (b"00dc", b"01wb"), (None, 4)):
        indx = next(c for c in chunks(data, strl[2] + 4, strl[2] + strl[3]) if c[0] == b"indx")
        longs, sub, typ, used, cc, r0, r1, r2 = struct.unpack_from("<HBBI4sIII", data, indx[2])
        assert (longs, sub, typ, cc, r0, r1, r2) == (4, 0, 0, stream, 0, 0, 0) and used == len(fs) and indx[3] == 24 + 16 * CAPACITY
        assert data[indx[2] + 24 + 16 * used:indx[2] + indx[3]] == b"\0" * (16 * (CAPACITY - used))
        for k in range(used):
            off, size, duration = struct.unpack_from("<QII", data, indx[2] + 24 + 16 * k)
            kind, at, fsize, walk, (movi, inner) = fs[k]
            assert at < off < at + 8 + fsize                                                  # inside segment k
            assert data[off:off + 4] == b"ix" + stream[:2] and struct.unpack_from("<I", data, off + 4)[0] == size - 8
            mine = walk.get(stream, [])
            assert duration == (len(mine) if per_tick is None else sum(s for _, s in mine) // per_tick)
            # the standard index behind it
            longs, sub, typ, n, cc, base, r = struct.unpack_from("<HBBI4sQI", data, off + 8)
            assert (longs, sub, typ, cc, r) == (2, 0, 1, stream, 0) and n == len(mine) and size == 8 + 24 + 8 * n
            for j, (where, length) in enumerate(mine):
                o, s = struct.unpack_from("<II", data, off + 32 + 8 * j)
                assert base + o == where and data[base + o - 8:base + o - 4] == stream
                assert struct.unpack_from("<I", data, base + o - 4)[0] == s & 0x7FFFFFFF == length
                assert bool(s >> 31) == (length == 0)                                         # not a key frame: a repeated empty chunk
            # the ix## chunks close the movi list, one per stream, in stream order
            assert [c[0] for c in inner[-2:]] == [b"ix00", b"ix01"]
    # idx1: the first segment alone
    idx1 = head[b"idx1"]
    first = sorted((where, cc, size) for cc, rows in fs[0][3].items() for where, size in rows)
    assert idx1[3] == 16 * len(first)
    for k, (where, cc, size) in enumerate(first):
        c, flags, off, s = struct.unpack_from("<4sIII", data, idx1[2] + 16 * k)
        assert (c, s) == (cc, size) and fs[0][4][0] + off + 8 == where and flags == (0x10 if size else 0)


def test_round_trip_and_the_default_still_refuses(tmp_path):
    blobs, pcm = inputs()
    (tmp_path / "odml.avi").write_bytes(built())
    avi.write_avi(tmp_path / "plain.avi", blobs, RATE, pcm=pcm, audio_rate=AUDIO_RATE)
    with avi.open_avi(tmp_path / "odml.avi", opendml=True) as a, avi.open_avi(tmp_path / "plain.avi") as b:
        assert a.n_frames == b.n_frames == 9 and [bytes(f) for f in a.frames] == [bytes(f) for f in b.frames]
        assert bytes(a.frames[3]) == blobs[2] and bytes(a.frames[6]) == blobs[5]               # repeated across a segment boundary too
        np.testing.assert_array_equal(a.pcm, b.pcm)
        np.testing.assert_array_equal(a.pcm, pcm)
        assert (a.width, a.height, a.rate, a.scale, a.audio_rate, a.codec) == (b.width, b.height, b.rate, b.scale, b.audio_rate, "MJPG")
    with avi.open_avi(tmp_path / "plain.avi", opendml=True) as b:                              # a plain file under the flag
        assert b.n_frames == 9
    with pytest.raises(ValueError, match="AVIX") as e:
        avi.open_avi(tmp_path / "odml.avi")
    assert "odml.avi" in str(e.value)
    one = avi.build_avi(blobs, RATE, pcm=pcm, audio_rate=AUDIO_RATE, opendml=True, segment_bytes=1 << 20, index_segments=CAPACITY)
    assert one.count(b"AVIX") == 0                                                             # one segment: the indx chunk is what is refused
    (tmp_path / "one.avi").write_bytes(one)
    with pytest.raises(ValueError, match="indx chunk"):
        avi.open_avi(tmp_path / "one.avi")
    with avi.open_avi(tmp_path / "one.avi", opendml=True) as a:
        assert a.n_frames == 9


def test_the_writer_in_pieces_gives_the_same_bytes(tmp_path):
    blobs, pcm = inputs()
    want = built()
    with avi.AviWriter(tmp_path / "w.avi", 16, 16, RATE, audio_rate=AUDIO_RATE, pcm=pcm, opendml=True, segment_bytes=SEGMENT,
                       index_segments=CAPACITY) as w:
        w.add_frames(blobs[:2]).add_frames(blobs[2:7]).add_frames(blobs[7:])
    assert (tmp_path / "w.avi").read_bytes() == want
    avi.write_avi(tmp_path / "w2.avi", blobs, RATE, pcm=pcm, audio_rate=AUDIO_RATE, opendml=True, segment_bytes=SEGMENT, index_segments=CAPACITY)
    assert (tmp_path / "w2.avi").read_bytes() == want
    # opendml=False: today's bytes
    with avi.AviWriter(tmp_path / "p.avi", 16, 16, RATE, audio_rate=AUDIO_RATE, pcm=pcm, opendml=False, segment_bytes=SEGMENT) as w:
        w.add_frames(blobs)
    plain = (tmp_path / "p.avi").read_bytes()
    assert plain == avi.build_avi(blobs, RATE, pcm=pcm, audio_rate=AUDIO_RATE) and b"AVIX" not in plain and b"indx" not in plain
    # one segment more than the super indexes hold
    n = want.count(b"AVIX") + 1
    path = tmp_path / "many.avi"
    with pytest.raises(OSError, match=f"index_segments = {n - 1}"):
        with avi.AviWriter(path, 16, 16, RATE, audio_rate=AUDIO_RATE, pcm=pcm, opendml=True, segment_bytes=SEGMENT, index_segments=n - 1) as w:
            w.add_frames(blobs)
    assert not path.exists()
    with avi.AviWriter(path, 16, 16, RATE, audio_rate=AUDIO_RATE, pcm=pcm, opendml=True, segment_bytes=SEGMENT, index_segments=n) as w:
        w.add_frames(blobs)
    assert path.read_bytes().count(b"AVIX") == n - 1


def test_a_file_past_4_gib(tmp_path):
    """A sparse file: the first segment, an AVIX form whose movi list holds one JUNK chunk of 4.2 GB and a real frame, and a second
    one with a smaller JUNK chunk and a real frame, which then lies behind byte 2^32.  (A RIFF size is 32 bits, so no single form or
    chunk can pass 4 GiB: the file does, and with it every offset the reader computes.)"""
    blobs = blobs_of(4)
    first = avi.build_avi(blobs[:2], RATE)
    path = tmp_path / "big.avi"
    try:
        with open(path, "wb") as f:
            f.write(first)
            for junk, blob in ((4_200_000_000, blobs[2]), (300_000_000, blobs[3])):
                tail = avi._chunk(b"00dc", blob)
                movi = 4 + 8 + junk + len(tail)
                f.write(b"RIFF" + struct.pack("<I", 4 + 8 + movi) + b"AVIX" + b"LIST" + struct.pack("<I", movi) + b"movi")
                f.write(b"JUNK" + struct.pack("<I", junk))
                f.seek(junk, os.SEEK_CUR)
                f.write(tail)
        sparse = os.stat(path).st_blocks * 512 < 1 << 28
    except OSError:
        sparse = False
    if not sparse:
        if path.exists():
            os.remove(path)
        pytest.skip("the filesystem of tmp_path has no sparse files")
    try:
        assert os.path.getsize(path) > 1 << 32
        with avi.open_avi(path, opendml=True) as a:
            assert a.n_frames == 4 and [bytes(f) for f in a.frames] == blobs
    finally:
        os.remove(path)


def test_refusals_with_the_flag_name_the_file(tmp_path):
    blobs = blobs_of(3)
    good = avi.build_avi(blobs, RATE, pcm=pcm_of(500, 2), opendml=True, segment_bytes=1500, index_segments=8)
    assert good.count(b"AVIX") >= 1
    last = good.rindex(b"RIFF")
    cases = {
        "trailing .*WAVE": good + avi._list(b"WAVE", avi._chunk(b"fmt ", b"\0" * 16), b"RIFF"),
        "trailing": good + avi._chunk(b"JUNK", b"\0" * 8),
        "AVIX form .* runs past the end": good[:-6],
        "has no movi list": good[:last] + avi._list(b"AVIX", avi._list(b"movx", b""), b"RIFF"),
        "runs past the end": good[:last + 24] + struct.pack("<4sI", b"00dc", 1 << 20) + good[last + 32:],
    }
    for reason, data in cases.items():
        path = tmp_path / "bad.avi"
        path.write_bytes(data)
        with pytest.raises(ValueError, match=reason) as e:
            avi.open_avi(path, opendml=True)
        assert "bad.avi" in str(e.value), reason


def test_ffmpeg_copies_a_writer_file_if_there_is_one(tmp_path):
    ffmpeg = shutil.which("ffmpeg")
    if ffmpeg is None:
        pytest.skip("no ffmpeg binary on this machine (an optional cross-check)")
    blobs, pcm = inputs()
    blobs = [b or blobs[0] for b in blobs]
    src, dst = tmp_path / "src.avi", tmp_path / "dst.avi"
    src.write_bytes(avi.build_avi(blobs, RATE, pcm=pcm, audio_rate=AUDIO_RATE, opendml=True, segment_bytes=SEGMENT, index_segments=CAPACITY))
    subprocess.run([ffmpeg, "-v", "error", "-y", "-i", str(src), "-c", "copy", str(dst)], check=True, timeout=60)
    with avi.open_avi(dst, opendml=True) as a:
        assert [bytes(f) for f in a.frames] == blobs
        np.testing.assert_array_equal(a.pcm, pcm)
