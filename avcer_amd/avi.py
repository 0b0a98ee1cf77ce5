"""Motion-JPEG or uncompressed-BGR / PCM AVI files read and written on the host: the container in front of `jpeg.decode_frames`
and `dib.unpack_frames` (no device but in AviFile.decode_frames, which picks between the two; no dependency beyond numpy).

What is read is the AVI that `ffmpeg -i clip.mp4 -c:v mjpeg -q:v 2 -c:a pcm_s16le -ar 44100 -ac 2 clip.avi` writes -- exactly as
`audio_pipeline.convert_mp4_to_mp3` reads "the WAV that ffmpeg writes": a RIFF `AVI ` form with a `hdrl` list (`avih`, one `strl`
list per stream holding `strh` and `strf`) and a `movi` list whose `NNdc` / `NNdb` chunks are baseline JPEG files, one per frame,
interleaved with the `NNwb` chunks of 16-bit PCM.  `open_avi` maps the file (mmap) and hands the frames out as memoryviews of the
mapping: no frame byte is copied on the way to the native header pass.

The same container with an uncompressed video stream -- `-c:v rawvideo -pix_fmt bgr24`: biCompression 0 (BI_RGB), 24 or 32 bits,
handler `DIB `, `RGB `, `RAW ` or none, rows padded to 4 bytes, bottom-up when biHeight > 0 -- is read too (AviFile.codec "DIB"; every
chunk is one frame of stride * height bytes, dib.py).  `open_avi(path, opendml=True)` reads OpenDML files: any number of RIFF `AVIX`
forms behind the first, every movi list walked in file order, the indexes (`indx`, `ix##`, LIST odml) skipped -- the walk is the
source of truth, as it is for idx1 -- and every offset a Python int over the mapping, so files past 4 GiB.

Everything else is refused with a ValueError that names the file and the reason, before any frame is touched: another codec
(palettised, 16-bit, BI_BITFIELDS, RLE and YUV streams by name), another audio format, a second video stream, OpenDML unless
`opendml=True` (`AVIX` segments, `indx` / `ix##` indexes), a trailing form that is no `AVIX`, an `AVIX` form cut short or without a
movi list, a chunk that runs past the end of the file, an uncompressed frame of the wrong length.  H.264 / MP4 is out of reach
without a codec library and is not pretended.

`write_avi` is the inverse (tests, tools/avi_bench.py, users who want the format); `AviWriter` is the same file written as the frames
come (the result video of a recording that is never whole in memory): chunks appended, the header sizes and `idx1` patched at
close.  Plain AVI below 4 GiB by default; `opendml=True` writes the OpenDML 1.02 layout instead (AviWriter's docstring), and
`write_avi_raw` / `build_avi_raw` write the uncompressed kind.
"""
from __future__ import annotations

import mmap
import os
import struct
from typing import Optional, Sequence

import numpy as np

WAVE_FORMAT_PCM = 1
AVIF_HASINDEX, AVIF_ISINTERLEAVED = 0x10, 0x100
AVIIF_KEYFRAME = 0x10


class AviFile:
    """An open Motion-JPEG AVI file (see `open_avi`).  `frames[i]` is a memoryview of the mapping and stays valid until `close()`
    (or the end of the `with` block); `pcm` is an array of its own."""

    def __init__(self, path, mapping, view, width, height, rate, scale, frames, audio_rate, audio_channels, pcm, codec="MJPG", bits=24,
                 bottom_up=False):
        self.path = path
        self.codec, self.bits, self.bottom_up = codec, int(bits), bool(bottom_up)
        self._map, self._view = mapping, view
        self.width, self.height = int(width), int(height)
        self.rate, self.scale = int(rate), int(scale)
        self.fps = self.rate / self.scale
        self.frames = frames
        self.n_frames = len(frames)
        self.audio_rate, self.audio_channels = audio_rate, audio_channels
        self.pcm = pcm

    def decode_frames(self, engine, lo: int = 0, hi: Optional[int] = None, bgr: bool = True, frames_per_pass: int = 64):
        """Frames [lo, hi) on the device, uint8 [hi - lo, height, width, 3] in BGR order (RGB with bgr=False): the ONE place that
        picks the decoder by `codec` -- jpeg.decode_frames for "MJPG", dib.unpack_frames for "DIB" -- for run_inference_file (in
        memory, streamed, and the result video's second sweep) and dataset.video_job_from_avi."""
        from . import dib, jpeg

        whole = lo == 0 and (hi is None or hi >= self.n_frames)
        part = self.frames if whole else self.frames[lo:hi]
        if self.codec == "MJPG":
            return jpeg.decode_frames(engine, part, self.height, self.width, bgr=bgr, frames_per_pass=frames_per_pass)[0]
        return dib.unpack_frames(engine, part, self.height, self.width, self.bits, self.bottom_up, bgr=bgr, frames_per_pass=frames_per_pass)

    def close(self):
        for f in self.frames:
            f.release()
        self.frames = []
        if self._view is not None:
            self._view.release()
            self._view = None
        if self._map is not None:
            self._map.close()
            self._map = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _walk(view, at, end, refuse):
    """The chunks of view[at:end): (fourcc, list type or None, first data byte, data length).  Chunks are padded to even length;
    a header or a body that runs past `end` is refused."""
    while at < end:
        if at + 8 > end:
            raise refuse(f"a chunk header at byte {at} runs past the end of its list")
        cc = bytes(view[at:at + 4])
        size = struct.unpack_from("<I", view, at + 4)[0]
        if at + 8 + size > end:
            raise refuse(f"chunk {cc!r} at byte {at} ({size} bytes) runs past the end of the file")
        kind = None
        if cc in (b"LIST", b"RIFF"):
            if size < 4:
                raise refuse(f"list at byte {at} has no type")
            kind = bytes(view[at + 8:at + 12])
        yield cc, kind, at + 8, size
        at += 8 + size + (size & 1)


# what an uncompressed stream's handler may be, and the YUV fourccs that are refused by name (their conversion to BGR is
# swscale's own arithmetic, which is neither stated nor checked here)
RAW_HANDLERS = (b"DIB ", b"RGB ", b"RAW ", b"\0\0\0\0")
YUV_FOURCCS = (b"YUY2", b"YUYV", b"UYVY", b"YVYU", b"I420", b"IYUV", b"YV12", b"NV12", b"NV21", b"Y800", b"Y422", b"YV16", b"Y42B", b"I444",
               b"Y41P", b"YVU9", b"HDYC", b"V210", b"AYUV", b"P010")
BI_NAMES = {1: "BI_RLE8", 2: "BI_RLE4", 3: "BI_BITFIELDS"}


def _parse(view, path, opendml=False):
    def refuse(reason):
        return ValueError(f"{path}: {reason}")

    n = len(view)
    if n < 12 or bytes(view[0:4]) != b"RIFF" or bytes(view[8:12]) != b"AVI ":
        raise refuse("not a RIFF AVI file")
    riff = struct.unpack_from("<I", view, 4)[0]
    if 8 + riff > n:
        raise refuse(f"the RIFF form ({riff} bytes) runs past the end of the file ({n} bytes)")
    end = 8 + riff
    if not opendml and end + (end & 1) + 12 <= n and bytes(view[end + (end & 1):end + (end & 1) + 4]) == b"RIFF":
        raise refuse("OpenDML file (a second RIFF segment, AVIX); only plain AVI up to 1 GiB is read")
    streams = []  # per strl, in file order: dict(type, handler, scale, rate, strf fields)
    movi = None
    for cc, kind, at, size in _walk(view, 12, end, refuse):
        if cc == b"LIST" and kind == b"hdrl":
            for cc2, kind2, at2, size2 in _walk(view, at + 4, at + size, refuse):
                if not (cc2 == b"LIST" and kind2 == b"strl"):
                    continue  # avih (not trusted: the movi walk counts the frames), JUNK, odml lists, ...
                s = {}
                for cc3, _, at3, size3 in _walk(view, at2 + 4, at2 + size2, refuse):
                    if cc3 == b"strh":
                        if size3 < 36:
                            raise refuse("a strh chunk of fewer than 36 bytes")
                        s["type"], s["handler"] = bytes(view[at3:at3 + 4]), bytes(view[at3 + 4:at3 + 8])
                        s["scale"], s["rate"] = struct.unpack_from("<II", view, at3 + 20)
                    elif cc3 == b"strf":
                        s["strf"] = (at3, size3)
                    elif cc3 == b"indx" and not opendml:
                        raise refuse("OpenDML file (an indx chunk); only plain AVI up to 1 GiB is read")
                    # vprp, strn, strd, JUNK, unknown: skipped
                if "type" not in s or "strf" not in s:
                    raise refuse("a stream list without strh or strf")
                streams.append(s)
        elif cc == b"LIST" and kind == b"movi" and movi is None:
            movi = (at + 4, at + size)
        # idx1 is optional and not trusted; JUNK, LIST INFO, unknown chunks: skipped
    video = [i for i, s in enumerate(streams) if s["type"] == b"vids"]
    audio = [i for i, s in enumerate(streams) if s["type"] == b"auds"]
    if not video:
        raise refuse("no video stream")
    if len(video) > 1:
        raise refuse(f"{len(video)} video streams; one is read")
    v = streams[video[0]]
    at, size = v["strf"]
    if size < 40:
        raise refuse("the video stream's strf is no BITMAPINFOHEADER")
    width, height = struct.unpack_from("<ii", view, at + 4)
    comp = bytes(view[at + 16:at + 20])
    depth = struct.unpack_from("<H", view, at + 14)[0]
    code = struct.unpack("<I", comp)[0]
    codec, frame_bytes = "MJPG", None
    if code == 0:  # BI_RGB: uncompressed
        if depth not in (24, 32):
            raise refuse(f"uncompressed video of {depth} bits a pixel ({'palettised' if depth <= 8 else 'a 16-bit format'}): only 24 and 32 bits "
                         "(BGR) are read")
        if v["handler"].upper() not in RAW_HANDLERS:
            raise refuse(f"video handler {v['handler']!r} beside biCompression 0 (BI_RGB): DIB, RGB, RAW or none is read")
        codec = "DIB"
    elif code in BI_NAMES:
        raise refuse(f"video biCompression {code} ({BI_NAMES[code]}): of the uncompressed formats only BI_RGB with 24 or 32 bits is read")
    elif comp.upper() in YUV_FOURCCS:
        raise refuse(f"video biCompression {comp!r}: a YUV format; of the uncompressed formats only BI_RGB with 24 or 32 bits (BGR) is read")
    elif comp.upper() != b"MJPG":
        raise refuse(f"video biCompression {comp!r}: only MJPG (Motion-JPEG) is read")
    elif v["handler"].upper() != b"MJPG":
        raise refuse(f"video handler {v['handler']!r}: only MJPG (Motion-JPEG) is read")
    if v["scale"] <= 0 or v["rate"] <= 0 or width <= 0 or height == 0:
        raise refuse(f"video stream of {width} x {height} at {v['rate']} / {v['scale']} frames per second")
    a_rate = a_ch = None
    if audio:
        a = streams[audio[0]]
        at, size = a["strf"]
        if size < 16:
            raise refuse("the audio stream's strf is no WAVEFORMAT")
        tag, a_ch, a_rate, _, _, bits = struct.unpack_from("<HHIIHH", view, at)
        if tag != WAVE_FORMAT_PCM or bits != 16:
            raise refuse(f"audio format tag {tag} with {bits} bits: only WAVE_FORMAT_PCM (1) with 16 bits is read")
        if a_ch < 1 or a_rate < 1:
            raise refuse(f"audio stream of {a_ch} channels at {a_rate} Hz")
    if movi is None:
        raise refuse("no movi list")
    if codec == "DIB":
        frame_bytes = ((width * (depth // 8) + 3) & ~3) * abs(height)
    movis = [movi]
    if opendml:
        # any number of RIFF AVIX forms behind the first: each holds a movi list, walked in file order like the first.  The indexes
        # (indx, ix##, the odml list) are skipped: the walk is the source of truth, as it is for idx1
        at = end + (end & 1)
        while at + 12 <= n:
            cc, kind = bytes(view[at:at + 4]), bytes(view[at + 8:at + 12])
            if cc != b"RIFF" or kind != b"AVIX":
                raise refuse(f"a trailing {cc!r} {kind!r} form at byte {at}: only RIFF AVIX segments follow the AVI form")
            size = struct.unpack_from("<I", view, at + 4)[0]
            if at + 8 + size > n:
                raise refuse(f"the AVIX form at byte {at} ({size} bytes) runs past the end of the file ({n} bytes)")
            found = None
            for cc2, kind2, at2, size2 in _walk(view, at + 12, at + 8 + size, refuse):
                if cc2 == b"LIST" and kind2 == b"movi" and found is None:
                    found = (at2 + 4, at2 + size2)
            if found is None:
                raise refuse(f"the AVIX form at byte {at} has no movi list")
            movis.append(found)
            at += 8 + size + (size & 1)
    # the movi walk is the source of truth: frames and PCM in file order (`rec ` lists hold chunks of their own)
    frames, sound = [], []

    def walk_movi(lo, hi, top=True):
        for cc, kind, at, size in _walk(view, lo, hi, refuse):
            if cc == b"LIST":
                if kind == b"rec " and top:  # (rec lists do not nest)
                    walk_movi(at + 4, at + size, False)
                continue  # LIST INFO, unknown lists
            if cc[:2] == b"ix":
                if opendml:
                    continue
                raise refuse("OpenDML file (an ix## index chunk in movi); only plain AVI up to 1 GiB is read")
            if not cc[:2].isdigit():
                continue  # JUNK, unknown
            stream, what = int(cc[:2]), cc[2:]
            if stream == video[0] and what in (b"dc", b"db"):
                if size == 0:  # a dropped frame: the previous one again
                    if not frames:
                        raise refuse("the first video chunk is empty (a dropped frame with no predecessor)")
                    frames.append(frames[-1])
                elif frame_bytes is not None and size != frame_bytes:
                    raise refuse(f"video frame {len(frames)}: a chunk of {size} bytes, an uncompressed frame of {width} x {abs(height)} at "
                                 f"{depth} bits is {frame_bytes} bytes")
                else:
                    frames.append((at, size))
            elif audio and stream == audio[0] and what == b"wb":
                sound.append((at, size))

    for span in movis:
        walk_movi(*span)
    return dict(width=width, height=abs(height), rate=v["rate"], scale=v["scale"], frames=frames, sound=sound, audio_rate=a_rate,
                audio_channels=a_ch, codec=codec, bits=depth if codec == "DIB" else 24, bottom_up=codec == "DIB" and height > 0)


def open_avi(path, opendml: bool = False) -> AviFile:
    """The Motion-JPEG or uncompressed-BGR AVI file `path` -> AviFile: codec ("MJPG": every frame is a JPEG file; "DIB": every frame
    is an uncompressed bitmap of `bits` = 24 or 32 bits a pixel, `bottom_up` when biHeight > 0; dib.py), width, height, rate, scale (the video stream's dwRate / dwScale), fps = rate /
    scale, n_frames, frames (one zero-copy memoryview per video chunk, in file order; an empty chunk repeats its predecessor),
    audio_rate, audio_channels and pcm (int16 [L, C]: the audio chunks joined, cut to whole sample frames; None, with both fields
    None, when there is no audio stream).  Stream numbers follow the order of the strl lists.  ValueError naming the file and
    the reason for anything outside that (the module's docstring), raised before a frame is looked at.
    opendml=True reads OpenDML files as well -- any number of RIFF AVIX segments behind the first form, every movi list walked in
    file order, the indx / ix## / odml indexes skipped, not trusted -- so files past 1 GiB (ffmpeg's switch) and past 4 GiB; False
    (the default) refuses them as ever."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        if os.fstat(f.fileno()).st_size == 0:
            raise ValueError(f"{path}: not a RIFF AVI file (empty)")
        mapping = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    view = memoryview(mapping)
    try:
        p = _parse(view, path, bool(opendml))
        frames = [view[at:at + size] for at, size in p["frames"]]
        pcm = None
        if p["audio_rate"] is not None:
            ch = p["audio_channels"]
            parts = [np.frombuffer(view[at:at + size], dtype=np.uint8) for at, size in p["sound"]]
            raw = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
            whole = raw.size // (2 * ch) * (2 * ch)
            pcm = raw[:whole].copy().view("<i2").reshape(-1, ch)
            del parts, raw
    except BaseException:
        view.release()
        mapping.close()
        raise
    return AviFile(path, mapping, view, p["width"], p["height"], p["rate"], p["scale"], frames, p["audio_rate"], p["audio_channels"], pcm,
                   p["codec"], p["bits"], p["bottom_up"])


# ---------------------------------------------------------------------------------------------------- writing
def jpeg_size(blob) -> tuple:
    """(width, height) of a JPEG file from its frame header (SOF0 .. SOF15 but DHT / JPG / DAC); ValueError when there is none."""
    b = bytes(blob[:65536]) if len(blob) > 65536 else bytes(blob)
    p = 2
    if b[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file (no SOI)")
    while p + 4 <= len(b):
        if b[p] != 0xFF:
            break
        m = b[p + 1]
        if m == 0xFF:
            p += 1
            continue
        length = (b[p + 2] << 8) | b[p + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if p + 9 > len(b):
                break
            return (b[p + 7] << 8) | b[p + 8], (b[p + 5] << 8) | b[p + 6]
        p += 2 + length
    raise ValueError("no frame header in the JPEG file")


def _chunk(cc: bytes, body: bytes) -> bytes:
    return cc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _list(kind: bytes, body: bytes, cc: bytes = b"LIST") -> bytes:
    return cc + struct.pack("<I", 4 + len(body)) + kind + body


def build_avi(jpeg_blobs: Sequence, rate: int, scale: int = 1, pcm: Optional[np.ndarray] = None, audio_rate: int = 44100,
              index: bool = True, audio_first: bool = False, movi_extra: Sequence = (), strl_extra: bytes = b"", opendml: bool = False,
              segment_bytes: int = 1 << 30, index_segments: int = 256) -> bytes:
    """The bytes `write_avi` writes (with `opendml`, `segment_bytes`, `index_segments`: the OpenDML file, AviWriter's docstring; the
    reader's options below do not combine with it).  Two options beyond it, for tests of the reader: `audio_first` puts the audio stream's strl in
    front of the video's (audio is then stream 00, video 01); `movi_extra` = [(k, raw bytes)], raw chunks or lists placed in movi
    in front of frame k's chunk (k = the frame count: at the end); `strl_extra`: raw chunks behind the video stream's strf (vprp,
    JUNK, ...)."""
    blobs = [bytes(b) for b in jpeg_blobs]
    first = next((b for b in blobs if b), None)
    if first is None:
        raise ValueError("write_avi: no frame")
    rate, scale = int(rate), int(scale)
    if rate <= 0 or scale <= 0:
        raise ValueError("write_avi: rate and scale positive")
    width, height = jpeg_size(first)
    if opendml:
        if audio_first or movi_extra or strl_extra or not index:
            raise ValueError("build_avi: audio_first, movi_extra, strl_extra and index=False are options of the plain file")
        return _in_memory(blobs, width, height, rate, scale, pcm, audio_rate, opendml=True, segment_bytes=segment_bytes,
                          index_segments=index_segments)
    n = len(blobs)
    if pcm is not None:
        pcm = _as_pcm(pcm)
    vs, as_ = (1, 0) if (audio_first and pcm is not None) else (0, 1)
    vid, aud = b"%02ddc" % vs, b"%02dwb" % as_
    movi, entries = [b"movi"], []
    at = 4  # idx1 offsets count from the 'movi' fourcc
    extra = {}
    for k, raw in movi_extra:
        extra.setdefault(int(k), []).append(bytes(raw))

    def put(cc, body, flags=AVIIF_KEYFRAME):
        nonlocal at
        c = _chunk(cc, body)
        entries.append(cc + struct.pack("<III", flags, at, len(body)))
        movi.append(c)
        at += len(c)

    for k in range(n + 1):
        for raw in extra.get(k, ()):
            movi.append(raw)
            at += len(raw)
        if k == n:
            break
        put(vid, blobs[k], AVIIF_KEYFRAME if blobs[k] else 0)
        if pcm is not None:  # the samples of about this frame's duration; the last frame takes what is left
            lo = min(len(pcm), k * audio_rate * scale // rate)
            hi = len(pcm) if k == n - 1 else min(len(pcm), (k + 1) * audio_rate * scale // rate)
            if hi > lo:
                put(aud, pcm[lo:hi].tobytes())
    movi_body = b"".join(movi)
    biggest = max(len(b) for b in blobs)
    hdrl = _hdrl(n, biggest, width, height, rate, scale, None if pcm is None else (len(pcm), pcm.shape[1]), audio_rate, index,
                 audio_first=vs == 1, strl_extra=bytes(strl_extra))
    body = hdrl + b"LIST" + struct.pack("<I", len(movi_body)) + movi_body
    if len(movi_body) & 1:
        body += b"\0"
    if index:
        body += _chunk(b"idx1", b"".join(entries))
    if len(body) + 4 >= 1 << 30:
        raise ValueError("write_avi: more than 1 GiB; OpenDML is not written")
    return _list(b"AVI ", body, b"RIFF")


def _super_index(cc: bytes, entries, capacity: int) -> bytes:
    """An OpenDML `indx` chunk, index of indexes, of fixed capacity: entries = [(file offset of an ix## chunk's header, its size with
    the header, its duration in stream ticks)]."""
    body = struct.pack("<HBBI4sIII", 4, 0, 0, len(entries), cc, 0, 0, 0) + b"".join(struct.pack("<QII", *e) for e in entries)
    return _chunk(b"indx", body + b"\0" * (16 * (capacity - len(entries))))


def _hdrl(n: int, biggest: int, width: int, height: int, rate: int, scale: int, sound, audio_rate: int, index: bool,
          audio_first: bool = False, strl_extra: bytes = b"", video=None, odml=None) -> bytes:
    """The `hdrl` list of a file of `n` frames, the largest of `biggest` bytes; `sound` = (sample frames, channels) or None.  Its
    length does not depend on `n`, `biggest` or the sample count: AviWriter writes it once with zeros and once more at close.
    `video` = (handler, biCompression, bits, biHeight, biSizeImage) of another video format than Motion-JPEG.  `odml` = (frames of
    the first segment, capacity, the video stream's super-index entries, the audio stream's): the OpenDML header -- an `indx`
    chunk of `capacity` entries in each stream list, avih counts the first segment, LIST odml / dmlh the file."""
    handler, comp, bits, bi_height, image = video if video is not None else (b"MJPG", b"MJPG", 24, height, width * height * 3)
    strl_v = _list(b"strl", _chunk(b"strh", struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", handler, 0, 0, 0, 0, scale, rate, 0, n, biggest,
                                                        0xFFFFFFFF, 0, 0, 0, width, height)) +
                   _chunk(b"strf", struct.pack("<IiiHH4sIiiII", 40, width, bi_height, 1, bits, comp, image, 0, 0, 0, 0)) + strl_extra +
                   (b"" if odml is None else _super_index(b"00dc", odml[2], odml[1])))
    lists = [strl_v]
    if sound is not None:
        length, ch = sound
        strl_a = _list(b"strl", _chunk(b"strh", struct.pack("<4s4sIHHIIIIIIIIhhhh", b"auds", b"\1\0\0\0", 0, 0, 0, 0, 1, audio_rate, 0, length,
                                                            0, 0xFFFFFFFF, 2 * ch, 0, 0, 0, 0)) +
                       _chunk(b"strf", struct.pack("<HHIIHH", WAVE_FORMAT_PCM, ch, audio_rate, audio_rate * 2 * ch, 2 * ch, 16)) +
                       (b"" if odml is None else _super_index(b"01wb", odml[3], odml[1])))
        lists = [strl_a, strl_v] if audio_first else [strl_v, strl_a]
    avih = _chunk(b"avih", struct.pack("<14I", max(1, 1000000 * scale // rate), 0, 0, (AVIF_HASINDEX if index else 0) | AVIF_ISINTERLEAVED,
                                       n if odml is None else odml[0], 0, len(lists), biggest, width, height, 0, 0, 0, 0))
    tail = b"" if odml is None else _list(b"odml", _chunk(b"dmlh", struct.pack("<I", n)))
    return _list(b"hdrl", avih + b"".join(lists) + tail)


# A plain AVI file is one RIFF form, and a RIFF size is 32 bits: the whole file stays below 4 GiB.  (ffmpeg changes to OpenDML
# past 1 GiB already; neither side of this module speaks it.)  A module constant so that a test can lower it.
AVI_MAX_BYTES = (1 << 32) - 1


def _as_pcm(pcm) -> np.ndarray:
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim not in (1, 2):
        raise ValueError("write_avi: pcm int16 [L] or [L, C]")
    return np.ascontiguousarray(pcm.reshape(len(pcm), -1)).astype("<i2", copy=False)


class AviWriter:
    """`write_avi` for frames that arrive in pieces: `add_frames(blobs)` appends one `00dc` chunk per JPEG file (an empty one is a
    dropped frame) as it comes, `close()` appends the `idx1` index and writes the header once more with the frame count, the
    largest frame and the list sizes -- the file is then, byte for byte, what `write_avi` writes from the same blobs and PCM, however
    they were cut into calls.  Only the index (16 bytes per chunk) is kept in memory.

    The sound is needed UP FRONT, as `pcm=` here or through `set_pcm(pcm)` before the first frame (int16 [L] / [L, C] at
    `audio_rate`; `channels`, when given, must be its channel count): every frame is followed by the samples of its own duration,
    and whether there is an audio stream decides the header's length.  The last frame takes the samples that are left, so the
    audio chunk of the newest frame is written when the next frame arrives, or at close.

    A plain AVI file cannot pass 4 GiB (AVI_MAX_BYTES): when an append would take the finished file -- the sound still owed and the
    index included -- past it, OSError names the limit and the partial file is removed; so is the file of a writer that is closed
    without one non-empty frame (ValueError), or left through an exception of its `with` block.

    `opendml=True` writes the layout of the OpenDML 1.02 extensions instead (what ffmpeg's muxer writes past 1 GiB; read back with
    open_avi(opendml=True)), and the file may pass 4 GiB: a first RIFF `AVI ` form whose movi list ends with one `ix##` standard index
    per stream, followed by an `idx1` over that form alone; then RIFF `AVIX` forms of one movi list each, ended the same way.  A
    chunk that would take the open form -- closed right behind it, its indexes included -- past `segment_bytes` opens the next
    form (a form holds at least one chunk, so only a chunk larger than that can make a form larger).  Each stream list carries an
    `indx` super index of `index_segments` entries, written with zeros and patched at close: {u64 file offset of the ix## chunk, u32
    its size with the header, u32 its duration in stream ticks}; a standard index entry is {u32 offset of the chunk's DATA from
    qwBaseOffset -- the file offset of its form's `movi` fourcc --, u32 size, bit 31 set for an empty (repeated) frame}.  avih counts
    the first form's frames, strh and LIST odml / dmlh the file's.  A file that would need more than `index_segments` forms raises
    OSError naming the limit and the partial file is removed.  With opendml=False (the default) neither argument is looked at.

    `codec="DIB"`: the chunks are uncompressed frames of `bits` (24 or 32) bits a pixel, bottom-up or top-down, instead of JPEG
    files (dib.py; write_avi_raw).  `path` may be a writable, seekable binary file object instead of a path; it is then neither
    closed nor removed."""

    def __init__(self, path, width: int, height: int, rate: int, scale: int = 1, audio_rate: int = 44100, channels: Optional[int] = None,
                 pcm: Optional[np.ndarray] = None, index: bool = True, opendml: bool = False, segment_bytes: int = 1 << 30,
                 index_segments: int = 256, codec: str = "MJPG", bits: int = 24, bottom_up: bool = True):
        self.opendml, self.segment_bytes, self.index_segments = bool(opendml), int(segment_bytes), int(index_segments)
        if self.opendml and not (0 < self.segment_bytes < 1 << 32 and self.index_segments >= 1 and index):
            raise ValueError("AviWriter: opendml takes segment_bytes in 1 .. 2^32 - 1, index_segments >= 1 and index=True")
        if codec not in ("MJPG", "DIB") or (codec == "DIB" and int(bits) not in (24, 32)):
            raise ValueError('AviWriter: codec "MJPG", or "DIB" with 24 or 32 bits')
        self._video = None
        if codec == "DIB":
            size = ((int(width) * (int(bits) // 8) + 3) & ~3) * int(height)
            self._video = (b"DIB ", b"\0\0\0\0", int(bits), int(height) if bottom_up else -int(height), size)
        self._owned = not hasattr(path, "write")
        self.path = path
        self.width, self.height, self.rate, self.scale = int(width), int(height), int(rate), int(scale)
        if self.rate <= 0 or self.scale <= 0:
            raise ValueError("write_avi: rate and scale positive")
        if self.width <= 0 or self.height <= 0:
            raise ValueError("write_avi: width and height positive")
        self.audio_rate, self.channels, self.index = int(audio_rate), channels, bool(index)
        self.n_frames = 0
        self._pcm = None
        self._file = None
        self._entries = []
        self._biggest = 0
        self._seen = False   # a non-empty frame has been written
        self._at = 4         # idx1 offsets count from the 'movi' fourcc
        self._closed = False
        if pcm is not None:
            self.set_pcm(pcm)

    def set_pcm(self, pcm):
        if self._file is not None or self._closed:
            raise ValueError("AviWriter: the sound must be set before the first frame (the header's length depends on it)")
        pcm = _as_pcm(pcm)
        if self.channels is not None and int(self.channels) != pcm.shape[1]:
            raise ValueError(f"AviWriter: pcm of {pcm.shape[1]} channels, channels={self.channels}")
        self._pcm = pcm

    def _sound(self):
        return None if self._pcm is None else (len(self._pcm), self._pcm.shape[1])

    def _header(self, n: int, biggest: int) -> bytes:
        odml = (self._first[2], self.index_segments, self._super[b"00dc"], self._super[b"01wb"]) if self.opendml else None
        return _hdrl(n, biggest, self.width, self.height, self.rate, self.scale, self._sound(), self.audio_rate, self.index, video=self._video,
                     odml=odml)

    def _open(self):
        self._file = open(self.path, "wb") if self._owned else self.path
        self._base = 0 if self._owned else self._file.tell()
        # OpenDML: the chunks of the open form per stream, the super-index entries of the closed ones, the first form's sizes
        self._seg, self._super, self._first = {b"00dc": [], b"01wb": []}, {b"00dc": [], b"01wb": []}, (0, 0, 0)
        self._seg_start, self._seg_frames, self._seg_ticks = 0, 0, 0
        hdrl = self._header(0, 0)
        self._file.write(b"RIFF\0\0\0\0AVI " + hdrl + b"LIST\0\0\0\0movi")
        self._movi = 12 + len(hdrl) + 8  # the file offset of the 'movi' fourcc

    def _fail(self, error):
        self._closed = True
        if self._file is not None:
            if self._owned:
                self._file.close()
                try:
                    os.remove(self.path)
                except OSError:
                    pass
            self._file = None
        return error

    def _streams(self):
        return (b"00dc",) if self._pcm is None else (b"00dc", b"01wb")

    def _form_bytes(self, cc: bytes, chunk: int) -> int:
        """The open form's length, header included, were a chunk of `chunk` bytes of stream `cc` appended and the form closed."""
        ix = sum(8 + 24 + 8 * (len(self._seg[c]) + (c == cc)) for c in self._streams())
        idx1 = 8 + 16 * (len(self._entries) + 1) if self._seg_start == 0 else 0
        return self._movi + self._at + chunk - self._seg_start + ix + idx1

    def _close_form(self):
        """The open form's ix## chunks (and the first form's idx1) behind its chunks, its two sizes, its super-index entries."""
        f = self._file
        for c in self._streams():
            rows = self._seg[c]
            body = struct.pack("<HBBI4sQI", 2, 0, 1, len(rows), c, self._base + self._movi, 0) + b"".join(struct.pack("<II", *r) for r in rows)
            self._super[c].append((self._base + self._movi + self._at, 8 + len(body), self._seg_frames if c == b"00dc" else self._seg_ticks))
            f.write(b"ix" + c[:2] + struct.pack("<I", len(body)) + body)
            self._at += 8 + len(body)
            self._seg[c] = []
        end = self._movi + self._at
        if self._seg_start == 0:
            body = b"".join(self._entries)
            f.write(b"idx1" + struct.pack("<I", len(body)) + body)
            end += 8 + len(body)
            self._first = (end - 8, self._at, self._seg_frames)  # written with the header, at close
        else:
            f.seek(self._base + self._seg_start + 4)
            f.write(struct.pack("<I", end - self._seg_start - 8))
            f.seek(self._base + self._movi - 4)
            f.write(struct.pack("<I", self._at))
            f.seek(self._base + end)
        return end

    def _next_form(self):
        if len(self._super[b"00dc"]) + 1 >= self.index_segments:
            raise self._fail(OSError(f"{self.path}: frame {self.n_frames} would open segment {self.index_segments + 1} of the file; its "
                                     f"super indexes hold index_segments = {self.index_segments} (of segment_bytes = {self.segment_bytes} bytes each)"))
        end = self._close_form()
        self._file.write(b"RIFF\0\0\0\0AVIXLIST\0\0\0\0movi")
        self._seg_start, self._movi, self._at = end, end + 20, 4
        self._seg_frames = self._seg_ticks = 0

    def _span(self, k: int, last: bool):
        """The samples behind frame k: about its duration's worth; the last frame takes what is left."""
        size = len(self._pcm)
        lo = min(size, k * self.audio_rate * self.scale // self.rate)
        hi = size if last else min(size, (k + 1) * self.audio_rate * self.scale // self.rate)
        return lo, hi

    def _put(self, cc: bytes, body, flags: int):
        size = len(body)
        if self.opendml:
            if (self._seg[b"00dc"] or self._seg[b"01wb"]) and self._form_bytes(cc, 8 + size + (size & 1)) > self.segment_bytes:
                self._next_form()
            self._seg[cc].append((self._at + 8, size | (0 if flags & AVIIF_KEYFRAME else 1 << 31)))
            if cc == b"00dc":
                self._seg_frames += 1
            else:
                self._seg_ticks += size // (2 * self._pcm.shape[1])
            if self._seg_start:  # idx1 covers the first form alone
                self._file.write(cc + struct.pack("<I", size))
                self._file.write(body)
                if size & 1:
                    self._file.write(b"\0")
                self._at += 8 + size + (size & 1)
                return
        self._entries.append(cc + struct.pack("<III", flags, self._at, size))
        self._file.write(cc + struct.pack("<I", size))
        self._file.write(body)
        if size & 1:
            self._file.write(b"\0")
        self._at += 8 + size + (size & 1)

    def _put_sound(self, k: int, last: bool):
        if self._pcm is not None:
            lo, hi = self._span(k, last)
            if hi > lo:
                self._put(b"01wb", self._pcm[lo:hi].tobytes(), AVIIF_KEYFRAME)

    def _room(self, size: int):
        """Refuses (OSError) the append of a video chunk of `size` bytes when the file, finished right behind it, would pass the limit."""
        owed = 0
        if self._pcm is not None:  # everything from the newest frame's first sample on is still to be written, in at most ...
            left = 2 * self._pcm.shape[1] * (len(self._pcm) - self._span(max(self.n_frames - 1, 0), False)[0])
            owed = left + 9 * 2  # ... two chunks (that frame's, and the new last frame's)
        index = 8 + 16 * (len(self._entries) + 3) if self.index else 0
        end = self._movi + self._at + 8 + size + 1 + owed + 1 + index
        if end > AVI_MAX_BYTES:
            raise self._fail(OSError(f"{self.path}: frame {self.n_frames} would take the file to {end} bytes, past the {AVI_MAX_BYTES} bytes "
                                     "(4 GiB) a plain AVI file can have; OpenDML is not written"))

    def add_frames(self, blobs: Sequence):
        """One video chunk per item of `blobs` (bytes-like; empty: a dropped frame), behind the frames already written."""
        if self._closed:
            raise ValueError("AviWriter: closed")
        for blob in blobs:
            if self._video is not None and len(blob) not in (0, self._video[4]):
                raise self._fail(ValueError(f"AviWriter: frame {self.n_frames}: {len(blob)} bytes, an uncompressed frame is {self._video[4]} bytes"))
            if self._file is None:
                self._open()
            if not self.opendml:
                self._room(len(blob))
            if self.n_frames:
                self._put_sound(self.n_frames - 1, False)
            self._put(b"00dc", blob, AVIIF_KEYFRAME if len(blob) else 0)
            self._biggest = max(self._biggest, len(blob))
            self._seen = self._seen or len(blob) > 0
            self.n_frames += 1
        return self

    def close(self):
        """The last frame's sound, the index, the header with its final counts.  Returns `path`."""
        if self._closed:
            return self.path
        if not self._seen:
            raise self._fail(ValueError("write_avi: no frame"))
        f = self._file
        self._put_sound(self.n_frames - 1, True)
        if self.opendml:
            end = self._close_form()
            f.seek(self._base)
            f.write(b"RIFF" + struct.pack("<I", self._first[0]) + b"AVI " + self._header(self.n_frames, self._biggest) + b"LIST" +
                    struct.pack("<I", self._first[1]))
            f.seek(self._base + end)
            if self._owned:
                f.close()
            self._file, self._closed = None, True
            return self.path
        if self._at & 1:  # (cannot happen, every chunk is padded; build_avi says the same)
            f.write(b"\0")
        if self.index:
            body = b"".join(self._entries)
            f.write(b"idx1" + struct.pack("<I", len(body)) + body)
        end = f.tell()
        hdrl = _hdrl(self.n_frames, self._biggest, self.width, self.height, self.rate, self.scale, self._sound(), self.audio_rate, self.index,
                     video=self._video)
        f.seek(self._base)
        f.write(b"RIFF" + struct.pack("<I", end - self._base - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", self._at))
        f.seek(end)
        if self._owned:
            f.close()
        self._file, self._closed = None, True
        return self.path

    def __enter__(self):
        return self

    def __exit__(self, kind, *exc):
        if kind is None:
            self.close()
        elif not self._closed:
            self._fail(None)


def _in_memory(blobs, width, height, rate, scale, pcm, audio_rate, **kw) -> bytes:
    """The bytes an AviWriter with these arguments writes from `blobs` in one append."""
    import io

    f = io.BytesIO()
    with AviWriter(f, width, height, rate, scale, audio_rate, pcm=pcm, **kw) as w:
        w.add_frames(blobs)
    return f.getvalue()


def raw_chunks(frames_u8_bgr, bits: int = 24, bottom_up: bool = True):
    """Frames uint8 [n, H, W, 3] in BGR order (or a sequence of [H, W, 3] frames; None or an empty one: a dropped frame) -> (the
    chunks of an uncompressed AVI stream of `bits` bits a pixel, one bytes object per frame, width, height): rows padded to 4 bytes
    with zeros, the last row first when bottom_up, a fourth byte of zero per pixel at 32 bits.  dib.unpack_numpy is the inverse."""
    if int(bits) not in (24, 32):
        raise ValueError("write_avi_raw: 24 or 32 bits")
    shape = next((np.shape(f) for f in frames_u8_bgr if f is not None and np.size(f)), None)
    if shape is None or len(shape) != 3 or shape[2] != 3:
        raise ValueError("write_avi_raw: no frame of shape [H, W, 3]")
    h, w = shape[:2]
    bpp = int(bits) // 8
    stride = (w * bpp + 3) & ~3
    chunks = []
    for k, f in enumerate(frames_u8_bgr):
        if f is None or not np.size(f):
            chunks.append(b"")
            continue
        f = np.asarray(f)
        if f.shape != shape or f.dtype != np.uint8:
            raise ValueError(f"write_avi_raw: frame {k}: {f.dtype} {list(f.shape)}, the frames are uint8 {list(shape)}")
        rows = np.zeros((h, stride), dtype=np.uint8)
        rows[:, :w * bpp].reshape(h, w, bpp)[:, :, :3] = f
        chunks.append((rows[::-1] if bottom_up else rows).tobytes())
    return chunks, w, h


def build_avi_raw(frames_u8_bgr, rate: int, scale: int = 1, pcm: Optional[np.ndarray] = None, audio_rate: int = 44100, bits: int = 24,
                  bottom_up: bool = True, opendml: bool = False, segment_bytes: int = 1 << 30, index_segments: int = 256) -> bytes:
    """The bytes `write_avi_raw` writes."""
    chunks, w, h = raw_chunks(frames_u8_bgr, bits, bottom_up)
    return _in_memory(chunks, w, h, rate, scale, pcm, audio_rate, codec="DIB", bits=bits, bottom_up=bottom_up, opendml=opendml,
                      segment_bytes=segment_bytes, index_segments=index_segments)


def write_avi_raw(path, frames_u8_bgr, rate: int, scale: int = 1, pcm: Optional[np.ndarray] = None, audio_rate: int = 44100, bits: int = 24,
                  bottom_up: bool = True, opendml: bool = False, segment_bytes: int = 1 << 30, index_segments: int = 256):
    """Writes the uncompressed AVI file `path` -- what `ffmpeg -c:v rawvideo -pix_fmt bgr24 -c:a pcm_s16le` writes: BI_RGB frames of
    `bits` (24 or 32) bits a pixel from `frames_u8_bgr` (uint8 [n, H, W, 3], BGR; raw_chunks), bottom-up (biHeight > 0) or top-down,
    sound and timing as write_avi.  A frame is stride * H bytes, so pass opendml=True for more than a few seconds of HD material (a
    plain file stops at 4 GiB: 690 frames of 1920 x 1080).  Returns `path`."""
    chunks, w, h = raw_chunks(frames_u8_bgr, bits, bottom_up)
    with AviWriter(path, w, h, rate, scale, audio_rate, pcm=pcm, codec="DIB", bits=bits, bottom_up=bottom_up, opendml=opendml,
                   segment_bytes=segment_bytes, index_segments=index_segments) as wr:
        wr.add_frames(chunks)
    return path


def write_avi(path, jpeg_blobs: Sequence, rate: int, scale: int = 1, pcm: Optional[np.ndarray] = None, audio_rate: int = 44100,
              index: bool = True, opendml: bool = False, segment_bytes: int = 1 << 30, index_segments: int = 256):
    """Writes the Motion-JPEG AVI file `path`: one `00dc` chunk per JPEG file of `jpeg_blobs` (an empty one is a dropped frame)
    at `rate` / `scale` frames per second, `pcm` (int16 [L] or [L, C] at `audio_rate`) as stream 01, interleaved in chunks of about
    one video frame's duration, and an `idx1` index when asked.  `open_avi` of the file gives the same bytes and the same samples.
    One AviWriter fed everything at once: the picture size is the first frame's own, and a file past 4 GiB is its OSError --
    unless `opendml` (with `segment_bytes`, `index_segments`: AviWriter) asks for the OpenDML layout, which has no such end.
    Returns `path`."""
    first = next((b for b in jpeg_blobs if len(b)), None)
    if first is None:
        raise ValueError("write_avi: no frame")
    rate, scale = int(rate), int(scale)
    if rate <= 0 or scale <= 0:
        raise ValueError("write_avi: rate and scale positive")
    width, height = jpeg_size(first)
    with AviWriter(path, width, height, rate, scale, audio_rate, pcm=pcm, index=index, opendml=opendml, segment_bytes=segment_bytes,
                   index_segments=index_segments) as w:
        w.add_frames(jpeg_blobs)
    return path
