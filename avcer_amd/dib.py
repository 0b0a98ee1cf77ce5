"""Uncompressed video frames of an AVI file: BI_RGB device-independent bitmaps of 24 or 32 bits a pixel, what
`ffmpeg -i clip.mp4 -c:v rawvideo -pix_fmt bgr24 -c:a pcm_s16le clip.avi` writes (avcer_amd/avi.py names the container).  These are
the decoder's own BGR frames -- what cv2.VideoCapture hands the reference (data/get_face_images.py:19-24, 44-47) -- without a lossy
Motion-JPEG transcode in between.

A frame is `height` rows of stride = (width * bits / 8 + 3) & ~3 bytes; bytes 0, 1, 2 of a pixel are B, G, R, byte 3 (32 bits) is
dropped; the picture's LAST row comes first when the frame is bottom-up (biHeight > 0).  A DIB frame behind a BITMAPFILEHEADER and
a BITMAPINFOHEADER is a BMP file, and the contract is identity with PIL's BMP reader on it, tolerance zero
(tests/test_dib_cpu.py).

`unpack_numpy` is the statement on the CPU, `unpack_frames` the same bytes on the device (avcer_dib_frames, csrc/dib.hip): the
file bytes of a pass are uploaded as they lie in the file -- no row is repacked on the host -- and the kernel drops the padding,
turns the rows over and swaps the channels on the way into the frame batch.
"""
from __future__ import annotations

import numpy as np


def stride_of(width: int, bits: int) -> int:
    """Bytes of a source row: width * bits / 8, padded to 4."""
    return (int(width) * (int(bits) // 8) + 3) & ~3


def _check(height, width, bits):
    height, width, bits = int(height), int(width), int(bits)
    if bits not in (24, 32):
        raise ValueError(f"dib: {bits} bits a pixel: 24 or 32 (BI_RGB) are read")
    if height <= 0 or width <= 0:
        raise ValueError("dib: height and width positive")
    return height, width, bits, stride_of(width, bits) * height


def _lengths(chunks, size):
    for i, c in enumerate(chunks):
        if len(c) != size:
            raise ValueError(f"frame {i}: a chunk of {len(c)} bytes, a frame is {size} bytes")


def unpack_numpy(chunks, height: int, width: int, bits: int, bottom_up: bool, bgr: bool = True) -> np.ndarray:
    """The frames `chunks` (bytes-like, stride_of(width, bits) * height bytes each) -> uint8 [n, height, width, 3], top-down, in BGR
    order or, with bgr=False, RGB: np.asarray(Image.open(<the frame as a BMP file>).convert("RGB")), channels reversed for bgr."""
    height, width, bits, size = _check(height, width, bits)
    _lengths(chunks, size)
    out = np.empty((len(chunks), height, width, 3), dtype=np.uint8)
    for i, c in enumerate(chunks):
        rows = np.frombuffer(c, dtype=np.uint8).reshape(height, -1)[:, :width * (bits // 8)].reshape(height, width, bits // 8)[:, :, :3]
        if bottom_up:
            rows = rows[::-1]
        out[i] = rows if bgr else rows[:, :, ::-1]
    return out


def _address(c) -> int:
    return np.frombuffer(c, dtype=np.uint8).ctypes.data if len(c) else 0


def unpack_frames(engine, chunks, height: int, width: int, bits: int, bottom_up: bool, bgr: bool = True, frames_per_pass: int = 64):
    """The same frames on the device -> uint8 [n, height, width, 3] there (`avi.open_avi(path).frames` of a raw file, or any n
    buffers of one frame each; what unpack_numpy returns, bit for bit).  The frames never exist unpacked on the host.
    Works in passes of at most `frames_per_pass` frames: the chunks of a pass are copied as they are, one copy each, back to back
    (2-byte aligned, as in the file) into a pinned staging buffer of the engine, cross in ONE copy, and avcer_dib_frames reads them
    through a table of one byte offset per frame.  A chunk that occurs twice in a pass -- a dropped frame repeats its predecessor --
    is copied once and its offset is used twice.  Staging and device storage are a pass's, not the video's, and the result does
    not depend on `frames_per_pass`.  ValueError naming the frame for a chunk of another length."""
    import torch

    height, width, bits, size = _check(height, width, bits)
    n, per = len(chunks), int(frames_per_pass)
    if per <= 0:
        raise ValueError("unpack_frames: frames_per_pass positive")
    _lengths(chunks, size)
    dev = engine.device
    frames = torch.empty(n, height, width, 3, dtype=torch.uint8, device=dev)
    slot = size + (size & 1)
    for lo in range(0, n, per):
        part = chunks[lo:lo + per]
        # one slot per DISTINCT chunk of the pass (the same bytes at the same address: the same memoryview, or an equal slice)
        seen, offsets = {}, np.empty(len(part), dtype=np.int64)
        for k, c in enumerate(part):
            offsets[k] = seen.setdefault(_address(c), len(seen)) * slot
        need = len(seen) * slot
        stage = engine.__dict__.get("_dib_stage")
        if stage is None or stage[0].numel() < need:
            if stage is not None:
                stage[2].synchronize()
            stage = engine.__dict__["_dib_stage"] = (torch.empty(need, dtype=torch.uint8, pin_memory=True),
                                                     torch.empty(need, dtype=torch.uint8, device=dev), torch.cuda.Event())
        host, span, busy = stage
        busy.synchronize()  # the pass before has left the staging buffer
        flat = host.numpy()
        done = set()
        for k, c in enumerate(part):
            at = int(offsets[k])
            if at not in done:
                done.add(at)
                flat[at:at + size] = np.frombuffer(c, dtype=np.uint8)
        span[:need].copy_(host[:need], non_blocking=True)
        table = torch.from_numpy(offsets).to(dev)
        busy.record(torch.cuda.current_stream(dev))
        engine.dib_frames(span[:need], table, len(part), height, width, bits, bottom_up, bgr=bgr, out=frames[lo:lo + len(part)])
    return frames
