"""JPEG face crops decoded behind a host entropy pass (csrc/jpeg.hip, include/avcer_hip.h "JPEG face crops").

`decode_tiles` / `decode_canvas` take the bytes of n files.  One native host call parses the markers and Huffman-decodes every file
the parser supports (a small thread pool, files are independent); the int16 coefficients and the per-file descriptors go to the
device through pinned staging buffers kept on the engine, and two kernels do the rest: dequantisation + inverse DCT into component
planes, then exactly the pixels the output needs (chroma upsampling, YCbCr -> RGB, the NEAREST tile or the full-size canvas).  The
result is bit-identical to `PIL.Image.open(...).convert("RGB")` (libjpeg-turbo's integer arithmetic, restated).

A file the parser does not handle -- a PNG under a .jpg name, a progressive or CMYK file, a truncated one, ... -- goes through the
PIL lines of `video_pipeline.read_face_dir` unchanged; what PIL does with it (decode it, or raise OSError) is what the caller sees.
Both functions also return, per file, which path served it: "device" or "pil".
"""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np
import torch

OK, NOT_HANDLED = 0, 1
R_NO_SPACE = 12  # csrc/jpeg.hip: the file's blocks did not fit the coefficient storage given

# struct avcer_jpeg_desc
DESC = np.dtype([("status", "<i4"), ("reason", "<i4"), ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"),
                 ("vs", "<i4"), ("bw", "<i4", 3), ("bh", "<i4", 3), ("tq", "<i4", 3), ("coef_block", "<i8"), ("n_blocks", "<i8"),
                 ("qt", "<u2", (3, 64))])
assert DESC.itemsize == 464


def probe(lib, blob: bytes) -> np.ndarray:
    """avcer_jpeg_probe of one file: a DESC record (header fields, status, reason)."""
    info = np.zeros(1, dtype=DESC)
    rc = lib.avcer_jpeg_probe(C.cast(C.c_char_p(blob), C.c_void_p), len(blob), info.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError(f"avcer_jpeg_probe failed: {rc}")
    return info[0]


def host_threads(threads: int = 0) -> int:
    """Threads of the host entropy pass: `threads`, or min(16, OMP_NUM_THREADS or 16) -- never the machine's core count."""
    if threads <= 0:
        try:
            threads = int(os.environ.get("OMP_NUM_THREADS", "16"))
        except ValueError:
            threads = 16
    return min(16, threads) if threads > 0 else 16


def entropy_batch(lib, blobs, coeffs: np.ndarray, desc: np.ndarray, threads: int = 0, ctx=None, cap_blocks: int | None = None) -> int:
    """avcer_jpeg_entropy_batch: the files `blobs` -> coefficients in `coeffs` (int16, room for `cap_blocks` blocks of 64, default all
    of it) and `desc[:n]` (DESC records).  Returns the blocks all files with a supported header need together."""
    n = len(blobs)
    files = (C.c_char_p * max(n, 1))(*blobs)
    lens = np.array([len(b) for b in blobs], dtype=np.int64)
    need = C.c_int64(0)
    cap = coeffs.size // 64 if cap_blocks is None else int(cap_blocks)
    assert coeffs.dtype == np.int16 and coeffs.flags.c_contiguous and cap * 64 <= coeffs.size
    assert desc.dtype == DESC and desc.flags.c_contiguous and len(desc) >= n
    rc = lib.avcer_jpeg_entropy_batch(ctx, C.cast(files, C.c_void_p), lens.ctypes.data_as(C.c_void_p), n,
                                      coeffs.ctypes.data_as(C.c_void_p), cap, desc.ctypes.data_as(C.c_void_p), host_threads(int(threads)),
                                      C.byref(need))
    if rc != 0:
        raise RuntimeError(f"avcer_jpeg_entropy_batch failed: {rc}")
    return int(need.value)


# ---------------------------------------------------------------------------------------------------- numpy statement (tests)
def _idct_1d(v, shift):
    """csrc/jpeg.hip idct_1d (libjpeg jidctint.c) along axis 0 of an int64 array [8, ...]."""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * (-15137)
    tmp3 = z1 + z2 * 6270
    z2, z3 = v[0], v[4]
    tmp0 = (z2 + z3) << 13
    tmp1 = (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                     tmp10 - tmp3]) + r >> shift


PAIR_MAX = 16383  # csrc/jpeg.hip IDCT_PAIR_MAX


def _plane(coeffs, qt, bw, bh):
    """Kernel A for one component: blocks [bh * bw, 64] int16 -> (u8 plane [8 bh, 8 bw], the range guard's verdict: True when
    every value stayed inside the range in which the decode is defined)."""
    x = coeffs.reshape(bh * bw, 8, 8).astype(np.int64) * qt.reshape(1, 8, 8).astype(np.int64)
    ok = np.abs(x).max(initial=0) <= PAIR_MAX
    x = _idct_1d(x.transpose(1, 0, 2), 11)                   # columns: [row, block, col]
    ok = ok and np.abs(x).max(initial=0) <= PAIR_MAX
    x = _idct_1d(x.transpose(2, 1, 0), 18)                   # rows: [col, block, row]
    ok = ok and x.min(initial=0) >= -512 and x.max(initial=0) <= 511
    x = np.clip(x + 128, 0, 255).astype(np.uint8)            # [col, block, row]
    return x.transpose(1, 2, 0).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw), bool(ok)


def _chroma(p, w, h, hs, vs):
    """Kernel B's chroma_at at every pixel of a w x h image: the plane `p` of a component subsampled hs x vs."""
    p = p.astype(np.int64)
    x, y = np.arange(w), np.arange(h)
    if hs == 1:
        return p[:h, :w]
    dw, dh = (w + 1) // 2, (h + vs - 1) // vs
    s = x >> 1
    if dw <= 2:
        return p[(y >> 1) if vs == 2 else y][:, s]
    sn = np.where(x & 1, np.minimum(s + 1, dw - 1), np.maximum(s - 1, 0))
    if vs == 1:
        r = p[:h]
        return (3 * r[:, s] + r[:, sn] + np.where(x & 1, 2, 1)[None]) >> 2
    t = y >> 1
    tn = np.where(y & 1, np.minimum(t + 1, dh - 1), np.maximum(t - 1, 0))
    col = 3 * p[t] + p[tn]                                   # [h, plane width]
    return (3 * col[:, s] + col[:, sn] + np.where(x & 1, 7, 8)[None]) >> 4


def pixels_numpy(coeffs: np.ndarray, desc: np.ndarray):
    """Kernels A and B of csrc/jpeg.hip stated in numpy (for the tests; not a product path): the coefficient storage and the DESC
    records of avcer_jpeg_entropy_batch -> per file the RGB image u8 [h, w, 3], or None where the status is not OK or the range guard
    of kernel A fires (the device's flag)."""
    out = []
    coeffs = coeffs.reshape(-1, 64)
    for d in np.atleast_1d(desc):
        if d["status"] != OK:
            out.append(None)
            continue
        w, h, nc = int(d["width"]), int(d["height"]), int(d["ncomp"])
        at = int(d["coef_block"])
        planes, ok = [], True
        for c in range(nc):
            bw, bh = int(d["bw"][c]), int(d["bh"][c])
            plane, fine = _plane(coeffs[at:at + bw * bh], d["qt"][c], bw, bh)
            planes.append(plane)
            ok = ok and fine
            at += bw * bh
        if not ok:
            out.append(None)
            continue
        yy = planes[0][:h, :w].astype(np.int64)
        if nc == 1:
            out.append(np.repeat(yy[:, :, None], 3, axis=2).astype(np.uint8))
            continue
        hs, vs = int(d["hs"]), int(d["vs"])
        cb = _chroma(planes[1], w, h, hs, vs) - 128
        cr = _chroma(planes[2], w, h, hs, vs) - 128
        r = yy + ((91881 * cr + 32768) >> 16)
        g = yy + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        b = yy + ((116130 * cb + 32768) >> 16)
        out.append(np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8))
    return out


# ---------------------------------------------------------------------------------------------------- the device path
class _Staging:
    """Pinned host buffers of one engine: coefficients and descriptors.  Reused by every call; the event says when the copies
    queued from them have been read, so the next call may overwrite them."""

    def __init__(self):
        self.coeffs = None
        self.desc = None
        self.event = None

    def reserve(self, blocks: int, n: int):
        if self.event is not None:
            self.event.synchronize()
        if self.coeffs is None or self.coeffs.numel() < 64 * blocks:
            self.coeffs = torch.empty(64 * (blocks + blocks // 4 + 1024), dtype=torch.int16, pin_memory=True)
        if self.desc is None or self.desc.numel() < DESC.itemsize * n:
            self.desc = torch.empty(DESC.itemsize * (n + n // 4 + 64), dtype=torch.uint8, pin_memory=True)


def _pil_rgb(blob: bytes) -> np.ndarray:
    from PIL import Image

    with Image.open(io.BytesIO(blob)) as img:
        return np.array(img.convert("RGB"))  # a copy: torch.from_numpy wants a writable array


def _pil_tile(blob: bytes) -> np.ndarray:
    """The lines of video_pipeline.read_face_dir."""
    from PIL import Image

    with Image.open(io.BytesIO(blob)) as img:
        return np.asarray(img.convert("RGB").resize((224, 224), Image.Resampling.NEAREST))


def _to_device(engine, blobs, threads: int):
    """Host entropy pass + copies: (coeffs on the device, desc on the device, n_blocks, desc records on the host)."""
    st = engine.__dict__.setdefault("_jpeg_staging", _Staging())
    n = len(blobs)
    # a JPEG of b bytes seldom holds more than b / 8 blocks (in practice a block costs tens of bits); grow and repeat if so.  The
    # parser refuses a header that claims more than 4 blocks per byte of scan (2 bits each at the least), so `need` is at most
    # 4 * the bytes given and a tiny file with a 65535 x 65535 header goes to PIL without any storage reserved for it
    st.reserve(max(sum(len(b) for b in blobs) // 8, 1024), n)
    while True:
        coeffs = st.coeffs.numpy()
        desc = st.desc.numpy()[:DESC.itemsize * n].view(DESC)
        need = entropy_batch(engine.lib, blobs, coeffs, desc, threads, engine.ctx)
        if not (desc["reason"] == R_NO_SPACE).any():
            break
        st.reserve(need, n)
    used = int((desc["coef_block"] + desc["n_blocks"]).max()) if n else 0
    if used == 0:
        return None, None, 0, desc.copy()
    dev = engine.device
    c_dev = st.coeffs[:64 * used].to(dev, non_blocking=True)
    d_dev = st.desc[:DESC.itemsize * n].to(dev, non_blocking=True)
    host = desc.copy()
    st.event = torch.cuda.Event()
    st.event.record(torch.cuda.current_stream(dev))
    return c_dev, d_dev, used, host


def _flags_to_host(engine, flags):
    """Queues the copy of kernel A's per-file flags (i32 [n] on the device) into pinned memory and returns the function that
    waits for it and hands out the numpy array: the caller does its other host work in between."""
    host = torch.empty(flags.shape, dtype=flags.dtype, pin_memory=True)
    host.copy_(flags, non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(engine.device))

    def wait():
        done.synchronize()
        return host.numpy()

    return wait


def decode_tiles(engine, blobs, threads: int = 0):
    """The files `blobs` -> (tiles u8 [n,224,224,3] RGB on the device, paths): tile i is
    Image.open(file i).convert("RGB").resize((224, 224), NEAREST); paths[i] is "device" or "pil"."""
    n = len(blobs)
    tiles = torch.empty(n, 224, 224, 3, dtype=torch.uint8, device=engine.device)
    if n == 0:
        return tiles, []
    c_dev, d_dev, used, desc = _to_device(engine, blobs, threads)
    status = desc["status"].copy()
    flags = _flags_to_host(engine, engine.jpeg_tiles(c_dev, d_dev, n, used, out=tiles)[1]) if used else None
    # the files the parser refused go through PIL while the kernels run; only then the range guard of kernel A is read (the one
    # wait of this call: `paths` cannot be known before it), and a file it flagged follows them
    host = {i: _pil_tile(blobs[i]) for i in range(n) if status[i] != OK}
    if flags is not None:
        for i in np.nonzero(flags())[0]:
            status[i] = NOT_HANDLED
            host[int(i)] = _pil_tile(blobs[i])
    if host:
        rest = sorted(host)
        tiles[torch.as_tensor(rest, device=engine.device)] = torch.from_numpy(np.stack([host[i] for i in rest])).to(engine.device)
    return tiles, ["device" if s == OK else "pil" for s in status]


def decode_canvas(engine, blobs, threads: int = 0):
    """The files `blobs` at full size -> ((canvas u8 [max(n,1), max h, max w, 3] on the device, rects i32 [n,5] = (i, 0, 0, w, h)),
    paths): the layout of video_pipeline.read_face_crops, the input of Engine.crop_resize_linear."""
    n = len(blobs)
    dev = engine.device
    if n == 0:
        return (torch.zeros(1, 1, 1, 3, dtype=torch.uint8, device=dev), np.zeros((0, 5), dtype=np.int32)), []
    c_dev, d_dev, used, desc = _to_device(engine, blobs, threads)
    status = desc["status"].copy()
    rest = {i: _pil_rgb(blobs[i]) for i in range(n) if status[i] != OK}
    sizes = [(rest[i].shape[1], rest[i].shape[0]) if i in rest else (int(desc["width"][i]), int(desc["height"][i])) for i in range(n)]
    wmax, hmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if used:
        canvas, flags = engine.jpeg_rgb(c_dev, d_dev, n, used, hmax, wmax)
        for i in np.nonzero(_flags_to_host(engine, flags)())[0]:  # the range guard of kernel A; such a file's slot is zero so far
            status[i] = NOT_HANDLED
            rest[int(i)] = _pil_rgb(blobs[i])
            if rest[int(i)].shape[:2] != (sizes[i][1], sizes[i][0]):
                raise OSError(f"file {i}: PIL reads another size than its header states")
    else:
        canvas = torch.zeros(n, hmax, wmax, 3, dtype=torch.uint8, device=dev)
    paths = ["device" if s == OK else "pil" for s in status]
    for i, img in rest.items():
        canvas[i, :img.shape[0], :img.shape[1]] = torch.from_numpy(img).to(dev)
    rects = np.array([(i, 0, 0, w, h) for i, (w, h) in enumerate(sizes)], dtype=np.int32).reshape(n, 5)
    return (canvas, rects), paths
