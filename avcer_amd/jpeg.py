"""JPEG face crops decoded behind a host entropy pass, and encoded in front of one (csrc/jpeg_*.hip, include/avcer_hip.h "JPEG
face crops").  Decoding first; `encode_images` and its numpy statement `forward_numpy` are in the second half of this file.

`decode_tiles` / `decode_canvas` take the bytes of n files.  One native host call parses the markers and Huffman-decodes every file
the parser supports (a small thread pool, files are independent); the int16 coefficients and the per-file descriptors go to the
device through pinned staging buffers kept on the engine, and two kernels do the rest: dequantisation + inverse DCT into component
planes, then exactly the pixels the output needs (chroma upsampling, YCbCr -> RGB, the NEAREST tile or the full-size canvas).  The
result is bit-identical to `PIL.Image.open(...).convert("RGB")` (libjpeg-turbo's integer arithmetic, restated).

A file the parser does not handle -- a PNG under a .jpg name, a progressive or CMYK file, a truncated one, ... -- goes through the
PIL lines of `video_pipeline.read_face_dir` unchanged; what PIL does with it (decode it, or raise OSError) is what the caller sees.
Both functions also return, per file, which path served it: "device" or "pil".

With entropy="device" the host parses the headers only (`scan_batch`), the files' entropy-coded bytes cross instead of the
coefficients, and `Engine.jpeg_unpack` Huffman-decodes them on the device (csrc/jpeg_unpack.hip avcer_jpeg_unpack); tiles, canvas and paths
are the same.

`decode_frames` is the same path for the frames of a Motion-JPEG video (avcer_amd/avi.py): whole frames of one size in BGR or
RGB order (avcer_jpeg_frames), in passes, frames without DHT segments decoded with the standard's tables.

`roundtrip_tiles` / `roundtrip_canvas` (the last part of this file) are decode(encode(crop)) without a file: the crop as the
reference's stage 1 sees it, from one fused kernel and the decoder's pixel kernel.
"""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np
import torch

OK, NOT_HANDLED = 0, 1
R_NO_SPACE = 12  # csrc/jpeg.h: the file's blocks did not fit the coefficient storage given

# struct avcer_jpeg_desc
DESC = np.dtype([("status", "<i4"), ("reason", "<i4"), ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"),
                 ("vs", "<i4"), ("bw", "<i4", 3), ("bh", "<i4", 3), ("tq", "<i4", 3), ("coef_block", "<i8"), ("n_blocks", "<i8"),
                 ("qt", "<u2", (3, 64))])
assert DESC.itemsize == 464
# struct avcer_jpeg_scan, struct avcer_jpeg_tab (the device entropy decoder's view of a file and of a Huffman table)
SCAN = np.dtype([("offset", "<i8"), ("nbytes", "<i8"), ("restart", "<i4"), ("dc", "<i4", 3), ("ac", "<i4", 3), ("pad", "<i4")])
TAB = np.dtype([("bits", "u1", 17), ("vals", "u1", 256), ("pad", "u1", 15)])
assert SCAN.itemsize == 48 and TAB.itemsize == 288


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


STD_TABLES = 1  # AVCER_JPEG_STD_TABLES


def _file_pointers(blobs):
    """The files as the native calls take them: (pointer array, lengths i64, what keeps the pointers alive).  `bytes` go as they
    are; any other buffer (a memoryview of a mapped AVI file, read-only) goes by its address: nothing is copied."""
    n = len(blobs)
    lens = np.array([len(b) for b in blobs], dtype=np.int64)
    if all(isinstance(b, bytes) for b in blobs):
        return (C.c_char_p * max(n, 1))(*blobs), lens, blobs
    keep = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
    return (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in keep]), lens, keep


def entropy_batch(lib, blobs, coeffs: np.ndarray, desc: np.ndarray, threads: int = 0, ctx=None, cap_blocks: int | None = None,
                  std_tables: bool = False) -> int:
    """avcer_jpeg_entropy_batch: the files `blobs` -> coefficients in `coeffs` (int16, room for `cap_blocks` blocks of 64, default all
    of it) and `desc[:n]` (DESC records).  Returns the blocks all files with a supported header need together.
    std_tables: avcer_jpeg_entropy_batch_ex with AVCER_JPEG_STD_TABLES -- a Huffman table the scan references and no DHT defined is
    the standard's (Motion-JPEG frames)."""
    n = len(blobs)
    files, lens, _keep = _file_pointers(blobs)
    need = C.c_int64(0)
    cap = coeffs.size // 64 if cap_blocks is None else int(cap_blocks)
    assert coeffs.dtype == np.int16 and coeffs.flags.c_contiguous and cap * 64 <= coeffs.size
    assert desc.dtype == DESC and desc.flags.c_contiguous and len(desc) >= n
    args = (ctx, C.cast(files, C.c_void_p), lens.ctypes.data_as(C.c_void_p), n, coeffs.ctypes.data_as(C.c_void_p), cap,
            desc.ctypes.data_as(C.c_void_p), host_threads(int(threads)))
    rc = lib.avcer_jpeg_entropy_batch_ex(*args, STD_TABLES, C.byref(need)) if std_tables else lib.avcer_jpeg_entropy_batch(*args, C.byref(need))
    if rc != 0:
        raise RuntimeError(f"avcer_jpeg_entropy_batch failed: {rc}")
    return int(need.value)


def scan_batch(lib, blobs, data: np.ndarray, desc: np.ndarray, scan: np.ndarray, tabs: np.ndarray, threads: int = 0, ctx=None,
               cap_bytes: int | None = None, cap_tabs: int | None = None, std_tables: bool = False):
    """avcer_jpeg_scan_batch: the files `blobs` -> `desc[:n]` as entropy_batch leaves them before its scan walk, `scan[:n]` (SCAN
    records), the batch's Huffman tables de-duplicated in `tabs` (TAB records) and every handled file's entropy-coded bytes in `data`
    (u8, room for `cap_bytes`, default all of it).  The host walks no bit stream.  Returns (tables, bytes, blocks) that all files
    with a supported header need together; a file that did not fit `data` or `tabs` has reason R_NO_SPACE.
    std_tables: avcer_jpeg_scan_batch_ex with AVCER_JPEG_STD_TABLES, as in entropy_batch."""
    n = len(blobs)
    files, lens, _keep = _file_pointers(blobs)
    cap_b = data.size if cap_bytes is None else int(cap_bytes)
    cap_t = len(tabs) if cap_tabs is None else int(cap_tabs)
    assert data.dtype == np.uint8 and data.flags.c_contiguous and cap_b <= data.size
    assert desc.dtype == DESC and desc.flags.c_contiguous and len(desc) >= n
    assert scan.dtype == SCAN and scan.flags.c_contiguous and len(scan) >= n
    assert tabs.dtype == TAB and tabs.flags.c_contiguous and cap_t <= len(tabs)
    n_tabs, need_bytes, need_blocks = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    args = (ctx, C.cast(files, C.c_void_p), lens.ctypes.data_as(C.c_void_p), n, data.ctypes.data_as(C.c_void_p), cap_b,
            desc.ctypes.data_as(C.c_void_p), scan.ctypes.data_as(C.c_void_p), tabs.ctypes.data_as(C.c_void_p), cap_t, host_threads(int(threads)))
    outs = (C.byref(n_tabs), C.byref(need_bytes), C.byref(need_blocks))
    rc = lib.avcer_jpeg_scan_batch_ex(*args, STD_TABLES, *outs) if std_tables else lib.avcer_jpeg_scan_batch(*args, *outs)
    if rc != 0:
        raise RuntimeError(f"avcer_jpeg_scan_batch failed: {rc}")
    return int(n_tabs.value), int(need_bytes.value), int(need_blocks.value)


def unpack_host(lib, data: np.ndarray, scan: np.ndarray, tabs: np.ndarray, desc: np.ndarray, n_blocks: int, sub_bits: int = 0):
    """avcer_jpeg_unpack_host: the device entropy decoder's algorithm as host loops (for the tests; not a product path).  The
    arrays as scan_batch wrote them -> (coefficients int16 [n_blocks, 64], status i32 [n]); `desc` gets status and reason."""
    n = len(desc)
    assert data.dtype == np.uint8 and data.flags.c_contiguous and scan.dtype == SCAN and scan.flags.c_contiguous and len(scan) >= n
    assert tabs.dtype == TAB and tabs.flags.c_contiguous and desc.dtype == DESC and desc.flags.c_contiguous
    coeffs = np.zeros((int(n_blocks), 64), dtype=np.int16)
    status = np.zeros(n, dtype=np.int32)
    rc = lib.avcer_jpeg_unpack_host(None, data.ctypes.data_as(C.c_void_p), data.size, scan.ctypes.data_as(C.c_void_p),
                                    tabs.ctypes.data_as(C.c_void_p), len(tabs), desc.ctypes.data_as(C.c_void_p), n,
                                    coeffs.ctypes.data_as(C.c_void_p), int(n_blocks), status.ctypes.data_as(C.c_void_p), int(sub_bits))
    if rc != 0:
        raise RuntimeError(f"avcer_jpeg_unpack_host failed: {rc}")
    return coeffs, status


# ---------------------------------------------------------------------------------------------------- numpy statement (tests)
def _idct_1d(v, shift):
    """csrc/jpeg.h idct_1d (libjpeg jidctint.c) along axis 0 of an int64 array [8, ...]."""
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


PAIR_MAX = 16383  # csrc/jpeg.h IDCT_PAIR_MAX


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
    """Kernels A and B of csrc/jpeg_decode.hip stated in numpy (for the tests; not a product path): the coefficient storage and the DESC
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
        self.files = None  # encode_images(entropy="device"): the files on their way to the host
        self.wire = None   # decode_*(entropy="device"): descriptors, scan records, tables and entropy-coded bytes, one copy
        self.event = None

    def reserve(self, blocks: int, n: int):
        if self.event is not None:
            self.event.synchronize()
        if self.coeffs is None or self.coeffs.numel() < 64 * blocks:
            self.coeffs = torch.empty(64 * (blocks + blocks // 4 + 1024), dtype=torch.int16, pin_memory=True)
        if self.desc is None or self.desc.numel() < DESC.itemsize * n:
            self.desc = torch.empty(DESC.itemsize * (n + n // 4 + 64), dtype=torch.uint8, pin_memory=True)

    def reserve_wire(self, nbytes: int):
        if self.event is not None:
            self.event.synchronize()
        if self.wire is None or self.wire.numel() < nbytes:
            self.wire = torch.empty(nbytes + nbytes // 4 + 4096, dtype=torch.uint8, pin_memory=True)
        return self.wire

    def reserve_files(self, nbytes: int):
        if self.files is None or self.files.numel() < nbytes:
            self.files = torch.empty(nbytes + nbytes // 4 + 4096, dtype=torch.uint8, pin_memory=True)
        return self.files


def _pil_rgb(blob: bytes) -> np.ndarray:
    from PIL import Image

    with Image.open(io.BytesIO(blob)) as img:
        return np.array(img.convert("RGB"))  # a copy: torch.from_numpy wants a writable array


def _pil_tile(blob: bytes) -> np.ndarray:
    """The lines of video_pipeline.read_face_dir."""
    from PIL import Image

    with Image.open(io.BytesIO(blob)) as img:
        return np.asarray(img.convert("RGB").resize((224, 224), Image.Resampling.NEAREST))


def _to_device(engine, blobs, threads: int, std_tables: bool = False):
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
        need = entropy_batch(engine.lib, blobs, coeffs, desc, threads, engine.ctx, std_tables=std_tables)
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


TABS_ROOM = 64  # tables a batch may carry before the staging is grown: a folder one encoder wrote carries four


def _to_device_unpacked(engine, blobs, threads: int, sub_bits: int = 0, std_tables: bool = False):
    """entropy="device": headers on the host (scan_batch; no bit stream is walked), ONE copy of descriptors, scan records, tables
    and entropy-coded bytes, avcer_jpeg_unpack -> (coeffs on the device, desc on the device, n_blocks, desc records on the host as the
    HEADERS left them, status i32 [n] on the device: what the device decode made of every file)."""
    st = engine.__dict__.setdefault("_jpeg_staging", _Staging())
    n = len(blobs)
    cap_bytes, cap_tabs = sum(len(b) for b in blobs) + 16 * n, TABS_ROOM
    while True:
        at_scan = DESC.itemsize * n
        at_tabs = at_scan + SCAN.itemsize * n
        at_data = at_tabs + TAB.itemsize * cap_tabs  # every part starts 16-byte aligned: 464, 48 and 288 are multiples of 16
        wire = st.reserve_wire(at_data + cap_bytes).numpy()
        desc, scan = wire[:at_scan].view(DESC), wire[at_scan:at_tabs].view(SCAN)
        n_tabs, need_bytes, _ = scan_batch(engine.lib, blobs, wire[at_data:at_data + cap_bytes], desc, scan,
                                           wire[at_tabs:at_data].view(TAB), threads, engine.ctx, std_tables=std_tables)
        if not (desc["reason"] == R_NO_SPACE).any():
            break
        cap_bytes, cap_tabs = max(cap_bytes, need_bytes), max(cap_tabs, n_tabs)
    host = desc.copy()
    used = int((desc["coef_block"] + desc["n_blocks"]).max()) if n else 0
    if used == 0:
        return None, None, 0, host, None
    ok = scan[desc["status"] == OK]
    n_bytes = int((ok["offset"] + ((ok["nbytes"] + 15) & ~15)).max())
    dev = engine.device
    w_dev = st.wire[:at_data + n_bytes].to(dev, non_blocking=True)
    st.event = torch.cuda.Event()
    st.event.record(torch.cuda.current_stream(dev))
    d_dev = w_dev[:at_scan]
    c_dev, status = engine.jpeg_unpack(w_dev[at_data:], w_dev[at_scan:at_tabs], w_dev[at_tabs:at_data], min(n_tabs, cap_tabs), d_dev, n, used,
                                       sub_bits)
    return c_dev, d_dev, used, host, status


def _flags_to_host(engine, flags, status=None):
    """Queues the copy of kernel A's per-file flags (i32 [n] on the device) into pinned memory and returns the function that
    waits for it and hands out the numpy array: the caller does its other host work in between.  With `status` (i32 [n] on the
    device, avcer_jpeg_unpack's) a file the device decode refused counts as flagged: the same copy, the same wait."""
    if status is not None:
        flags = flags | (status != OK).to(flags.dtype)
    host = torch.empty(flags.shape, dtype=flags.dtype, pin_memory=True)
    host.copy_(flags, non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(engine.device))

    def wait():
        done.synchronize()
        return host.numpy()

    return wait


def _check_entropy(entropy):
    if entropy not in ("host", "device"):
        raise ValueError(f'entropy must be "host" or "device", not {entropy!r}')


def decode_tiles(engine, blobs, threads: int = 0, entropy: str = "host", out=None):
    """The files `blobs` -> (tiles u8 [n,224,224,3] RGB on the device, paths): tile i is
    Image.open(file i).convert("RGB").resize((224, 224), NEAREST); paths[i] is "device" or "pil".
    entropy="device": the host parses the headers only and the files' bytes cross, avcer_jpeg_unpack Huffman-decodes them on the
    device (`threads` then serves the header pass); tiles and paths are the same.
    `out`: the tiles are written there and it is returned -- a contiguous u8 [n,224,224,3] on the engine's device, typically the
    slice buffer[a:a + n] of a larger tile buffer (video_corpus.run_video_corpus' pending tiles); nothing outside it is touched.
    Anything else raises ValueError before any work."""
    _check_entropy(entropy)
    n = len(blobs)
    if out is not None and not (torch.is_tensor(out) and tuple(out.shape) == (n, 224, 224, 3) and out.dtype == torch.uint8
                                and out.device == engine.device and out.is_contiguous()):
        raise ValueError(f"decode_tiles: out must be a contiguous uint8 [{n},224,224,3] on {engine.device}")
    tiles = torch.empty(n, 224, 224, 3, dtype=torch.uint8, device=engine.device) if out is None else out
    if n == 0:
        return tiles, []
    if entropy == "device":
        c_dev, d_dev, used, desc, refused = _to_device_unpacked(engine, blobs, threads)
    else:
        c_dev, d_dev, used, desc = _to_device(engine, blobs, threads)
        refused = None
    status = desc["status"].copy()
    flags = _flags_to_host(engine, engine.jpeg_tiles(c_dev, d_dev, n, used, out=tiles)[1], refused) if used else None
    # the files the parser refused go through PIL while the kernels run; only then the range guard of kernel A is read (the one
    # wait of this call: `paths` cannot be known before it), and a file it flagged follows them
    host = {i: _pil_tile(blobs[i]) for i in range(n) if status[i] != OK}
    if flags is not None:
        for i in np.nonzero(flags())[0]:
            if int(i) in host:  # refused by its header already
                continue
            status[i] = NOT_HANDLED
            host[int(i)] = _pil_tile(blobs[i])
    if host:
        rest = sorted(host)
        tiles[torch.as_tensor(rest, device=engine.device)] = torch.from_numpy(np.stack([host[i] for i in rest])).to(engine.device)
    return tiles, ["device" if s == OK else "pil" for s in status]


def decode_canvas(engine, blobs, threads: int = 0, entropy: str = "host"):
    """The files `blobs` at full size -> ((canvas u8 [max(n,1), max h, max w, 3] on the device, rects i32 [n,5] = (i, 0, 0, w, h)),
    paths): the layout of video_pipeline.read_face_crops, the input of Engine.crop_resize_linear.  `entropy`: as in decode_tiles."""
    _check_entropy(entropy)
    n = len(blobs)
    dev = engine.device
    if n == 0:
        return (torch.zeros(1, 1, 1, 3, dtype=torch.uint8, device=dev), np.zeros((0, 5), dtype=np.int32)), []
    if entropy == "device":
        c_dev, d_dev, used, desc, refused = _to_device_unpacked(engine, blobs, threads)
    else:
        c_dev, d_dev, used, desc = _to_device(engine, blobs, threads)
        refused = None
    status = desc["status"].copy()
    rest = {i: _pil_rgb(blobs[i]) for i in range(n) if status[i] != OK}
    sizes = [(rest[i].shape[1], rest[i].shape[0]) if i in rest else (int(desc["width"][i]), int(desc["height"][i])) for i in range(n)]
    wmax, hmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if used:
        canvas, flags = engine.jpeg_rgb(c_dev, d_dev, n, used, hmax, wmax)
        for i in np.nonzero(_flags_to_host(engine, flags, refused)())[0]:  # the range guard of kernel A; such a file's slot is zero so far
            if int(i) in rest:  # refused by its header already
                continue
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


def _pil_frame(blob, i: int, height: int, width: int, bgr: bool) -> np.ndarray:
    """Frame i through PIL, in the channel order asked for; OSError naming the frame where PIL cannot read it or reads another size."""
    try:
        img = _pil_rgb(blob)
    except Exception as e:  # PIL raises OSError and its subclasses, SyntaxError or ValueError on some broken files
        raise OSError(f"frame {i}: neither the device path nor PIL can read it ({type(e).__name__}: {e})") from e
    if img.shape[:2] != (height, width):
        two = bytes(blob).find(b"\xff\xd8", 2) >= 0 and 2 * img.shape[0] in (height, height - 1, height + 1)
        why = " -- two SOI markers: interlaced two-field Motion-JPEG (AVI1 field pairs) is not read" if two else ""
        raise OSError(f"frame {i}: a picture of {img.shape[1]} x {img.shape[0]}, the video is {width} x {height}{why}")
    return np.ascontiguousarray(img[:, :, ::-1]) if bgr else img


def decode_frames(engine, blobs, height: int, width: int, bgr: bool = True, entropy: str = "device", threads: int = 0,
                  frames_per_pass: int = 64, std_tables: bool = True):
    """The frames of a Motion-JPEG video (`avi.open_avi(path).frames`, or any n JPEG files of one size; bytes or buffers, nothing
    is copied in Python) -> (frames u8 [n, height, width, 3] on the device, paths): frame i is
    Image.open(file i).convert("RGB"), channels flipped with `bgr` (the order cv2 hands the reference, run_inference's frames_bgr);
    paths[i] is "device" or "pil".  The frames never exist on the host.
    Works in passes of at most `frames_per_pass` files, so coefficient and plane storage is that of a pass, not of the video; the
    result does not depend on `frames_per_pass`, `threads` or `entropy` ("device": the Huffman decode runs on the device too,
    avcer_jpeg_unpack; "host": avcer_jpeg_entropy_batch).  std_tables: a frame without DHT segments is decoded with the standard's
    annex-K tables (AVCER_JPEG_STD_TABLES), as Motion-JPEG producers mean it.
    A frame the device path reports -- header refused, flag 1 (range guard), flag 2 (another size) -- goes through PIL, as in
    decode_canvas; one PIL cannot read either, or reads at another size, raises OSError naming the frame index."""
    _check_entropy(entropy)
    n, height, width, per = len(blobs), int(height), int(width), int(frames_per_pass)
    if height <= 0 or width <= 0 or per <= 0:
        raise ValueError("decode_frames: height, width and frames_per_pass positive")
    dev = engine.device
    frames = torch.empty(n, height, width, 3, dtype=torch.uint8, device=dev)
    paths = []

    def settle(lo, part, status, wait):
        """The pass behind the one just queued: its flags are read now, and what the device did not decode goes through PIL."""
        flagged = wait() if wait is not None else np.ones(len(part), dtype=np.int32)
        rest = [k for k in range(len(part)) if status[k] != OK or flagged[k]]
        if rest:
            host = np.stack([_pil_frame(part[k], lo + k, height, width, bgr) for k in rest])
            frames[torch.as_tensor([lo + k for k in rest], device=dev)] = torch.from_numpy(host).to(dev)
        paths.extend("pil" if (status[k] != OK or flagged[k]) else "device" for k in range(len(part)))

    behind = None
    for lo in range(0, n, per):
        part = blobs[lo:lo + per]
        if entropy == "device":
            c_dev, d_dev, used, desc, refused = _to_device_unpacked(engine, part, threads, std_tables=std_tables)
        else:
            c_dev, d_dev, used, desc = _to_device(engine, part, threads, std_tables=std_tables)
            refused = None
        wait = None
        if used:
            wait = _flags_to_host(engine, engine.jpeg_frames(c_dev, d_dev, len(part), used, height, width, bgr=bgr, out=frames[lo:lo + len(part)])[1],
                                  refused)
        if behind is not None:
            settle(*behind)
        behind = (lo, part, desc["status"].copy(), wait)
    if behind is not None:
        settle(*behind)
    return frames, paths


# ==================================================================================================== encoding
# The mirror image of the above (include/avcer_hip.h "JPEG face crops", encoding): the device computes the quantised coefficients
# of every image (colour conversion, chroma downsampling, forward DCT, quantisation: avcer_jpeg_forward), the host writes the
# files (avcer_jpeg_write_batch: headers, Huffman coding) -- or, with entropy="device", the device does (avcer_jpeg_pack) and only
# the files cross to the host.  The contract is byte-identity with
# PIL.Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=subsampling) (libjpeg-turbo, standard Huffman tables).
HEADER_BYTES = 623  # csrc/jpeg.h: SOI, APP0, two DQT, SOF0, four DHT, SOS
R_ENC_SIZE = 18  # csrc/jpeg.h: an image of zero width or height, or of more than 65535 pixels a side

# libjpeg's jcparam.c: the two tables of the standard's annex K in natural order
_STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72,
                      92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
_STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                        99, 99, 99] + [99] * 32, dtype=np.int64)
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}  # PIL's `subsampling` -> the luma sampling factors (hs, vs); chroma is 1 x 1


def quant_tables_numpy(quality: int) -> np.ndarray:
    """jpeg_set_quality(quality, force_baseline): u16 [2, 64], luma and chroma, natural order (avcer_jpeg_quant_tables)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (_STD_LUMA, _STD_CHROMA)]).astype(np.uint16)


def plan_numpy(sizes, quality: int, subsampling: int) -> np.ndarray:
    """avcer_jpeg_plan in numpy: DESC records of images of `sizes` [(w, h)] (tests; the product path calls the library)."""
    hs, vs = SAMPLING[int(subsampling)]
    qt = quant_tables_numpy(quality)
    desc = np.zeros(len(sizes), dtype=DESC)
    at = 0
    for d, (w, h) in zip(desc, sizes):
        d["width"], d["height"], d["ncomp"], d["hs"], d["vs"] = w, h, 3, hs, vs
        d["coef_block"] = at
        if not (0 < w <= 65535 and 0 < h <= 65535):
            d["status"], d["reason"] = NOT_HANDLED, R_ENC_SIZE
            continue
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        d["bw"], d["bh"], d["tq"] = (mx * hs, mx, mx), (my * vs, my, my), (0, 1, 1)
        d["qt"][0], d["qt"][1], d["qt"][2] = qt[0], qt[1], qt[1]
        d["n_blocks"] = mx * my * (hs * vs + 2)
        at += int(d["n_blocks"])
    return desc


def _fdct_1d(d, first):
    """libjpeg's jfdctint.c (jpeg_fdct_islow), one 1-D pass along axis 0 of an int64 array [8, ...]: 13-bit constants; the first pass
    leaves its results scaled up by 2^PASS1_BITS = 4, the second takes that out again (and leaves the factor 8 of the 2-D DCT)."""
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = 11 if first else 15
    ds = lambda x: (x + (1 << (sh - 1))) >> sh
    o0, o4 = ((tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2) if first else ((tmp10 + tmp11 + 2) >> 2, (tmp10 - tmp11 + 2) >> 2)
    z1 = (tmp12 + tmp13) * 4433
    o2, o6 = ds(z1 + tmp13 * 6270), ds(z1 + tmp12 * (-15137))
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return np.stack([o0, ds(tmp7 + z1 + z4), o2, ds(tmp6 + z2 + z3), o4, ds(tmp5 + z2 + z4), o6, ds(tmp4 + z1 + z3)])


def _forward_plane(p, qt):
    """A sample plane u8-valued [8 bh, 8 bw] -> quantised blocks int16 [bh, bw, 64] (natural order): minus 128, rows, columns, then
    jcdctmgr.c's division by 8 q, halves rounded away from zero."""
    bh, bw = p.shape[0] // 8, p.shape[1] // 8
    x = p.astype(np.int64).reshape(bh, 8, bw, 8).transpose(3, 0, 2, 1) - 128   # [col, bh, bw, row]
    x = _fdct_1d(x, True)                                                      # [u, bh, bw, row]
    x = _fdct_1d(x.transpose(3, 1, 2, 0), False)                               # [v, bh, bw, u]
    x = x.transpose(1, 2, 0, 3).reshape(bh, bw, 64)
    q8 = qt.astype(np.int64).reshape(1, 1, 64) * 8
    return (np.sign(x) * ((np.abs(x) + (q8 >> 1)) // q8)).astype(np.int16)


def _edge(a, rows, cols):
    """`a` with its last row and column repeated out to [rows, cols]."""
    return a[np.minimum(np.arange(rows), a.shape[0] - 1)][:, np.minimum(np.arange(cols), a.shape[1] - 1)]


def forward_numpy(images, quality: int = 95, subsampling: int = 2):
    """avcer_jpeg_forward stated in numpy (for the tests; not a product path): RGB images u8 [h, w, 3] -> (coefficients int16
    [blocks, 64] in the layout of avcer_jpeg_entropy_batch, DESC records).  libjpeg's forward path: jccolor.c (16-bit fixed point),
    jcsample.c (box filter, alternating bias), jcprepct.c's edges, jfdctint.c, jcdctmgr.c, and jccoefct.c's dummy blocks."""
    desc = plan_numpy([(im.shape[1], im.shape[0]) for im in images], quality, subsampling)
    out = np.zeros((int((desc["coef_block"] + desc["n_blocks"]).max()) if len(desc) else 0, 64), dtype=np.int16)
    for im, d in zip(images, desc):
        if d["status"] != OK:
            continue
        h, w = im.shape[:2]
        hs, vs = int(d["hs"]), int(d["vs"])
        r, g, b = (im[..., c].astype(np.int64) for c in range(3))
        y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
        cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
        cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
        at = int(d["coef_block"])
        bw, bh = int(d["bw"][0]), int(d["bh"][0])
        yb = _forward_plane(_edge(y, 8 * bh, 8 * bw), d["qt"][0])
        # dummy blocks -- those that only pad the component to whole MCUs: no AC, the DC of the block coded before them in the MCU.
        # A real row's dummy (the odd column past the last real one) follows its left neighbour; a dummy row (the odd row past the
        # last real one) takes, in every block, the DC of the LAST block of the row above in its MCU
        wb, hb = -(-w // 8), -(-h // 8)
        for by in range(bh):
            for bx in range(bw):
                if by < hb and bx < wb:
                    continue
                sy, sx = (by, bx - 1) if by < hb else (by - 1, bx // hs * hs + hs - 1)
                sx -= sx >= wb
                yb[by, bx] = 0
                yb[by, bx, 0] = yb[sy, sx, 0]
        out[at:at + bw * bh] = yb.reshape(-1, 64)
        at += bw * bh
        cw, chh = int(d["bw"][1]), int(d["bh"][1])
        for c, p in ((1, cb), (2, cr)):
            # jcprepct.c: the last input row is repeated only to complete the row group (an odd height under 4:2:0), the last
            # DOWNSAMPLED row is then repeated down to the MCU; columns are repeated before downsampling (expand_right_edge)
            p = _edge(p, h + (h % vs), 8 * cw * hs)
            if hs == 2 and vs == 1:
                p = (p[:, 0::2] + p[:, 1::2] + (np.arange(8 * cw) & 1)[None]) >> 1
            elif hs == 2:
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + (1 + (np.arange(8 * cw) & 1))[None]) >> 2
            out[at:at + cw * chh] = _forward_plane(_edge(p, 8 * chh, 8 * cw), d["qt"][c]).reshape(-1, 64)
            at += cw * chh
    return out, desc


def quant_tables(lib, quality: int) -> np.ndarray:
    """avcer_jpeg_quant_tables: u16 [2, 64], luma and chroma, natural order."""
    qt = np.zeros((2, 64), dtype=np.uint16)
    rc = lib.avcer_jpeg_quant_tables(int(quality), qt.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"avcer_jpeg_quant_tables({quality}) failed: {rc}")
    return qt


def plan(lib, sizes, quality: int = 95, subsampling: int = 2, desc: np.ndarray | None = None):
    """avcer_jpeg_plan: image sizes [(w, h)] -> (DESC records, written into `desc[:n]` when given; the blocks they need together)."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
    n = len(sizes)
    desc = np.zeros(n, dtype=DESC) if desc is None else desc
    assert desc.dtype == DESC and desc.flags.c_contiguous and len(desc) >= n
    need = C.c_int64(0)
    rc = lib.avcer_jpeg_plan(sizes.ctypes.data_as(C.c_void_p), n, int(subsampling), int(quality), desc.ctypes.data_as(C.c_void_p),
                             C.byref(need))
    if rc != 0:
        raise ValueError(f"avcer_jpeg_plan failed: {rc} (quality {quality} in 1..100, subsampling {subsampling} in 0, 1, 2)")
    return desc[:n], int(need.value)


def write_batch(lib, coeffs: np.ndarray, desc: np.ndarray, out: np.ndarray, threads: int = 0, ctx=None, cap_bytes: int | None = None):
    """avcer_jpeg_write_batch: the coefficient storage and DESC records -> the files back to back in `out` (u8, room for `cap_bytes`,
    default all of it).  Returns (offsets i64 [n + 1], the bytes all files need together); `desc` gets the status and reason of a
    file that was not written."""
    n = len(desc)
    cap = out.size if cap_bytes is None else int(cap_bytes)
    assert coeffs.dtype == np.int16 and coeffs.flags.c_contiguous and desc.dtype == DESC and desc.flags.c_contiguous
    assert out.dtype == np.uint8 and out.flags.c_contiguous and cap <= out.size
    offsets = np.zeros(n + 1, dtype=np.int64)
    need = C.c_int64(0)
    rc = lib.avcer_jpeg_write_batch(ctx, coeffs.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), n,
                                    out.ctypes.data_as(C.c_void_p), cap, offsets.ctypes.data_as(C.c_void_p), host_threads(int(threads)),
                                    C.byref(need))
    if rc != 0:
        raise RuntimeError(f"avcer_jpeg_write_batch failed: {rc}")
    return offsets, int(need.value)


def _encode_rects(src, rects) -> np.ndarray:
    """`rects` as int32 [n,5] = (slot, x0, y0, x1, y1), checked against `src` [N,H,W,3]: a zero-area rectangle or one that leaves
    its frame raises ValueError naming the image."""
    r = np.ascontiguousarray(np.asarray(rects.cpu() if torch.is_tensor(rects) else rects, dtype=np.int64).reshape(-1, 5))
    n_src, h, w = (int(v) for v in src.shape[:3])
    for i, (slot, x0, y0, x1, y1) in enumerate(r):
        if x1 <= x0 or y1 <= y0:
            raise ValueError(f"image {i}: empty rectangle ({x0}, {y0}, {x1}, {y1})")
        if not (0 <= slot < n_src and 0 <= x0 and x1 <= w and 0 <= y0 and y1 <= h):
            raise ValueError(f"image {i}: rectangle ({x0}, {y0}, {x1}, {y1}) of slot {slot} leaves the source [{n_src},{h},{w},3]")
    return r.astype(np.int32)


def _not_written(status, reason):
    i = int(np.nonzero(status != OK)[0][0])
    return RuntimeError(f"image {i} was not written: reason {int(reason[i])} (csrc/jpeg.h R_*)")


def _pack_to_host(engine, st, coeffs, d_dev, n: int, blocks: int) -> list:
    """The device entropy coder behind avcer_jpeg_forward: avcer_jpeg_pack, then offsets and statuses to the host, then exactly the
    bytes of the files through the pinned staging of the engine."""
    dev = engine.device
    cap = HEADER_BYTES * n + 40 * blocks  # the guess of the host path; repeated once with what the files need when it was short
    small = torch.empty(2 * n + 2, dtype=torch.int64, pin_memory=True)  # offsets [n + 1], bytes_needed, status [n] as i32 pairs
    for attempt in range(2):
        out, offsets, status, need = engine.jpeg_pack(coeffs, d_dev, n, blocks, cap)
        small[:n + 1].copy_(offsets, non_blocking=True)
        small[n + 1:n + 2].copy_(need, non_blocking=True)
        s_host = small[n + 2:].view(torch.int32)[:n]
        s_host.copy_(status, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        offs, reason = small[:n + 1].numpy(), s_host.numpy()
        if attempt == 0 and (reason == R_NO_SPACE).any():
            cap = int(small[n + 1])
            continue
        break
    if (reason != OK).any():
        raise _not_written(reason, reason)
    total = int(offs[n])
    host = st.reserve_files(total)
    host[:total].copy_(out[:total], non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    blob = host.numpy()
    return [blob[offs[i]:offs[i + 1]].tobytes() for i in range(n)]


def _plan_to_device(engine, src, rects, quality, subsampling):
    """What every call that cuts images out of `src` does first: the checks, avcer_jpeg_plan on the host, source, rectangles and
    descriptors on the device.  Returns None for no image, else (src, rects i32 [n,5], descriptors as bytes) on the device, the
    DESC records on the host, n, the blocks of the plan, and the engine's staging."""
    src = src if torch.is_tensor(src) else torch.from_numpy(np.array(src))  # a copy: torch.from_numpy wants a writable array
    if src.dim() != 4 or src.shape[-1] != 3 or src.dtype != torch.uint8:
        raise ValueError("src must be uint8 [N,H,W,3]")
    r = _encode_rects(src, rects)
    n = len(r)
    if n == 0:
        return None
    dev = engine.device
    st = engine.__dict__.setdefault("_jpeg_staging", _Staging())
    sizes = np.stack([r[:, 3] - r[:, 1], r[:, 4] - r[:, 2]], axis=1)
    st.reserve(int(((sizes[:, 0].astype(np.int64) + 15) // 8 * ((sizes[:, 1] + 15) // 8)).sum()) * 3, n)  # an upper bound of the plan
    desc, blocks = plan(engine.lib, sizes, quality, subsampling, st.desc.numpy()[:DESC.itemsize * n].view(DESC))
    if (desc["status"] != OK).any():
        i = int(np.nonzero(desc["status"] != OK)[0][0])
        raise ValueError(f"image {i}: {int(desc['width'][i])} x {int(desc['height'][i])} pixels cannot be a JPEG file (1..65535 a side)")
    host = desc.copy()
    d_dev = st.desc[:DESC.itemsize * n].to(dev, non_blocking=True)
    r_dev = torch.from_numpy(r).to(dev)
    return src.to(dev).contiguous(), r_dev, d_dev, host, n, blocks, st


def files_from_coeffs(engine, coeffs, d_dev, host: np.ndarray, threads: int = 0, entropy: str = "host") -> list:
    """The entropy-coding half of encode_images: coefficients int16 [>= 64 * blocks] on the device as avcer_jpeg_forward (or a
    round trip with keep_coeffs) left them, their descriptors on the device (`d_dev`) and on the host (`host`, DESC records) -> the
    n files as bytes."""
    _check_entropy(entropy)
    dev = engine.device
    st = engine.__dict__.setdefault("_jpeg_staging", _Staging())
    n = len(host)
    blocks = int((host["coef_block"] + host["n_blocks"]).max()) if n else 0
    if n == 0:
        return []
    if entropy == "device":
        st.event = torch.cuda.Event()  # the descriptors were copied out of the pinned staging
        st.event.record(torch.cuda.current_stream(dev))
        return _pack_to_host(engine, st, coeffs, d_dev, n, blocks)
    st.reserve(blocks, n)
    st.coeffs[:64 * blocks].copy_(coeffs[:64 * blocks], non_blocking=True)
    st.event = torch.cuda.Event()
    st.event.record(torch.cuda.current_stream(dev))
    st.event.synchronize()  # the coefficients are on the host: the one wait of this call
    c_host = st.coeffs.numpy()[:64 * blocks]
    # a block of a photograph costs some 17 bytes at quality 95 (untouched pages of the buffer cost nothing); grow and repeat when
    # the guess was short
    out = np.empty(HEADER_BYTES * n + 40 * blocks, dtype=np.uint8)
    while True:
        d = host.copy()
        offsets, need = write_batch(engine.lib, c_host, d, out, threads, engine.ctx)
        if not (d["reason"] == R_NO_SPACE).any():
            break
        out = np.empty(need, dtype=np.uint8)
    if (d["status"] != OK).any():
        raise _not_written(d["status"], d["reason"])
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)]


def encode_images(engine, src, rects, bgr: bool = False, quality: int = 95, subsampling: int = 2, threads: int = 0,
                  entropy: str = "host") -> list:
    """JPEG files of n images cut out of `src` (u8 [N,H,W,3], moved to the device if it is not there): image i is the half-open
    rectangle rects[i] = (slot, x0, y0, x1, y1).  Returns the n files as bytes, byte-identical to
    PIL.Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=subsampling).  plan (host) -> descriptors to the device
    -> avcer_jpeg_forward -> coefficients into the pinned staging of the engine -> avcer_jpeg_write_batch (host threads).
    entropy="device": the coefficients stay where they are, avcer_jpeg_pack writes the files on the device and only their bytes
    cross (`threads` is then unused); the files are the same."""
    _check_entropy(entropy)
    planned = _plan_to_device(engine, src, rects, quality, subsampling)
    if planned is None:
        return []
    src_d, r_dev, d_dev, host, n, blocks, _ = planned
    coeffs = engine.jpeg_forward(src_d, r_dev, d_dev, n, blocks, bgr=bgr)
    return files_from_coeffs(engine, coeffs, d_dev, host, threads, entropy)


# ==================================================================================================== the round trip
# What stage 1 of the reference sees of a face crop is the JPEG file stage 0 wrote of it, read back (include/avcer_hip.h "The round
# trip without the file").  Huffman coding is lossless, so that picture is decode(encode(crop)) = the pixel pass of the decoder on
# the coefficients of the encoder's forward pass: no file, no entropy pass.  cv2 is not among this project's dependencies: the claim
# is identity with PIL on both sides (libjpeg-turbo, the defaults cv2.imwrite uses: quality 95, 4:2:0).
def roundtrip_numpy(images, quality: int = 95, subsampling: int = 2):
    """The CPU statement of the round trip (for the tests; not a product path): RGB images u8 [h, w, 3] -> per image
    Image.open(the file Image.save(..., "JPEG", quality, subsampling) writes of it).convert("RGB"), u8 [h, w, 3]."""
    return pixels_numpy(*forward_numpy(images, quality, subsampling))


def check_roundtrip_options(lib, quality, subsampling):
    """ValueError for a quality or a subsampling avcer_jpeg_plan refuses (asked of the call itself, with no image)."""
    plan(lib, np.zeros((0, 2), dtype=np.int32), quality, subsampling)


def _roundtrip(engine, src, rects, bgr, quality, subsampling, keep_coeffs, launch):
    check_roundtrip_options(engine.lib, quality, subsampling)
    planned = _plan_to_device(engine, src, rects, quality, subsampling)
    if planned is None:
        return None
    src_d, r_dev, d_dev, host, n, blocks, st = planned
    out, flags, coeffs = launch(src_d, r_dev, d_dev, host, n, blocks)
    st.event = torch.cuda.Event()  # the descriptors were copied out of the pinned staging
    st.event.record(torch.cuda.current_stream(engine.device))
    # the one wait of the call.  An encoder's own coefficients cannot leave the inverse DCT's range (include/avcer_hip.h): a flag is
    # an error of this library, and a zero tile must not reach a network as if it were a face
    bad = np.nonzero(_flags_to_host(engine, flags)())[0]
    if len(bad):
        raise RuntimeError(f"image {int(bad[0])}: the JPEG round trip left the range of the inverse DCT (flag 1, include/avcer_hip.h)")
    return out, coeffs, d_dev, host


def roundtrip_tiles(engine, src, rects, bgr: bool = False, quality: int = 95, subsampling: int = 2, keep_coeffs: bool = False):
    """n images cut out of `src` (u8 [N,H,W,3]; image i is the half-open rectangle rects[i] = (slot, x0, y0, x1, y1)) as their JPEG
    files would read back: tiles u8 [n,224,224,3] RGB on the device, tile i bit-identical to
    decode_tiles(engine, encode_images(engine, src, rects, bgr, quality, subsampling))[0][i] -- to
    Image.open(file).convert("RGB").resize((224, 224), NEAREST) of the file PIL writes of the image.  One fused kernel (forward DCT,
    quantisation, dequantisation, inverse DCT per block) and the decoder's pixel kernel; no file, no entropy pass, and the
    coefficients stay on the chip.
    keep_coeffs: returns (tiles, coeffs, d_dev, desc) instead -- the quantised coefficients int16 [64 * blocks] on the device exactly
    as avcer_jpeg_forward stores them, with their descriptors on the device and on the host: files_from_coeffs writes the files
    from them without a second forward pass.
    A quality or subsampling avcer_jpeg_plan refuses, an empty rectangle or one that leaves its frame: ValueError before any launch."""
    got = _roundtrip(engine, src, rects, bgr, quality, subsampling, keep_coeffs,
                     lambda s, r, d, host, n, blocks: engine.jpeg_roundtrip_tiles(s, r, d, n, blocks, bgr=bgr, keep_coeffs=keep_coeffs))
    if got is None:
        tiles = torch.empty(0, 224, 224, 3, dtype=torch.uint8, device=engine.device)
        return (tiles, torch.empty(0, dtype=torch.int16, device=engine.device), None, np.zeros(0, dtype=DESC)) if keep_coeffs else tiles
    return got if keep_coeffs else got[0]


def roundtrip_canvas(engine, src, rects, bgr: bool = False, quality: int = 95, subsampling: int = 2, keep_coeffs: bool = False):
    """The full-size twin of roundtrip_tiles: (canvas u8 [max(n,1), max h, max w, 3] RGB on the device, rects i32 [n,5] = (i, 0, 0, w,
    h)) in the layout of decode_canvas, image i bit-identical to Image.open(file).convert("RGB"); with keep_coeffs
    ((canvas, rects), coeffs, d_dev, desc)."""
    def launch(s, r, d, host, n, blocks):
        return engine.jpeg_roundtrip_rgb(s, r, d, n, blocks, int(host["height"].max()), int(host["width"].max()), bgr=bgr,
                                         keep_coeffs=keep_coeffs)

    got = _roundtrip(engine, src, rects, bgr, quality, subsampling, keep_coeffs, launch)
    if got is None:
        out = (torch.zeros(1, 1, 1, 3, dtype=torch.uint8, device=engine.device), np.zeros((0, 5), dtype=np.int32))
        return (out, torch.empty(0, dtype=torch.int16, device=engine.device), None, np.zeros(0, dtype=DESC)) if keep_coeffs else out
    canvas, coeffs, d_dev, host = got
    out = (canvas, np.array([(i, 0, 0, int(d["width"]), int(d["height"])) for i, d in enumerate(host)], dtype=np.int32).reshape(-1, 5))
    return (out, coeffs, d_dev, host) if keep_coeffs else out
