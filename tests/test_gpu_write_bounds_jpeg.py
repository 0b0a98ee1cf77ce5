"""Guard bands (tests/guard_band.py) around every output of the JPEG entries on the device: only the output is written, all of it,
the same bits in every run, the inputs unchanged.  These are the entries whose extents depend on the DATA -- file lengths from a
prefix sum over code lengths and byte stuffing, run lengths out of malformed streams, MCU-padded geometry with dummy blocks --
and every mask here comes from the host statement of the same operation (avcer_jpeg_write_batch's offsets, avcer_jpeg_entropy_batch's
verdicts and block ranges, avcer_jpeg_plan's geometry), never from what the device call returned.  The VALUES are the business of
tests/test_gpu_jpeg*.py; they are compared here where the host statement is at hand anyway.  Scratch inside the context's JPEG
workspace (212 bytes a block for the writer, the reader's unstuffed bytes, the round trips' component planes) cannot be guarded
from outside.

Entries and the edge each case was chosen for:
  avcer_jpeg_pack              the crafted set of tests/jpeg_pack_cases.py and three noise images at quality 100 (FF 00 stuffing), one
                               per subsampling, sides no multiples of 16; out / offsets / status / bytes_needed at three capacities:
                               4096 bytes of room (the tail is a gap), one byte short (the last codable file has no bytes: a gap
                               from the host writer's offsets[n] on), and one byte into a middle file
  avcer_jpeg_unpack            golden, crafted and all defects of tests/jpeg_unpack_cases.py in one batch (104 of 121 files are OK,
                               14 % of the blocks belong to refused files), sub_bits 128 and 0: the blocks of OK files must be written, those of
                               files the host pass refuses MAY be -- the header: "every OK file's blocks are written, zeros
                               included", and not a word about the others -- nothing else; status; desc changes in status and
                               reason alone
  avcer_jpeg_forward           nine rectangles of 1 x 1 to 52 x 37 in a two-slot source, slot 1's at odd x0, RGB and BGR, per
                               subsampling: coeffs fully written, dummy blocks included
  avcer_jpeg_roundtrip_tiles / _rgb   the same, without and with `coeffs` (then bit-identical to avcer_jpeg_forward's); with a
                               descriptor the plan did not write: zeros, flag 1, and its coefficients avcer_jpeg_forward's
  avcer_jpeg_tiles / _rgb      the supported golden files, a NOT_HANDLED descriptor and the corrupt-table file: every tile and the
                               whole canvas written, zeros where the header says zeros; hmax, wmax odd and larger than every image"""
import functools

import numpy as np
import pytest
import torch

import jpeg_pack_cases as pack_cases
import jpeg_unpack_cases as unpack_cases
from avcer_amd import jpeg
from avcer_amd.engine import _ptr
from guard_band import Band, check

pytestmark = pytest.mark.gpu


def _call(engine, name, *args):
    engine._check(getattr(engine.lib, name)(engine.ctx, *args, engine._stream()))


def _dev(engine, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.uint8) if a.dtype.fields else a).reshape(-1).copy()).to(engine.device)


# ----------------------------------------------------------------------------- avcer_jpeg_pack
@pytest.fixture(scope="module")
def pack_set(engine):
    """(coefficients [blocks, 64], DESC records, and the host writer's offsets with room for everything)."""
    _, coeffs, desc, _ = pack_cases.crafted(engine.lib)
    parts, descs, at = [coeffs], [desc], len(coeffs)
    for sub, (w, h) in enumerate(((17, 13), (33, 19), (41, 23))):
        c, d = jpeg.forward_numpy([np.random.default_rng(100 + sub).integers(0, 256, (h, w, 3), dtype=np.uint8)], 100, sub)
        d = d.copy()
        d["coef_block"] += at
        at += len(c)
        parts.append(c)
        descs.append(d)
    coeffs, desc = np.concatenate(parts), np.concatenate(descs)
    blobs, offsets, status, need = pack_cases.host_write(engine.lib, coeffs, desc)
    assert need == offsets[-1] and sum(pack_cases.stuffed_bytes(b) for b in blobs[-3:]) >= 3 and not status[-3:].any()
    return coeffs, desc, offsets


@pytest.mark.parametrize("which", ["room", "one byte short", "inside a middle file"])
def test_jpeg_pack(engine, pack_set, which):
    coeffs, desc, full = pack_set
    n, blocks, need = len(desc), len(coeffs), int(full[-1])
    cap = {"room": need + 4096, "one byte short": need - 1, "inside a middle file": int(full[n // 2]) + 1}[which]
    blobs, offsets, status, hneed = pack_cases.host_write(engine.lib, coeffs, desc, cap=cap)
    end = int(offsets[-1])
    assert hneed == need and end <= cap and (which == "room") == (end == need)
    if which == "one byte short":
        last = max(i for i in range(n) if len(blobs[i]) or status[i] == pack_cases.R_NO_SPACE)
        assert status[last] == pack_cases.R_NO_SPACE and blobs[last] == b"" and (status == pack_cases.R_NO_SPACE).sum() == 1
    if which == "inside a middle file":
        assert full[n // 2 + 1] > full[n // 2] and status[n // 2] == pack_cases.R_NO_SPACE
    c_dev, d_dev = _dev(engine, coeffs), _dev(engine, desc)
    written = torch.zeros(cap, dtype=torch.bool)
    written[:end] = True
    bands = [Band("out", (cap,), torch.uint8, written=written, row_bytes=1024), Band("offsets", (n + 1,), torch.int64, row_bytes=8),
             Band("status", (n,), torch.int32, row_bytes=4), Band("bytes_needed", (1,), torch.int64)]

    def run(outs):
        _call(engine, "avcer_jpeg_pack", _ptr(c_dev), blocks, _ptr(d_dev), n, _ptr(outs[0]), cap, _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]))

    out, goff, gstatus, gneed = check(run, bands, [c_dev, d_dev], device=engine.device)
    np.testing.assert_array_equal(goff.numpy(), offsets)
    np.testing.assert_array_equal(gstatus.numpy(), status)
    assert int(gneed[0]) == need
    assert out.numpy()[:end].tobytes() == b"".join(blobs)


# ----------------------------------------------------------------------------- avcer_jpeg_unpack
@pytest.fixture(scope="module")
def unpack_set(engine):
    """golden + crafted + defects: the scanned batch, the host pass's DESC records and the block masks they give.  No defects
    entry had to be left out for the condition (at least half the files OK, less than half the blocks under `may`)."""
    files = unpack_cases.golden()
    crafted, _, _ = unpack_cases.crafted(engine.lib)
    blobs = [b for _, b in files + crafted] + [b for _, b, _ in unpack_cases.defects(files)]
    _, want = unpack_cases.oracle(engine.lib, blobs)
    s = unpack_cases.scanned(engine.lib, blobs)
    ok, header = want["status"] == jpeg.OK, s["desc"]["status"] == jpeg.OK
    assert not (ok & ~header).any()
    for f in ("coef_block", "n_blocks"):
        np.testing.assert_array_equal(s["desc"][f][header], want[f][header])
    written, may = (torch.zeros(s["need_blocks"], 1, dtype=torch.bool) for _ in range(2))
    for i in np.nonzero(header)[0]:
        a, k = int(want["coef_block"][i]), int(want["n_blocks"][i])
        (written if ok[i] else may)[a:a + k] = True
    assert 2 * int(ok.sum()) >= len(blobs) and 2 * int(may.sum()) < s["need_blocks"] and int(may.sum()) > 0
    assert not (written & may).any() and bool((written | may).all())
    return s, want, written, may


@pytest.mark.parametrize("sub_bits", unpack_cases.SUB_BITS)
def test_jpeg_unpack(engine, unpack_set, sub_bits):
    s, want, written, may = unpack_set
    n, blocks = len(want), int(s["need_blocks"])
    data, scan, tabs = _dev(engine, s["data"][:s["need_bytes"]]), _dev(engine, s["scan"]), _dev(engine, s["tabs"][:s["n_tabs"]])
    pristine = _dev(engine, s["desc"])
    size = jpeg.DESC.itemsize
    bands = [Band("coeffs", (blocks, 64), torch.int16, written=written, may=may), Band("status", (n,), torch.int32, row_bytes=4),
             Band("desc", (n, size), torch.uint8)]

    def run(outs):
        outs[2].copy_(pristine.view(n, size))           # updated in place: every call starts from the host's records
        _call(engine, "avcer_jpeg_unpack", _ptr(data), int(data.numel()), _ptr(scan), _ptr(tabs), int(s["n_tabs"]), _ptr(outs[2]), n,
              _ptr(outs[0]), blocks, _ptr(outs[1]), sub_bits)

    _, status, desc = check(run, bands, [data, scan, tabs, pristine], device=engine.device)
    got = desc.numpy().reshape(-1).view(jpeg.DESC)
    np.testing.assert_array_equal(status.numpy(), want["status"])
    for f in jpeg.DESC.names:
        np.testing.assert_array_equal(got[f], want[f] if f in ("status", "reason") else s["desc"][f], err_msg=f)


# ----------------------------------------------------------------------------- avcer_jpeg_forward and the round trips
RECTS = np.array([[0, 0, 0, 1, 1], [0, 3, 2, 10, 11], [0, 16, 8, 32, 24], [0, 40, 5, 57, 38], [0, 10, 25, 62, 62],       # 1x1 7x9 16x16 17x33 52x37
                  [1, 1, 0, 10, 7], [1, 5, 3, 38, 20], [1, 41, 1, 78, 53], [1, 79, 63, 80, 64]], dtype=np.int32)          # 9x7 33x17 37x52 1x1
HMAX, WMAX = 59, 61


@functools.lru_cache(maxsize=None)
def _source():
    a = np.random.default_rng(77).integers(0, 256, (2, 64, 80, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _plan(engine, sub, edit=None):
    desc, blocks = jpeg.plan(engine.lib, [(r[3] - r[1], r[4] - r[2]) for r in RECTS], 95, sub)
    assert (desc["status"] == jpeg.OK).all() and blocks == int(desc["n_blocks"].sum())
    if edit is not None:
        desc["qt"][edit, 2, 5] += 1        # the two chroma tables differ: avcer_jpeg_plan never writes that; the geometry is left alone
    return desc, blocks


@pytest.mark.parametrize("bgr", [0, 1], ids=["rgb", "bgr"])
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_jpeg_forward_and_round_trips(engine, sub, bgr):
    dev = engine.device
    desc, blocks = _plan(engine, sub)
    n = len(RECTS)
    src, rects, d_dev = torch.from_numpy(_source().copy()).to(dev), torch.from_numpy(RECTS.copy()).to(dev), _dev(engine, desc)
    inputs = [src, rects, d_dev]
    head = (_ptr(src), 2, 64, 80, _ptr(rects), _ptr(d_dev), n, bgr)
    coeffs = Band("coeffs", (blocks, 64), torch.int16)
    flags, tiles = Band("flags", (n,), torch.int32, row_bytes=4), Band("tiles", (n, 224, 224, 3), torch.uint8, row_bytes=672)
    canvas = Band("canvas", (n, HMAX, WMAX, 3), torch.uint8, row_bytes=3 * WMAX)

    fwd, = check(lambda outs: _call(engine, "avcer_jpeg_forward", *head, _ptr(outs[0]), blocks), [coeffs], inputs, device=dev)
    images = [_source()[s, y0:y1, x0:x1, ::-1 if bgr else 1] for s, x0, y0, x1, y1 in RECTS]
    np.testing.assert_array_equal(fwd.numpy(), jpeg.forward_numpy(images, 95, sub)[0])

    f1, t1 = check(lambda outs: _call(engine, "avcer_jpeg_roundtrip_tiles", *head, None, blocks, _ptr(outs[0]), _ptr(outs[1])),
                   [flags, tiles], inputs, device=dev)
    f2, t2, c2 = check(lambda outs: _call(engine, "avcer_jpeg_roundtrip_tiles", *head, _ptr(outs[2]), blocks, _ptr(outs[0]), _ptr(outs[1])),
                       [flags, tiles, coeffs], inputs, device=dev)
    assert torch.equal(c2, fwd) and torch.equal(t1, t2) and not f1.any() and not f2.any() and all(t1[i].any() for i in range(1, 8))

    f3, v1 = check(lambda outs: _call(engine, "avcer_jpeg_roundtrip_rgb", *head, None, blocks, _ptr(outs[0]), _ptr(outs[1]), HMAX, WMAX),
                   [flags, canvas], inputs, device=dev)
    f4, v2, c4 = check(lambda outs: _call(engine, "avcer_jpeg_roundtrip_rgb", *head, _ptr(outs[2]), blocks, _ptr(outs[0]), _ptr(outs[1]), HMAX,
                                          WMAX), [flags, canvas, coeffs], inputs, device=dev)
    assert torch.equal(c4, fwd) and torch.equal(v1, v2) and not f3.any() and not f4.any()
    for i, (_, x0, y0, x1, y1) in enumerate(RECTS):                     # "image i in the top left corner of slot i, zeros around it"
        assert not v1[i, y1 - y0:].any() and not v1[i, :, x1 - x0:].any()


@pytest.mark.parametrize("sub", [0, 2])
def test_round_trips_with_a_descriptor_the_plan_did_not_write(engine, sub):
    """Image 4 (52 x 37, the largest): "such an image's tile / canvas slot is zero and no pixel is stored or read through its
    geometry" -- its tile and its canvas slot are WRITTEN zeros and its flag is 1.  Its coefficient blocks are not a gap: `coeffs`
    "receives what avcer_jpeg_forward stores", which does not judge a descriptor, so they are written and equal
    avcer_jpeg_forward's for the same records.  (The header used to say of such an image that "nothing is stored or read through
    its geometry"; with `coeffs` given the run showed 105 blocks of it written, from block 66 on -- the forward half's, in bounds.
    The sentence was corrected, not the kernel.)"""
    dev = engine.device
    bad = 4
    desc, blocks = _plan(engine, sub, edit=bad)
    n = len(RECTS)
    src, rects, d_dev = torch.from_numpy(_source().copy()).to(dev), torch.from_numpy(RECTS.copy()).to(dev), _dev(engine, desc)
    head = (_ptr(src), 2, 64, 80, _ptr(rects), _ptr(d_dev), n, 0)
    coeffs = Band("coeffs", (blocks, 64), torch.int16)
    fwd, = check(lambda outs: _call(engine, "avcer_jpeg_forward", *head, _ptr(outs[0]), blocks), [coeffs], [src, rects, d_dev], device=dev)
    flags = Band("flags", (n,), torch.int32, row_bytes=4)
    want = [int(i == bad) for i in range(n)]

    f, t, c = check(lambda outs: _call(engine, "avcer_jpeg_roundtrip_tiles", *head, _ptr(outs[2]), blocks, _ptr(outs[0]), _ptr(outs[1])),
                    [flags, Band("tiles", (n, 224, 224, 3), torch.uint8, row_bytes=672), coeffs], [src, rects, d_dev], device=dev)
    assert f.tolist() == want and not t[bad].any() and all(t[i].any() for i in range(1, 8) if i != bad) and torch.equal(c, fwd)
    f, v, c = check(lambda outs: _call(engine, "avcer_jpeg_roundtrip_rgb", *head, _ptr(outs[2]), blocks, _ptr(outs[0]), _ptr(outs[1]), HMAX,
                                       WMAX), [flags, Band("canvas", (n, HMAX, WMAX, 3), torch.uint8, row_bytes=3 * WMAX), coeffs],
                    [src, rects, d_dev], device=dev)
    assert f.tolist() == want and not v[bad].any() and all(v[i].any() for i in range(1, 8) if i != bad) and torch.equal(c, fwd)


# ----------------------------------------------------------------------------- avcer_jpeg_tiles, avcer_jpeg_rgb
def test_jpeg_tiles_and_rgb(engine):
    """The supported golden files, then a file the host pass does not handle (CMYK) and the corrupt-table file of
    tests/test_gpu_jpeg.py (two quantisation steps turned into 214 and 202: the range flag): their tiles and canvas slots are zeros,
    and written.  The canvas is 3 rows and 5 columns larger than the largest image, both sides odd."""
    g = np.load(unpack_cases.GOLDEN)
    names = [str(x) for x in g["names"]]
    keep = [i for i in range(len(names)) if bool(g["handled"][i])]
    blobs = [g[f"jpg_{i}"].tobytes() for i in keep]
    wild = bytearray(blobs[[names[i] for i in keep].index("7x9_rgb_s0_q95")])
    wild[94], wild[381] = 0xD6, 0xCA
    blobs += [g[f"jpg_{names.index('40x30_cmyk')}"].tobytes(), bytes(wild)]
    n = len(blobs)
    coeffs = np.zeros(64 * (sum(len(b) for b in blobs) + 1024), dtype=np.int16)
    desc = np.zeros(n, dtype=jpeg.DESC)
    jpeg.entropy_batch(engine.lib, blobs, coeffs, desc, 1)
    assert (desc["status"][:n - 2] == jpeg.OK).all() and desc["status"][n - 2] == jpeg.NOT_HANDLED and desc["status"][n - 1] == jpeg.OK
    ok = desc["status"] == jpeg.OK
    used = int((desc["coef_block"] + desc["n_blocks"])[ok].max())
    hmax, wmax = int(desc["height"][ok].max()) + 3, int(desc["width"][ok].max()) + 5
    hmax, wmax = hmax + (hmax % 2 == 0), wmax + (wmax % 2 == 0)
    assert hmax % 16 and wmax % 16
    c_dev, d_dev = _dev(engine, coeffs[:64 * used]), _dev(engine, desc)
    flags = Band("flags", (n,), torch.int32, row_bytes=4)
    want = [0] * (n - 1) + [1]

    f, t = check(lambda outs: _call(engine, "avcer_jpeg_tiles", _ptr(c_dev), used, _ptr(d_dev), n, _ptr(outs[0]), _ptr(outs[1])),
                 [flags, Band("tiles", (n, 224, 224, 3), torch.uint8, row_bytes=672)], [c_dev, d_dev], device=engine.device)
    assert f.tolist() == want and not t[n - 2:].any() and t[:n - 2].any()
    f, v = check(lambda outs: _call(engine, "avcer_jpeg_rgb", _ptr(c_dev), used, _ptr(d_dev), n, _ptr(outs[0]), _ptr(outs[1]), hmax, wmax),
                 [flags, Band("canvas", (n, hmax, wmax, 3), torch.uint8, row_bytes=3 * wmax)], [c_dev, d_dev], device=engine.device)
    assert f.tolist() == want and not v[n - 2:].any()
    for i in range(n - 2):
        h, w = int(desc["height"][i]), int(desc["width"][i])
        assert not v[i, h:].any() and not v[i, :, w:].any(), names[keep[i]]
