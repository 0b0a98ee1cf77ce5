"""Inputs of the device entropy DECODER's tests (tests/test_jpeg_unpack_host.py on avcer_jpeg_unpack_host, tests/test_gpu_jpeg_unpack.py
on avcer_jpeg_unpack): sets of JPEG files, and the two ways to their coefficients -- the host pass avcer_jpeg_entropy_batch, which is
the oracle with tolerance zero, and scan_batch + one of the unpackers.  No test in here."""
import io
import os

import numpy as np

import jpeg_pack_cases as pack_cases
from avcer_amd import jpeg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_crops.npz")
SUB_BITS = (128, 0)  # what the tests run: the shortest subsequence there is, and the library's default
R_RESTART, R_NO_EOI = 14, 15
MUTANT_SEED = 20261019


def golden():
    """[(name, bytes)] of tests/golden/jpeg_crops.npz, the four fallbacks included."""
    g = np.load(GOLDEN)
    return [(str(n), g[f"jpg_{i}"].tobytes()) for i, n in enumerate(g["names"])]


def crafted(lib):
    """The files the host writer makes of jpeg_pack_cases.crafted(): ([(name, bytes)], coefficients, DESC records of those files) --
    the coefficients a decoder must find are known by construction."""
    names, coeffs, desc, want = pack_cases.crafted(lib)
    blobs, _, status, _ = pack_cases.host_write(lib, coeffs, desc)
    keep = [i for i in range(len(names)) if want[i] == 0]
    assert all(len(blobs[i]) for i in keep) and not status[keep].any()
    c, d = pack_cases.subset(coeffs, desc, keep)
    return [(names[i], blobs[i]) for i in keep], c, d


def _pil(a, **kw):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


def stress():
    """Synchronisation stress: images whose every block is the same four or six bits (a misaligned start never meets a code it
    cannot read and need not resynchronise by itself), and noise at quality 100 (long codes, dozens of FF 00)."""
    out = []
    for side in (64, 256):
        for sub in (2, 0):
            out.append((f"zero {side} s{sub}", _pil(np.zeros((side, side, 3), dtype=np.uint8), quality=95, subsampling=sub)))
            out.append((f"constant {side} s{sub}", _pil(np.full((side, side, 3), (200, 90, 40), dtype=np.uint8), quality=95, subsampling=sub)))
    out.append(("noise 40 q100", _pil(np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8), quality=100, subsampling=0)))
    return out


def scan_start(blob: bytes) -> int:
    """Offset of the first entropy-coded byte of a baseline file: behind its (only) SOS segment."""
    p = 2
    while True:
        assert blob[p] == 0xFF, p
        m, n = blob[p + 1], (blob[p + 2] << 8) | blob[p + 3]
        p += 2 + n
        if m == 0xDA:
            return p


def _rst(blob):
    at = scan_start(blob)
    return [p for p in range(at, len(blob) - 1) if blob[p] == 0xFF and 0xD0 <= blob[p + 1] <= 0xD7]


def defects(files):
    """Single-defect files made from one good 52 x 37 4:2:0 file and its restart-marker twin: [(name, bytes, the reason: 0 where the
    file must stay OK, -1 where it must not and the reason is the host pass's to name)]."""
    by = dict(files)
    good, rst = by["52x37_rgb_s2_q75"], by["52x37_rgb_s0_q95_rst3"]
    marks = _rst(rst)
    assert len(marks) >= 8 and good[-2:] == b"\xff\xd9" and rst[-2:] == b"\xff\xd9"
    out = []
    for name, b in (("good", good), ("rst3", rst)):
        for cut in (1, 2, 40):
            out.append((f"{name}: tail cut by {cut}", b[:-cut], -1))
        out.append((f"{name}: EOI replaced by FF D0", b[:-1] + b"\xd0", R_NO_EOI))
        out.append((f"{name}: FF FF D9", b[:-2] + b"\xff\xff\xd9", 0))
        out.append((f"{name}: garbage behind EOI", b + b"garbage\x00\xff\x00\xff\xd9\xff", 0))
    m = marks[3]
    out.append(("rst3: a marker renumbered", rst[:m + 1] + bytes([0xD0 + ((rst[m + 1] + 1) & 7)]) + rst[m + 2:], R_RESTART))
    out.append(("rst3: a marker removed", rst[:m] + rst[m + 2:], -1))
    mid = (marks[4] + 2 + marks[5]) // 2
    mid += rst[mid - 1] == 0xFF  # not between a 0xFF and its stuffed zero
    assert marks[4] + 2 < mid < marks[5]
    out.append(("rst3: a stray FF D3 inside an interval", rst[:mid] + b"\xff\xd3" + rst[mid:], -1))
    # a segment without a data byte still is a subsequence to decode (jsync::seg_subs: at least one)
    out.append(("rst3: an empty interval", rst[:m + 2] + bytes([0xFF, 0xD0 + ((rst[m + 1] + 1) & 7)]) + rst[m + 2:], -1))
    # exactly 8 bits behind a segment's last block (jsync::write_step: fewer than 8 may be left): a zero byte in front of a marker
    # whose segment ends without padding -- padding bits are ones, so an even last byte has none
    even = [p for p in marks + [len(rst) - 2] if rst[p - 1] % 2 == 0 and not (rst[p - 1] == 0 and rst[p - 2] == 0xFF)]
    assert even
    out.append(("rst3: a byte too many in front of a marker", rst[:even[0]] + b"\x00" + rst[even[0]:], -1))
    return out


def mutants(files, count=200, seed=MUTANT_SEED):
    """`count` files with one byte of the scan overwritten at random: malformed data as a reader may meet it."""
    by = dict(files)
    bases = [by[n] for n in ("52x37_rgb_s2_q75", "52x37_rgb_s2_q95_rst3", "52x37_rgb_s0_q95_optimize", "17x33_rgb_s1_q20_noise",
                             "52x37_l_q95_rst3", "52x37_rgb_s1_q95_rstrow")]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        b = bytearray(bases[k % len(bases)])
        p = int(rng.integers(scan_start(b), len(b)))
        b[p] = int(rng.integers(0, 256))
        out.append((f"mutant {k} (byte {p})", bytes(b)))
    return out


# ------------------------------------------------------------------------------------------------ the two ways
def oracle(lib, blobs, threads=1):
    """avcer_jpeg_entropy_batch with room for everything: (coefficients [blocks, 64], DESC records)."""
    room = max(sum(int(jpeg.probe(lib, b)["n_blocks"]) for b in blobs), 1)
    coeffs = np.zeros((room, 64), dtype=np.int16)
    desc = np.zeros(len(blobs), dtype=jpeg.DESC)
    jpeg.entropy_batch(lib, blobs, coeffs, desc, threads)
    return coeffs, desc


def scanned(lib, blobs, threads=1, cap_bytes=None, cap_tabs=64):
    """scan_batch with room for everything (or for cap_bytes): a dict of its arrays and counts.  `data` is followed by a guard."""
    n = len(blobs)
    room = sum(len(b) for b in blobs) + 16 * n + 16
    data = np.full(room + 64, 0xA5, dtype=np.uint8)
    desc, scan, tabs = np.zeros(n, dtype=jpeg.DESC), np.zeros(n, dtype=jpeg.SCAN), np.zeros(cap_tabs, dtype=jpeg.TAB)
    cap = room if cap_bytes is None else cap_bytes
    n_tabs, need_bytes, need_blocks = jpeg.scan_batch(lib, blobs, data, desc, scan, tabs, threads, cap_bytes=cap)
    return {"data": data, "cap": cap, "desc": desc, "scan": scan, "tabs": tabs, "n_tabs": n_tabs, "need_bytes": need_bytes,
            "need_blocks": need_blocks}


def unpacked_host(lib, blobs, sub_bits):
    """scan_batch + avcer_jpeg_unpack_host: (coefficients, DESC records, status)."""
    s = scanned(lib, blobs)
    desc = s["desc"].copy()
    if not (desc["status"] == jpeg.OK).any():
        return np.zeros((1, 64), dtype=np.int16), desc, desc["status"].astype(np.int32)
    coeffs, status = jpeg.unpack_host(lib, s["data"][:max(s["need_bytes"], 16)], s["scan"], s["tabs"][:max(s["n_tabs"], 1)], desc,
                                      max(s["need_blocks"], 1), sub_bits)
    return coeffs, desc, status


def assert_same(got, want, names, reasons=True):
    """(coefficients, DESC records) of a decoder against the oracle's: status of every file, reason (where asked), the blocks of
    every file both call OK."""
    gc, gd = got
    wc, wd = want
    for i, name in enumerate(names):
        assert gd["status"][i] == wd["status"][i], (name, int(gd["reason"][i]), int(wd["reason"][i]))
        if reasons:
            assert gd["reason"][i] == wd["reason"][i], name
        if wd["status"][i] == jpeg.OK:
            assert gd["n_blocks"][i] == wd["n_blocks"][i] and gd["coef_block"][i] == wd["coef_block"][i], name
            a, n = int(wd["coef_block"][i]), int(wd["n_blocks"][i])
            np.testing.assert_array_equal(gc[a:a + n], wc[a:a + n], err_msg=name)
