"""The device entropy decoder's algorithm on the host: avcer_jpeg_scan_batch + avcer_jpeg_unpack_host (the phases of the kernel as
loops over its threads, csrc/jpeg_unpack.hip) against the host pass avcer_jpeg_entropy_batch on the same files, tolerance zero: the same
status for every file, the same reason on the single-defect files, the same coefficients for every file both call OK -- as one
batch, file by file and permuted, at the shortest subsequence length and at the default.  Also: what scan_batch does with a short
buffer, and that it de-duplicates Huffman tables by content."""
import ctypes

import numpy as np
import pytest

import jpeg_unpack_cases as cases
from avcer_amd import jpeg


@pytest.fixture(scope="module")
def lib():
    from avcer_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(build.LIB)
    for name in ("avcer_jpeg_probe", "avcer_jpeg_entropy_batch", "avcer_jpeg_plan", "avcer_jpeg_write_batch", "avcer_jpeg_scan_batch",
                 "avcer_jpeg_unpack_host"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def sets(lib):
    """{set: [(name, bytes)]} and the oracle's (coefficients, DESC records) of each, computed once."""
    files = cases.golden()
    crafted, c, d = cases.crafted(lib)
    out = {"golden": files, "crafted": crafted, "stress": cases.stress(), "defects": [(n, b) for n, b, _ in cases.defects(files)],
           "mutants": cases.mutants(files)}
    return out, {k: cases.oracle(lib, [b for _, b in v]) for k, v in out.items()}, (c, d)


def test_the_library_exports_the_device_decoder():
    from avcer_amd import _lib, build

    build.build()
    for name in ("avcer_jpeg_scan_batch", "avcer_jpeg_unpack", "avcer_jpeg_unpack_host"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(build.LIB), name)


def test_an_unknown_entropy_is_refused_before_any_work():
    for bad in ("bogus", "", "Device", None):
        for fn in (jpeg.decode_tiles, jpeg.decode_canvas):
            with pytest.raises(ValueError, match="entropy"):
                fn(None, [b"x"], entropy=bad)


def test_the_oracle_reads_the_crafted_files_as_they_were_written(lib, sets):
    files, want, (c, d) = sets
    wc, wd = want["crafted"]
    assert (wd["status"] == jpeg.OK).all()
    for i, (name, _) in enumerate(files["crafted"]):
        a, n = int(d["coef_block"][i]), int(d["n_blocks"][i])
        np.testing.assert_array_equal(wc[int(wd["coef_block"][i]):int(wd["coef_block"][i]) + n], c[a:a + n], err_msg=name)


def test_the_sets_hold_what_the_comparison_needs(lib, sets):
    files, want, _ = sets
    status = want["mutants"][1]["status"]
    assert (status == jpeg.OK).sum() >= 20 and (status != jpeg.OK).sum() >= 20  # the host pass alone
    for (name, _, reason), st, r in zip(cases.defects(files["golden"]), want["defects"][1]["status"], want["defects"][1]["reason"]):
        assert (st == jpeg.OK) == (reason == 0), (name, int(r))
        if reason > 0:
            assert r == reason, name
    assert (want["stress"][1]["status"] == jpeg.OK).all()
    assert sum(b.count(b"\xff\x00") for _, b in files["stress"]) >= 30
    assert (want["golden"][1]["status"] != jpeg.OK).sum() == 4


@pytest.mark.parametrize("sub_bits", cases.SUB_BITS)
@pytest.mark.parametrize("which", ("golden", "crafted", "stress", "defects", "mutants"))
def test_one_batch_equals_the_host_pass(lib, sets, which, sub_bits):
    files, want, (c, d) = sets
    names, blobs = [n for n, _ in files[which]], [b for _, b in files[which]]
    gc, gd, status = cases.unpacked_host(lib, blobs, sub_bits)
    np.testing.assert_array_equal(status, gd["status"])
    cases.assert_same((gc, gd), want[which], names, reasons=which != "mutants")
    if which == "crafted":  # and they are the coefficients the files were written from
        for i, name in enumerate(names):
            a, n = int(d["coef_block"][i]), int(d["n_blocks"][i])
            np.testing.assert_array_equal(gc[int(gd["coef_block"][i]):int(gd["coef_block"][i]) + n], c[a:a + n], err_msg=name)


@pytest.mark.parametrize("sub_bits", cases.SUB_BITS)
def test_a_file_is_what_it_is_alone_and_in_any_order(lib, sets, sub_bits):
    files, want, _ = sets
    pool = files["golden"] + files["crafted"] + files["stress"] + files["defects"] + files["mutants"][:40]
    whole = cases.unpacked_host(lib, [b for _, b in pool], sub_bits)

    def blocks(res, i):
        a, n = int(res[1]["coef_block"][i]), int(res[1]["n_blocks"][i])
        return res[0][a:a + n]

    for i, (name, blob) in enumerate(pool):
        one = cases.unpacked_host(lib, [blob], sub_bits)
        assert one[1]["status"][0] == whole[1]["status"][i] and one[1]["reason"][0] == whole[1]["reason"][i], name
        if one[1]["status"][0] == jpeg.OK:
            np.testing.assert_array_equal(blocks(one, 0), blocks(whole, i), err_msg=name)
    order = np.random.default_rng(5).permutation(len(pool))
    mixed = cases.unpacked_host(lib, [pool[i][1] for i in order], sub_bits)
    for k, i in enumerate(order):
        assert mixed[1]["status"][k] == whole[1]["status"][i] and mixed[1]["reason"][k] == whole[1]["reason"][i], pool[i][0]
        if mixed[1]["status"][k] == jpeg.OK:
            np.testing.assert_array_equal(blocks(mixed, k), blocks(whole, i), err_msg=pool[i][0])


def test_scan_batch_assigns_what_the_host_pass_assigns_whatever_the_thread_count(lib, sets):
    files, want, _ = sets
    blobs = [b for _, b in files["golden"] + files["defects"]]
    wd = cases.oracle(lib, blobs)[1]
    for threads in (1, 3, 16):
        s = cases.scanned(lib, blobs, threads)
        header_ok = s["desc"]["status"] == jpeg.OK
        # the scan walk is the device's: a file the host pass refuses while walking it is still OK here
        assert (header_ok | (wd["status"] != jpeg.OK)).all()
        np.testing.assert_array_equal(s["desc"]["coef_block"], wd["coef_block"])
        np.testing.assert_array_equal(s["desc"]["n_blocks"][header_ok], wd["n_blocks"][header_ok])
        np.testing.assert_array_equal(s["desc"]["reason"][~header_ok], wd["reason"][~header_ok])
        assert s["need_blocks"] == int(wd["n_blocks"].sum()) and (s["scan"]["offset"] % 16 == 0).all()
        for i in np.nonzero(header_ok)[0]:
            at, n = int(s["scan"]["offset"][i]), int(s["scan"]["nbytes"][i])
            assert s["data"][at:at + n].tobytes() == blobs[i][cases.scan_start(blobs[i]):]
        assert (s["data"][s["need_bytes"]:] == 0xA5).all()


def test_a_short_buffer_is_reported_and_respected(lib, sets):
    files, _, _ = sets
    blobs = [b for n, b in files["golden"] if n.startswith("52x37_rgb")]
    full = cases.scanned(lib, blobs)
    need = full["need_bytes"]
    assert (full["desc"]["status"] == jpeg.OK).all() and need == int(((full["scan"]["nbytes"] + 15) // 16 * 16).sum())
    for cap in (need - 1, need // 2, 15, 0):
        s = cases.scanned(lib, blobs, cap_bytes=cap)
        refused = s["desc"]["reason"] == jpeg.R_NO_SPACE
        assert refused.any() and (s["desc"]["status"][refused] == jpeg.NOT_HANDLED).all() and (s["desc"]["n_blocks"][refused] == 0).all()
        assert s["need_bytes"] == need and s["need_blocks"] == full["need_blocks"]
        assert (s["data"][cap:] == 0xA5).all()  # nothing behind the capacity given
        kept = ~refused
        assert ((s["scan"]["offset"] + s["scan"]["nbytes"])[kept] <= cap).all()
        if kept.any():  # what fits is decoded as ever
            desc = s["desc"].copy()
            coeffs, status = jpeg.unpack_host(lib, s["data"][:max(cap, 16)], s["scan"], s["tabs"][:s["n_tabs"]], desc, full["need_blocks"], 128)
            want = cases.oracle(lib, [b for b, k in zip(blobs, kept) if k])
            got_blocks = np.concatenate([coeffs[int(d["coef_block"]):int(d["coef_block"] + d["n_blocks"])] for d in desc[kept]])
            np.testing.assert_array_equal(got_blocks, want[0][:len(got_blocks)])
    s = cases.scanned(lib, blobs, cap_tabs=3)  # tables are capacity too
    assert (s["desc"]["reason"] == jpeg.R_NO_SPACE).any() and s["n_tabs"] == full["n_tabs"] > 3


def test_tables_are_kept_once(lib, sets):
    files, _, _ = sets
    std = [b for n, b in files["golden"] if n.endswith("_q95") and "_rgb_" in n]
    opt = [b for n, b in files["golden"] if n == "52x37_rgb_s2_q95_optimize"]
    assert len(std) >= 10 and len(opt) == 1
    a = cases.scanned(lib, std)
    assert a["n_tabs"] == 4 and (a["desc"]["status"] == jpeg.OK).all()
    b = cases.scanned(lib, std + opt)
    own = {(int(b["scan"]["dc"][-1][c]), int(b["scan"]["ac"][-1][c])) for c in range(3)}
    new = {t for pair in own for t in pair} - set(range(4))
    assert b["n_tabs"] == 4 + len(new) and 1 <= len(new) <= 4
    np.testing.assert_array_equal(b["tabs"][:4], a["tabs"][:4])
    np.testing.assert_array_equal(b["scan"][:len(std)], a["scan"])
    assert cases.scanned(lib, opt + std)["n_tabs"] == b["n_tabs"]
