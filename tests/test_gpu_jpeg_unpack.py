"""The entropy DECODER on the device (csrc/jpeg_unpack.hip avcer_jpeg_unpack, Engine.jpeg_unpack, jpeg.decode_tiles / decode_canvas with
entropy="device") against its oracle, the host pass avcer_jpeg_entropy_batch, and against its own host statement
avcer_jpeg_unpack_host, on the sets of tests/jpeg_unpack_cases.py (tests/test_jpeg_unpack_host.py shows what these hold and that the
algorithm is right on them): status, reason and coefficients are equal.  Then the callers: tiles, canvas, rects and paths are those
of entropy="host".  No case has a tolerance.  Files are at most 256 x 256, mostly 52 x 37: at 128 bits a subsequence these are
already some hundred subsequences in several units and a dozen segments a file."""
import os

import numpy as np
import pytest
import torch

import jpeg_unpack_cases as cases
from avcer_amd import jpeg, video_pipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets(engine):
    """{set: [(name, bytes)]} and the oracle's (coefficients, DESC records) of each.  Never written to."""
    files = cases.golden()
    crafted, _, _ = cases.crafted(engine.lib)
    out = {"golden": files, "crafted": crafted, "stress": cases.stress(), "defects": [(n, b) for n, b, _ in cases.defects(files)],
           "mutants": cases.mutants(files)}
    return out, {k: cases.oracle(engine.lib, [b for _, b in v]) for k, v in out.items()}


def _unpack(engine, blobs, sub_bits):
    """scan_batch + Engine.jpeg_unpack: (coefficients [blocks, 64], DESC records as the device left them, status)."""
    s = cases.scanned(engine.lib, blobs)
    dev = engine.device
    data = torch.from_numpy(s["data"][:s["need_bytes"]].copy()).to(dev)
    scan = torch.from_numpy(s["scan"].view(np.uint8).reshape(-1).copy()).to(dev)
    tabs = torch.from_numpy(s["tabs"][:s["n_tabs"]].view(np.uint8).reshape(-1).copy()).to(dev)
    desc = torch.from_numpy(s["desc"].view(np.uint8).reshape(-1).copy()).to(dev)
    coeffs, status = engine.jpeg_unpack(data, scan, tabs, s["n_tabs"], desc, len(blobs), s["need_blocks"], sub_bits)
    torch.cuda.synchronize()
    return coeffs.cpu().numpy().reshape(-1, 64), desc.cpu().numpy().view(jpeg.DESC), status.cpu().numpy()


@pytest.mark.parametrize("sub_bits", cases.SUB_BITS)
@pytest.mark.parametrize("which", ("golden", "crafted", "stress", "defects"))
def test_one_batch_equals_the_host_pass_and_the_host_statement(engine, sets, which, sub_bits):
    files, want = sets
    names, blobs = [n for n, _ in files[which]], [b for _, b in files[which]]
    gc, gd, status = _unpack(engine, blobs, sub_bits)
    np.testing.assert_array_equal(status, gd["status"])
    cases.assert_same((gc, gd), want[which], names)
    hc, hd, hstatus = cases.unpacked_host(engine.lib, blobs, sub_bits)
    np.testing.assert_array_equal(status, hstatus)
    cases.assert_same((gc, gd), (hc, hd), names)


def test_two_hundred_mutants_in_one_batch(engine, sets):
    """Malformed data as a reader may meet it, one launch, not repeated: every loop of the kernel is counted (at most 258 rounds a
    unit), and tests/test_jpeg_unpack_host.py runs the same phases on the same files on the host."""
    files, want = sets
    names, blobs = [n for n, _ in files["mutants"]], [b for _, b in files["mutants"]]
    assert (want["mutants"][1]["status"] == jpeg.OK).sum() >= 20 and (want["mutants"][1]["status"] != jpeg.OK).sum() >= 20
    gc, gd, status = _unpack(engine, blobs, 128)
    np.testing.assert_array_equal(status, gd["status"])
    cases.assert_same((gc, gd), want["mutants"], names, reasons=False)
    hc, hd, hstatus = cases.unpacked_host(engine.lib, blobs, 128)
    np.testing.assert_array_equal(status, hstatus)
    np.testing.assert_array_equal(gd["reason"], hd["reason"])


def test_bad_arguments_are_refused(engine):
    s = cases.scanned(engine.lib, [cases.golden()[8][1]])
    dev = engine.device
    args = [torch.from_numpy(s[k].view(np.uint8).reshape(-1).copy()).to(dev) for k in ("data", "scan", "tabs", "desc")]
    for sub in (64, 130, -32):
        with pytest.raises(ValueError, match="sub_bits"):
            engine.jpeg_unpack(args[0], args[1], args[2], s["n_tabs"], args[3], 1, s["need_blocks"], sub)
    with pytest.raises(ValueError, match="scan"):
        engine.jpeg_unpack(args[0], args[1][:8], args[2], s["n_tabs"], args[3], 1, s["need_blocks"])
    with pytest.raises(ValueError, match="device"):
        engine.jpeg_unpack(args[0].cpu(), args[1], args[2], s["n_tabs"], args[3], 1, s["need_blocks"])


def test_decode_tiles_and_canvas_are_those_of_the_host_entropy_pass(engine, sets):
    files, _ = sets
    blobs = [b for n, b in files["golden"] if not n.endswith("cut40")] + [b for n, b in files["defects"] if "FF FF D9" in n or "garbage" in n]
    tiles_h, paths_h = jpeg.decode_tiles(engine, blobs, 2)
    tiles_d, paths_d = jpeg.decode_tiles(engine, blobs, 2, entropy="device")
    assert paths_d == paths_h and paths_h.count("pil") == 3 and "device" in paths_h
    assert torch.equal(tiles_d, tiles_h)
    (canvas_h, rects_h), cp_h = jpeg.decode_canvas(engine, blobs, 2)
    (canvas_d, rects_d), cp_d = jpeg.decode_canvas(engine, blobs, 2, entropy="device")
    assert cp_d == cp_h == paths_h
    np.testing.assert_array_equal(rects_d, rects_h)
    assert torch.equal(canvas_d, canvas_h)
    # a file only the scan walk refuses (its header is fine): both ways hand it to PIL, which reads what it can of a cut file
    cut = [b for n, b in files["golden"] if n.endswith("cut40")] + blobs[:3]
    for entropy in ("host", "device"):
        try:
            got = jpeg.decode_tiles(engine, cut, 1, entropy=entropy)
        except OSError as e:
            got = type(e)
        if entropy == "host":
            want = got
    assert (got is want) if isinstance(want, type) else (got[1] == want[1] and torch.equal(got[0], want[0]))


def test_read_face_dir_device_reads_the_same_folder_either_way(engine, sets, tmp_path):
    files, _ = sets
    keep = [b for n, b in files["golden"] if n.startswith(("52x37", "100x75_rgb_s", "203x187", "40x30_png"))]
    folder = tmp_path / "clip" / "00"
    os.makedirs(folder)
    for i, b in enumerate(keep):
        if i != 2:  # a missing frame
            (folder / f"{i:06d}.jpg").write_bytes(b)
    a, pa = video_pipeline.read_face_dir_device(engine, str(tmp_path / "clip"), len(keep) + 1)
    b, pb = video_pipeline.read_face_dir_device(engine, str(tmp_path / "clip"), len(keep) + 1, entropy="device")
    np.testing.assert_array_equal(pa, pb)
    assert torch.equal(a, b) and not pa[2] and a[3].any()
    with pytest.raises(ValueError, match="entropy"):
        video_pipeline.read_face_dir_device(engine, str(tmp_path / "clip"), 4, entropy="gpu")
    with pytest.raises(ValueError, match="jpeg_entropy"):
        video_pipeline.preprocess_video_and_predict(engine, str(tmp_path / "clip"), str(tmp_path), 25, 4, jpeg_entropy="gpu")
