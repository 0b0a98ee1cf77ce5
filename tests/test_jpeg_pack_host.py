"""The inputs of the device entropy coder's tests (tests/jpeg_pack_cases.py) on the HOST writer, avcer_jpeg_write_batch, which is
the oracle of tests/test_gpu_jpeg_pack.py: the sets hold what makes that comparison worth something -- a stuffed FF 00 in front of
EOI, ZRL symbols, stuffed bytes by the dozen, scans of every bit length mod 8 -- and the facts about PIL's files they rest on are
true here.  Also: the library exports avcer_jpeg_pack, and encode_images refuses an unknown `entropy` before any work."""
import ctypes

import numpy as np
import pytest

import jpeg_pack_cases as cases
from avcer_amd import jpeg


@pytest.fixture(scope="module")
def lib():
    from avcer_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(build.LIB)
    for name in ("avcer_jpeg_plan", "avcer_jpeg_write_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def written(lib):
    """Every file of both sets as the host writer writes it: [(name, bytes, coefficients, DESC record)]."""
    names, coeffs, desc, want = cases.crafted(lib)
    blobs, offsets, status, need = cases.host_write(lib, coeffs, desc)
    np.testing.assert_array_equal(status, want)
    assert need == offsets[-1] == sum(len(b) for b in blobs)
    out = [(n, b, coeffs, d) for n, b, d in zip(names, blobs, desc)]
    for (q, s), imgs in cases.image_groups().items():
        c, d = jpeg.forward_numpy(imgs, q, s)
        blobs, _, status, _ = cases.host_write(lib, c, d)
        assert not status.any()
        for k, (im, b) in enumerate(zip(imgs, blobs)):
            assert b == cases.pil_bytes(im, q, s), (q, s, k)
            out.append((f"image {k} q{q} s{s}", b, c, d[k]))
    return out


def test_the_library_exports_the_device_coder():
    from avcer_amd import _lib, build

    build.build()
    assert "avcer_jpeg_pack" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(build.LIB), "avcer_jpeg_pack")


def test_an_unknown_entropy_is_refused_before_any_work():
    for bad in ("bogus", "", "Device", None):
        with pytest.raises(ValueError, match="entropy"):
            jpeg.encode_images(None, None, None, entropy=bad)


def test_crafted_files_are_refused_for_the_reason_stated_and_their_neighbours_are_intact(lib):
    names, coeffs, desc, want = cases.crafted(lib)
    blobs, _, status, _ = cases.host_write(lib, coeffs, desc)
    assert sorted(set(want.tolist())) == [0, cases.R_RANGE, cases.R_ENC_DESC]
    for i, n in enumerate(names):
        assert (len(blobs[i]) == 0) == (want[i] != 0), n
        if want[i] == 0:  # alone, a file is what it is among the others
            c, d = cases.subset(coeffs, desc, [i])
            assert cases.host_write(lib, c, d)[0] == [blobs[i]], n
    assert 200 <= len(coeffs) <= 400


def test_the_sets_hold_what_the_device_comparison_needs(written):
    live = [(n, b, c, d) for n, b, c, d in written if b]
    stats = {n: cases.scan_stats(b, c, d) for n, b, c, d in live}
    for n, b, c, d in live:  # the bit count of this file's statement is the writer's: the scan is that many bits, filled up, stuffed
        assert len(b) == 623 + (stats[n][0] + 7) // 8 + cases.stuffed_bytes(b) + 2, n
    assert any(b[-4:] == b"\xff\x00\xff\xd9" for _, b, _, _ in live)
    assert sum(z for _, z in stats.values()) >= 1 and stats["last coefficient only"][1] == 9 and stats["runs of 15 and 16"][1] == 4
    assert sum(cases.stuffed_bytes(b) for _, b, _, _ in live) >= 30
    assert {bits % 8 for bits, _ in stats.values()} == set(range(8))
    crafted_bits = {stats[n][0] % 8 for n in stats if n.startswith("luma DC category")}
    assert crafted_bits == set(range(8))
    # the longest block: 20 + 63 * 26 bits, three of them in a file
    assert stats["every AC 1023 behind the largest DC difference"][0] >= 2 * (20 + 63 * 26)
    assert stats["all zero 64 x 64"][0] == 512


def test_the_facts_about_pils_files():
    ends = [cases.pil_bytes(np.random.default_rng(s).integers(0, 256, (8, 8, 3)).astype(np.uint8), 95, 0)[-4:] == b"\xff\x00\xff\xd9"
            for s in range(100)]
    assert ends[8] and 5 <= sum(ends) <= 20  # about one seed in ten
    noise = np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8)
    assert cases.stuffed_bytes(cases.pil_bytes(noise, 100, 0)) == 37
    assert len(cases.pil_bytes(np.full((64, 64, 3), 128, dtype=np.uint8), 95, 2)) == 623 + 64 + 2
