"""The host half of the JPEG crop decoder (csrc/jpeg_decode.hip avcer_jpeg_probe / avcer_jpeg_entropy_batch, ctx NULL: no device) and the
numpy statement of its device half (avcer_amd/jpeg.py pixels_numpy) against PIL's decode (libjpeg-turbo), bit for bit."""
import ctypes
import io
import os

import numpy as np
import pytest

from avcer_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALLBACKS = {"100x75_rgb_progressive", "40x30_png_named_jpg", "100x75_rgb_cut40", "40x30_cmyk"}


@pytest.fixture(scope="module")
def lib():
    from avcer_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(build.LIB)
    for name in ("avcer_jpeg_probe", "avcer_jpeg_entropy_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("jpeg_crops")
    names = [str(n) for n in g["names"]]
    return [(n, g[f"jpg_{i}"].tobytes(), bool(g["handled"][i]), np.cumsum(g[f"rgbdx_{i}"], axis=1, dtype=np.uint8) if f"rgbdx_{i}" in g.files else None)  # undo_dx of make_jpeg_golden
            for i, n in enumerate(names)]


def _pil_rgb(blob):
    from PIL import Image

    with Image.open(io.BytesIO(blob)) as img:
        return np.asarray(img.convert("RGB"))


def _decode(lib, blobs, threads=0, cap_blocks=None, room=None):
    room = room if room is not None else sum(len(b) for b in blobs) + 4096
    coeffs = np.zeros(64 * room, dtype=np.int16)
    desc = np.zeros(len(blobs), dtype=jpeg.DESC)
    need = jpeg.entropy_batch(lib, blobs, coeffs, desc, threads, cap_blocks=cap_blocks)
    return coeffs, desc, need


def _random_files(count=200, seed=5):
    """Freshly PIL-encoded images of random size <= 64 x 64 over the fixtures' parameter grid."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    out = []
    for t in range(count):
        w, h = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        mode = "L" if t % 5 == 0 else "RGB"
        shape = (h, w, 3) if mode == "RGB" else (h, w)
        if t % 3 == 0:
            a = rng.integers(0, 256, shape)
        elif t % 3 == 1:
            yy, xx = np.mgrid[0:h, 0:w]
            a = (np.sin(xx / 7.0) + np.cos(yy / 5.0)) * 60 + 128
            a = (a[..., None] if mode == "RGB" else a) + rng.normal(0, 8, shape)
        else:
            a = rng.integers(0, 2, shape) * 255
        kw = dict(quality=int(rng.choice([95, 75, 20])), subsampling=int(rng.integers(0, 3)))
        if t % 4 == 0:
            kw["optimize"] = True
        if t % 7 == 0:
            kw["restart_marker_blocks"] = 3
        if t % 11 == 0:
            kw["restart_marker_rows"] = 1
        b = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), mode).save(b, "JPEG", **kw)
        out.append(b.getvalue())
    return out


def test_fixture_is_what_pil_decodes_here(cases):
    """The committed goldens are PIL's decode on the machine that wrote them; this machine's PIL agrees (where it does not, the
    oracle itself moved and the generator has to be looked at, not the decoder)."""
    for name, blob, handled, rgb in cases:
        if handled:
            np.testing.assert_array_equal(_pil_rgb(blob), rgb, err_msg=name)


def test_entropy_pass_and_numpy_pixels_equal_pil_on_every_fixture(lib, cases):
    blobs = [c[1] for c in cases if c[2]]
    coeffs, desc, _ = _decode(lib, blobs)
    got = jpeg.pixels_numpy(coeffs, desc)
    for (name, _, _, rgb), img in zip([c for c in cases if c[2]], got):
        assert img is not None, name
        np.testing.assert_array_equal(img, rgb, err_msg=name)


def test_entropy_pass_and_numpy_pixels_equal_pil_on_random_files(lib):
    blobs = _random_files()
    coeffs, desc, _ = _decode(lib, blobs)
    assert (desc["status"] == jpeg.OK).all(), desc["reason"]
    for i, (blob, img) in enumerate(zip(blobs, jpeg.pixels_numpy(coeffs, desc))):
        np.testing.assert_array_equal(img, _pil_rgb(blob), err_msg=f"random file {i}")


def test_probe_fields_equal_what_pil_reports(lib, cases):
    from PIL import Image

    for name, blob, handled, _ in cases:
        info = jpeg.probe(lib, blob)
        if not handled:
            continue
        assert info["status"] == jpeg.OK, name
        with Image.open(io.BytesIO(blob)) as img:
            assert (info["width"], info["height"]) == img.size, name
            assert info["ncomp"] == len(img.layer) == (1 if img.mode == "L" else 3), name
            assert (info["hs"], info["vs"]) == tuple(img.layer[0][1:3]), name
            for c, (_, hs, vs, tq) in enumerate(img.layer):
                assert info["tq"][c] == tq, name
                np.testing.assert_array_equal(info["qt"][c], np.asarray(img.quantization[tq], dtype=np.uint16), err_msg=name)
            inter = len(img.layer) == 3
            mx = -(-img.size[0] // (8 * (info["hs"] if inter else 1)))
            my = -(-img.size[1] // (8 * (info["vs"] if inter else 1)))
            want = [(mx * hs, my * vs) for _, hs, vs, _ in img.layer] if inter else [(mx, my)]
            assert [(info["bw"][c], info["bh"][c]) for c in range(len(want))] == want, name
            assert info["n_blocks"] == sum(a * b for a, b in want), name


def test_status_is_ok_for_every_baseline_file_and_not_handled_for_exactly_the_four(lib, cases):
    """The cap on the fallback: it may not hide a decoder failure."""
    _, desc, _ = _decode(lib, [c[1] for c in cases])
    refused = {c[0] for c, d in zip(cases, desc) if d["status"] != jpeg.OK}
    assert refused == FALLBACKS == {c[0] for c in cases if not c[2]}
    assert set(desc["status"].tolist()) == {jpeg.OK, jpeg.NOT_HANDLED}
    # the probe sees the header alone: the cut file's header is whole, the other three are refused there already
    by = {c[0]: jpeg.probe(lib, c[1])["status"] for c in cases if not c[2]}
    assert by == {"100x75_rgb_progressive": jpeg.NOT_HANDLED, "40x30_png_named_jpg": jpeg.NOT_HANDLED,
                  "100x75_rgb_cut40": jpeg.OK, "40x30_cmyk": jpeg.NOT_HANDLED}


def test_malformed_streams_are_reported_not_decoded(lib, cases):
    """Cuts of a small file at every length, a missing EOI, a second SOI in its place: reported, never decoded (and never for lack of
    room: every cut has room for the whole picture).  Bytes behind the EOI are ignored, as PIL ignores them."""
    blob = next(c[1] for c in cases if c[0] == "17x33_rgb_s2_q75_rst3")
    cuts = [blob[:k] for k in range(0, len(blob))]
    blocks = int(jpeg.probe(lib, blob)["n_blocks"])
    _, desc, _ = _decode(lib, cuts, room=blocks * len(cuts))
    assert (desc["status"] == jpeg.NOT_HANDLED).all() and not (desc["reason"] == jpeg.R_NO_SPACE).any()
    coeffs, desc, _ = _decode(lib, [blob[:-2], blob[:-2] + b"\xff\xd8", blob + b"trailing bytes"], room=3 * blocks)
    assert desc["status"].tolist() == [jpeg.NOT_HANDLED, jpeg.NOT_HANDLED, jpeg.OK]
    np.testing.assert_array_equal(jpeg.pixels_numpy(coeffs, desc)[2], _pil_rgb(blob))


def test_a_batch_equals_single_files_at_1_and_16_threads(lib, cases):
    blobs = [c[1] for c in cases]
    c1, d1, n1 = _decode(lib, blobs, threads=1)
    c16, d16, n16 = _decode(lib, blobs, threads=16)
    assert n1 == n16 and d1.tobytes() == d16.tobytes()
    np.testing.assert_array_equal(c1, c16)
    assert (np.diff(d1["coef_block"]) >= 0).all()
    for i, blob in enumerate(blobs):
        cs, ds, _ = _decode(lib, [blob], threads=1, room=max(int(d1["n_blocks"][i]), 1))
        assert ds["status"][0] == d1["status"][i] and ds["reason"][0] == d1["reason"][i]
        if ds["status"][0] == jpeg.OK:
            at, nb = int(d1["coef_block"][i]), int(d1["n_blocks"][i])
            assert ds["n_blocks"][0] == nb and ds["coef_block"][0] == 0
            np.testing.assert_array_equal(cs[:64 * nb], c1[64 * at:64 * (at + nb)], err_msg=cases[i][0])


def test_storage_one_block_short_is_not_handled_and_nothing_is_written_behind_it(lib, cases):
    picks = [c for c in cases if c[0] in ("17x33_rgb_s2_q95", "52x37_l_q95_optimize", "100x75_rgb_s1_q95")]
    assert len(picks) == 3
    blobs = [c[1] for c in picks]
    _, full, need = _decode(lib, blobs)
    assert need == int(full["n_blocks"].sum())
    guard = 0x5A5A
    for cap in (need - 1, int(full["n_blocks"][0]), 0):
        coeffs = np.full(64 * need + 256, guard, dtype=np.int16)
        desc = np.zeros(3, dtype=jpeg.DESC)
        assert jpeg.entropy_batch(lib, blobs, coeffs, desc, 4, cap_blocks=cap) == need
        fits = np.cumsum(full["n_blocks"]) <= cap
        # files are placed in order; one that does not fit is refused and a later, smaller one may still fit behind the others
        used = 0
        for i in range(3):
            ok = full["n_blocks"][i] <= cap - used
            assert (desc["status"][i] == jpeg.OK) == ok, (cap, i)
            if ok:
                used += int(full["n_blocks"][i])
            else:
                assert desc["reason"][i] == jpeg.R_NO_SPACE and desc["n_blocks"][i] == 0
        assert used <= cap and (coeffs[64 * cap:] == guard).all(), cap
        assert fits[0] == (desc["status"][0] == jpeg.OK)


def test_range_guard_of_the_numpy_statement(lib, cases):
    """The inverse DCT is defined -- the same in libjpeg's C and SIMD code -- while dequantised coefficients and pass-1 results stay
    within +-16383 and samples within [-512, 511].  Every fixture is far inside (pass 1 below 8192, samples below 384); a file
    with two quantisation steps corrupted (its stream still parses) is outside, and pixels_numpy returns no picture for it."""
    blobs = [c[1] for c in cases if c[2]]
    coeffs, desc, _ = _decode(lib, blobs)
    worst1 = worst2 = 0
    for d in desc:
        at = int(d["coef_block"])
        for c in range(int(d["ncomp"])):
            nb = int(d["bw"][c]) * int(d["bh"][c])
            x = coeffs.reshape(-1, 64)[at:at + nb].reshape(nb, 8, 8).astype(np.int64) * d["qt"][c].reshape(1, 8, 8).astype(np.int64)
            p1 = jpeg._idct_1d(x.transpose(1, 0, 2), 11)
            p2 = jpeg._idct_1d(p1.transpose(2, 1, 0), 18)
            worst1, worst2 = max(worst1, int(np.abs(p1).max())), max(worst2, int(np.abs(p2).max()))
            at += nb
    assert worst1 < 8192 and worst2 < 384, (worst1, worst2)
    wild = bytearray(next(c[1] for c in cases if c[0] == "7x9_rgb_s0_q95"))
    wild[94], wild[381] = 0xD6, 0xCA
    coeffs, desc, _ = _decode(lib, [bytes(wild)])
    assert desc["status"][0] == jpeg.OK and jpeg.pixels_numpy(coeffs, desc) == [None]


def test_a_header_that_claims_more_blocks_than_the_bytes_can_hold_reserves_nothing(lib, cases):
    """A whole, valid header with the frame size changed to 65535 x 65535: about 1e8 blocks claimed by a file of some hundred bytes.
    A block costs two bits at the least, so the file is cut short whatever follows; it is refused at the header -- by the probe
    too -- and adds nothing to the storage the batch asks for (the caller would otherwise pin gigabytes before the scan fails)."""
    blob = next(c[1] for c in cases if c[0] == "17x33_rgb_s2_q95")
    at = blob.index(b"\xff\xc0")
    huge = blob[:at + 5] + b"\xff\xff\xff\xff" + blob[at + 9:]
    info = jpeg.probe(lib, huge)
    assert (info["width"], info["height"]) == (65535, 65535) and info["status"] == jpeg.NOT_HANDLED
    _, desc, need = _decode(lib, [blob, huge, blob])
    assert desc["status"].tolist() == [jpeg.OK, jpeg.NOT_HANDLED, jpeg.OK] and desc["reason"][1] != jpeg.R_NO_SPACE
    assert need == 2 * int(desc["n_blocks"][0]) and desc["n_blocks"][1] == 0
    # the bound is the stream's own: every fixture, the uniform 1 x 1 ones included, is far inside it
    for name, b, handled, _ in cases:
        if handled:
            i = jpeg.probe(lib, b)
            assert i["status"] == jpeg.OK and int(i["n_blocks"]) <= len(b), name
