"""The host half of the JPEG encoder (csrc/jpeg_encode.hip avcer_jpeg_quant_tables / avcer_jpeg_plan / avcer_jpeg_write_batch, ctx NULL: no
device) and the numpy statement of its device half (avcer_amd/jpeg.py forward_numpy) against the files PIL writes (libjpeg-turbo),
byte for byte."""
import ctypes
import io

import numpy as np
import pytest

from avcer_amd import jpeg

QUALITIES = (1, 20, 75, 95, 100)


@pytest.fixture(scope="module")
def lib():
    from avcer_amd import _lib, build

    build.build()
    lib = ctypes.CDLL(build.LIB)
    for name in ("avcer_jpeg_probe", "avcer_jpeg_entropy_batch", "avcer_jpeg_quant_tables", "avcer_jpeg_plan", "avcer_jpeg_write_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def _pil(rgb, quality, subsampling):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=int(quality), subsampling=int(subsampling))
    return b.getvalue()


@pytest.fixture(scope="module")
def fixtures(golden):
    g = golden("jpeg_encode")
    return [(str(n), g[f"rgb_{i}"], int(g["quality"][i]), int(g["subsampling"][i]), g[f"jpg_{i}"].tobytes()) for i, n in enumerate(g["names"])]


@pytest.fixture(scope="module")
def corpus(fixtures):
    """Every fixture and 300 random images -- 1..69 pixels a side, the five qualities, the three samplings, noise / smooth / bilevel
    -- each with the file PIL writes for it here: (name, rgb, quality, subsampling, bytes).  Computed once, never written to."""
    rng = np.random.default_rng(23)
    out = [(n, rgb, q, s, _pil(rgb, q, s)) for n, rgb, q, s, _ in fixtures]
    for t in range(300):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        if t % 3 == 0:
            a = rng.integers(0, 256, (h, w, 3))
        elif t % 3 == 1:
            yy, xx = np.mgrid[0:h, 0:w]
            a = ((np.sin(xx / 7.0) + np.cos(yy / 5.0)) * 60 + 128)[..., None] + rng.normal(0, 8, (h, w, 3))
        else:
            a = rng.integers(0, 2, (h, w, 3)) * 255
        rgb = np.clip(a, 0, 255).astype(np.uint8)
        q, s = QUALITIES[(t // 3) % 5], int(rng.integers(0, 3))
        out.append((f"random {t}: {w}x{h} q{q} s{s}", rgb, q, s, _pil(rgb, q, s)))
    return out


def _groups(corpus):
    """The corpus by (quality, subsampling): one plan / one write_batch call takes one pair."""
    by = {}
    for c in corpus:
        by.setdefault((c[2], c[3]), []).append(c)
    return by


def _write(lib, coeffs, desc, threads=0, room=None, cap=None):
    desc = desc.copy()
    # by default: the header and the most a block can take (csrc/jpeg_encode.hip BLOCK_ROOM)
    out = np.zeros(room if room is not None else 623 * len(desc) + 420 * (coeffs.size // 64), dtype=np.uint8)
    offsets, need = jpeg.write_batch(lib, np.ascontiguousarray(coeffs.reshape(-1)), desc, out, threads, cap_bytes=cap)
    return out, offsets, need, desc


def test_fixture_is_what_pil_writes_here(fixtures):
    """The committed bytes are PIL's on the machine that wrote them; this machine's PIL agrees (where it does not, the oracle
    itself moved and the generator has to be looked at, not the encoder)."""
    for name, rgb, q, s, blob in fixtures:
        assert _pil(rgb, q, s) == blob, name


def test_forward_numpy_equals_the_coefficients_in_pils_files_over_the_whole_padded_grid(lib, corpus):
    """Dummy blocks included: the entropy pass of the decoder reads every block of the MCU-padded grid out of PIL's file."""
    for name, rgb, q, s, blob in corpus:
        coeffs = np.zeros(64 * 512, dtype=np.int16)
        desc = np.zeros(1, dtype=jpeg.DESC)
        jpeg.entropy_batch(lib, [blob], coeffs, desc)
        assert desc["status"][0] == jpeg.OK, name
        mine, md = jpeg.forward_numpy([rgb], q, s)
        for f in ("width", "height", "ncomp", "hs", "vs", "bw", "bh", "tq", "n_blocks", "qt"):
            np.testing.assert_array_equal(md[f][0], desc[f][0], err_msg=f"{name}: {f}")
        np.testing.assert_array_equal(mine, coeffs[:mine.size].reshape(-1, 64), err_msg=name)


def test_plan_equals_its_numpy_statement_and_refuses_impossible_sizes(lib):
    sizes = [(1, 1), (17, 33), (0, 5), (64, 48), (5, 0), (65536, 2), (65535, 1), (40, 38)]
    for q in (1, 95):
        for s in (0, 1, 2):
            desc, need = jpeg.plan(lib, sizes, q, s)
            want = jpeg.plan_numpy(sizes, q, s)
            assert desc.tobytes() == want.tobytes()
            assert need == int(want["n_blocks"].sum())
            assert desc["status"].tolist() == [0, 0, 1, 0, 1, 1, 0, 0]
            assert set(desc["reason"][desc["status"] != 0].tolist()) == {jpeg.R_ENC_SIZE}
            assert (np.diff(desc["coef_block"]) == desc["n_blocks"][:-1]).all()
    with pytest.raises(ValueError):
        jpeg.plan(lib, [(8, 8)], 0, 2)
    with pytest.raises(ValueError):
        jpeg.plan(lib, [(8, 8)], 95, 3)


def test_write_batch_of_forward_numpy_equals_pils_bytes_for_1_3_and_16_threads(lib, corpus):
    for (q, s), group in _groups(corpus).items():
        coeffs, desc = jpeg.forward_numpy([c[1] for c in group], q, s)
        first = None
        for threads in (1, 3, 16):
            out, offsets, need, d = _write(lib, coeffs, desc, threads)
            assert (d["status"] == jpeg.OK).all()
            assert need == offsets[-1] == sum(len(c[4]) for c in group)
            for i, c in enumerate(group):
                assert out[offsets[i]:offsets[i + 1]].tobytes() == c[4], c[0]
            first = out[:need].tobytes() if first is None else first
            assert out[:need].tobytes() == first


def test_a_short_buffer_is_reported_and_nothing_is_written_behind_it(lib, fixtures):
    group = [c for c in fixtures if (c[2], c[3]) == (95, 2)]
    assert len(group) >= 4
    coeffs, desc = jpeg.forward_numpy([c[1] for c in group], 95, 2)
    lens = [len(c[4]) for c in group]
    total = sum(lens)
    # room for the first two files and some of the third; the smaller ones behind it that still fit are written, as in the decoder
    cap = lens[0] + lens[1] + lens[2] // 2
    room = total + 4096
    out = np.full(room, 0xA5, dtype=np.uint8)
    d = desc.copy()
    offsets, need = jpeg.write_batch(lib, np.ascontiguousarray(coeffs.reshape(-1)), d, out, 3, cap_bytes=cap)
    assert need == total
    assert offsets[-1] <= cap
    assert (out[cap:] == 0xA5).all()
    assert d["status"][2] == jpeg.NOT_HANDLED and d["reason"][2] == jpeg.R_NO_SPACE and offsets[3] == offsets[2]
    used = 0
    for i, c in enumerate(group):
        if d["status"][i] == jpeg.OK:
            assert out[offsets[i]:offsets[i + 1]].tobytes() == c[4], c[0]
            used += lens[i]
        else:
            assert d["reason"][i] == jpeg.R_NO_SPACE and lens[i] > cap - used and offsets[i + 1] == offsets[i]
    assert d["status"][:2].tolist() == [jpeg.OK, jpeg.OK]
    # no room at all, and a NULL buffer of no room
    d = desc.copy()
    offsets, need = jpeg.write_batch(lib, np.ascontiguousarray(coeffs.reshape(-1)), d, out, 1, cap_bytes=0)
    assert need == total and not offsets.any() and (d["reason"] == jpeg.R_NO_SPACE).all() and (out[cap:] == 0xA5).all()
    # the exact size fits
    out, offsets, need, d = _write(lib, coeffs, desc, 0, room=total + 64, cap=total)
    assert (d["status"] == jpeg.OK).all() and offsets[-1] == total and not out[total:].any()


def test_a_descriptor_the_plan_did_not_write_and_a_coefficient_without_a_code_are_refused(lib, fixtures):
    _, rgb, q, s, blob = fixtures[-1]
    coeffs, desc = jpeg.forward_numpy([rgb, rgb], q, s)
    bad = desc.copy()
    bad["bw"][0][0] += 1
    out, offsets, need, d = _write(lib, coeffs, bad)
    assert d["status"].tolist() == [jpeg.NOT_HANDLED, jpeg.OK] and d["reason"][0] == 19
    assert offsets[1] == 0 and out[:offsets[2]].tobytes() == blob
    wild = coeffs.copy()
    wild[3, 5] = 1024   # 11 bits of AC: the standard table stops at 10
    out, offsets, need, d = _write(lib, wild, desc)
    assert d["status"].tolist() == [jpeg.NOT_HANDLED, jpeg.OK] and d["reason"][0] == 16
    assert out[:offsets[2]].tobytes() == blob


def test_quant_tables_equal_the_tables_in_pils_files_for_every_quality(lib):
    rgb = np.zeros((8, 8, 3), dtype=np.uint8)
    for q in range(1, 101):
        info = jpeg.probe(lib, _pil(rgb, q, 2))
        qt = jpeg.quant_tables(lib, q)
        np.testing.assert_array_equal(qt[0], info["qt"][0], err_msg=f"quality {q}")
        np.testing.assert_array_equal(qt[1], info["qt"][1], err_msg=f"quality {q}")
        np.testing.assert_array_equal(qt, jpeg.quant_tables_numpy(q))
    for q in (0, 101):
        with pytest.raises(ValueError):
            jpeg.quant_tables(lib, q)


def test_our_files_are_read_back_by_our_decoder(lib, fixtures):
    for name, rgb, q, s, _ in fixtures:
        coeffs, desc = jpeg.forward_numpy([rgb], q, s)
        out, offsets, _, _ = _write(lib, coeffs, desc)
        blob = out[:offsets[1]].tobytes()
        info = jpeg.probe(lib, blob)
        assert info["status"] == jpeg.OK and (info["width"], info["height"]) == (rgb.shape[1], rgb.shape[0]), name
        back = np.zeros(coeffs.size, dtype=np.int16)
        d = np.zeros(1, dtype=jpeg.DESC)
        jpeg.entropy_batch(lib, [blob], back, d)
        assert d["status"][0] == jpeg.OK, name
        np.testing.assert_array_equal(back.reshape(-1, 64), coeffs, err_msg=name)
