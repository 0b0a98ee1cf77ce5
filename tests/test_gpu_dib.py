"""Uncompressed BGR video on the GPU: avcer_dib_frames / dib.unpack_frames against dib.unpack_numpy (which tests/test_dib_cpu.py pins to
PIL's BMP reader), tolerance zero.  Shapes are the smallest at which the kernel can go wrong: rows of 3, 15, 48, 51, 66, 192 and 1023
bytes (shorter than one 16-byte piece, exactly three, no multiple of 16 or of 4, more than a wave's 64 pieces), one and several
rows and frames, both bit depths, orientations and channel orders, source frames at every byte residue mod 16 (chunk data in an
AVI file are only 2-byte aligned), the batch at every residue too, a frame read twice, a short last pass.

Bounds: the batch lies between 64 guard bytes on each side, which must come back unchanged; the source span ends where its tensor
ends and starts `lead` bytes into it, and the bytes in front of it are filled with another pattern on a second run, which must not
change a byte of the result.  Nothing here tries to provoke a fault: values and guards alone are checked."""
import numpy as np
import pytest
import torch

from avcer_amd import dib

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS, COUNTS = (1, 5, 16, 17, 22, 64, 341), (1, 2, 7), (1, 3)
GUARD, FILL = 64, 0xA5


def source(n, h, w, bits, seed):
    """n random frames as chunks (random padding and fourth bytes) and what they unpack to, top-down BGR."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, dib.stride_of(w, bits) * h, dtype=np.uint8).tobytes() for _ in range(n)]


def unpack(engine, chunks, order, h, w, bits, bottom_up, bgr, lead, shift, front=0):
    """avcer_dib_frames on a span that holds `chunks` back to back behind `lead` bytes (each padded by 2 more than the one before, so
    that every frame has another residue), frame k = chunks[order[k]], into a batch `shift` bytes off a 64-byte border, between
    guard bands.  Returns the batch on the host."""
    parts, offsets, at = [bytes([front]) * lead], [], lead
    for k, c in enumerate(chunks):
        offsets.append(at)
        pad = 2 * k + (len(c) & 1)
        parts.append(c + bytes([front]) * pad)
        at += len(c) + pad
    last = len(chunks[-1])
    blob = b"".join(parts)[:offsets[-1] + last]                      # the span ends with the last frame's last byte ...
    whole = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(engine.device)
    span = whole[0:]                                                 # ... and the tensor with the span
    table = torch.tensor([offsets[i] for i in order], dtype=torch.int64, device=engine.device)
    n = len(order)
    size = n * h * w * 3
    buf = torch.full((GUARD + 16 + size + GUARD,), FILL, dtype=torch.uint8, device=engine.device)
    out = buf[GUARD + shift:GUARD + shift + size].view(n, h, w, 3)
    got = engine.dib_frames(span, table, n, h, w, bits, bottom_up, bgr=bgr, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:GUARD + shift] == FILL).all() and (host[GUARD + shift + size:] == FILL).all(), "a byte outside the batch was written"
    return host[GUARD + shift:GUARD + shift + size].reshape(n, h, w, 3)


@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("bottom_up", [True, False])
def test_the_kernel_equals_unpack_numpy_inside_guard_bands(engine, bits, bottom_up):
    case = 0
    seen = set()
    for w in WIDTHS:
        for h in HEIGHTS:
            for n in COUNTS:
                chunks = source(n, h, w, bits, 100 * w + 10 * h + n)
                for bgr in (True, False):
                    want = dib.unpack_numpy(chunks, h, w, bits, bottom_up, bgr=bgr)
                    lead, shift = case % 16, (5 * case + 3) % 16      # every residue of the span and of the batch, odd ones included
                    seen.add(lead)
                    got = unpack(engine, chunks, list(range(n)), h, w, bits, bottom_up, bgr, lead, shift)
                    np.testing.assert_array_equal(got, want, err_msg=f"{w} x {h} n={n} bgr={bgr} lead={lead} shift={shift}")
                    case += 1
    assert seen == set(range(16))


@pytest.mark.parametrize("bits", [24, 32])
def test_every_residue_of_source_and_batch(engine, bits):
    """One awkward shape (rows of 51 bytes, source rows of 52 / 68) at all 16 x 16 alignments of source against batch; a frame read twice;
    the bytes in front of the span do not matter."""
    w, h = 17, 2
    chunks = source(2, h, w, bits, 7)
    order = [0, 1, 0]                                                # a repeated frame: the same offset twice
    for bgr in (True, False):
        want = dib.unpack_numpy([chunks[i] for i in order], h, w, bits, True, bgr=bgr)
        for lead in range(16):
            for shift in range(16):
                got = unpack(engine, chunks, order, h, w, bits, True, bgr, lead, shift)
                np.testing.assert_array_equal(got, want, err_msg=f"bgr={bgr} lead={lead} shift={shift}")
            again = unpack(engine, chunks, order, h, w, bits, True, bgr, lead, 3, front=0xFF)
            np.testing.assert_array_equal(again, want, err_msg=f"bgr={bgr} lead={lead}: bytes outside the frames reached the result")


def test_a_frame_outside_the_span_is_zero_and_bad_arguments_raise(engine):
    w, h, bits = 5, 2, 24
    chunks = source(2, h, w, bits, 9)
    span = torch.from_numpy(np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()).to(engine.device)
    size = len(chunks[0])
    table = torch.tensor([0, size + 1, -1, size], dtype=torch.int64, device=engine.device)   # 1: one byte short of the span; 2: negative
    got = engine.dib_frames(span, table, 4, h, w, bits, True).cpu().numpy()
    want = dib.unpack_numpy(chunks, h, w, bits, True)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[3], want[1])
    assert not got[1].any() and not got[2].any()
    with pytest.raises(ValueError, match="bits"):
        engine.dib_frames(span, table, 4, h, w, 16, True)
    with pytest.raises(ValueError, match="out must be"):
        engine.dib_frames(span, table, 4, h, w, bits, True, out=torch.empty(4, h, w + 1, 3, dtype=torch.uint8, device=engine.device))
    with pytest.raises(ValueError, match="offsets"):
        engine.dib_frames(span, table.to(torch.int32), 4, h, w, bits, True)


@pytest.mark.parametrize("bits,bottom_up", [(24, True), (32, False)])
def test_unpack_frames_in_passes(engine, bits, bottom_up):
    w, h = 22, 7
    a, b = source(2, h, w, bits, 11)
    chunks = [memoryview(a), memoryview(a), memoryview(b)]            # the same view twice: a dropped frame repeats its predecessor
    want = dib.unpack_numpy(chunks, h, w, bits, bottom_up)
    for per in (2, 1, 64):                                            # 2: a short last pass
        got = dib.unpack_frames(engine, chunks, h, w, bits, bottom_up, frames_per_pass=per)
        assert got.is_cuda and got.dtype == torch.uint8
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(per))
    rgb = dib.unpack_frames(engine, chunks, h, w, bits, bottom_up, bgr=False, frames_per_pass=2)
    np.testing.assert_array_equal(rgb.cpu().numpy(), want[..., ::-1])
    assert dib.unpack_frames(engine, [], h, w, bits, bottom_up).shape == (0, h, w, 3)
    with pytest.raises(ValueError, match="frame 2"):
        dib.unpack_frames(engine, [a, a, b[:-1]], h, w, bits, bottom_up)
    with pytest.raises(ValueError, match="frames_per_pass"):
        dib.unpack_frames(engine, chunks, h, w, bits, bottom_up, frames_per_pass=0)
