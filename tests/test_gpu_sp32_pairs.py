"""Every kernel-level entry that STORES sp32 pairs writes, bit for bit, the pair avcer_amd/sp32.py:to_sp32 defines: hi = the
f32 value rounded to fp16 (nearest even), lo = fp16(value - hi), both from one f32 number (csrc/split_dev.h).

One [64, 256] f32 tensor carries the cases a split can get wrong: normals at three scales, values below 2^-3 (subnormal lo
half), exact fp16 ties with their f32 neighbours (where two roundings of "the same" value disagree by one hi ulp), +-0.0
and +-65519, the largest magnitudes inside the range contract -- so the overflow counter must read 0 after every site.
Overflow, inf and NaN are covered by test_x3_overflow_is_nan_not_a_wrong_number and test_gpu_edges.py.

Sites: avcer_split_weights on the raw tensor; avcer_maxpool2 in sp32 storage over constant 2 x 2 windows (an identity);
avcer_conv_gemm with a 256 x 256 identity weight at dtype 4 (f32 in, split on the fly, staged epilogue), 5 (staged), 7
(weights-direct) and 9 (skinny).
The pooling reads the pairs of the raw tensor, to_sp32(x0): what it loads is from_sp32 of them (hi + lo in f32, the
kernel's own read), a maximum over four equal values is that value -- -0.0 included, which a value that underflows both
halves leaves behind --, so it must store to_sp32(from_sp32(to_sp32(x0))).
The contractions get x = from_sp32(to_sp32(x0)) + 0.0: exactly a pair, and without -0.0 (an MFMA accumulator starts at +0,
and +0 + -0 = +0: the identity product of -0.0 IS +0.0), so the identity product (one non-zero term per output, weights
scaled by a power of two) is exact in f32 and the stored bits must equal to_sp32(x).
The expectation is the Python definition alone."""
import pytest
import torch

from avcer_amd.sp32 import from_sp32, to_sp32
from test_gpu_kernels import _desc

pytestmark = pytest.mark.gpu

M, C = 64, 256


def _input():
    g = torch.Generator().manual_seed(20)
    x = torch.empty(M, C)
    x[0:8] = torch.randn(8, C, generator=g) * 1e-3
    x[8:24] = torch.randn(16, C, generator=g)
    x[24:32] = torch.randn(8, C, generator=g) * 1e3
    x[32:40] = (torch.rand(8, C, generator=g) - 0.5) * 0.25          # |x| < 2^-3: the lo half is a subnormal fp16
    x[40:48] = torch.randn(8, C, generator=g) * 2.0 ** -16           # ... and most of the hi half's bits are gone too
    # exact fp16 ties (odd multiples of half an fp16 ulp, at several exponents and both signs) and their f32 neighbours
    k = torch.arange(C, dtype=torch.float32)
    tie = (1.0 + (2.0 * k + 1.0) * 2.0 ** -11) * 2.0 ** ((torch.arange(C) % 24) - 12).float() * (1.0 - 2.0 * (torch.arange(C) % 2)).float()
    x[48:50] = tie
    x[50:52] = tie * (1.0 + 2.0 ** -23)
    x[52:54] = tie * (1.0 - 2.0 ** -23)
    x[54] = 1.0 + 2.0 ** -11
    x[55] = (1.0 + 2.0 ** -11) * (1.0 + 2.0 ** -23)
    x[56] = (1.0 + 2.0 ** -11) * (1.0 - 2.0 ** -23)
    x[57:64] = torch.randn(7, C, generator=g)
    x[57, 0::2], x[57, 1::2] = 0.0, -0.0
    x[58, 0::2], x[58, 1::2] = 65519.0, -65519.0                     # below 65520: in range, hi = 65504, lo = 15
    x[59, 0::2], x[59, 1::2] = -2.0 ** -30, 2.0 ** -30               # both halves underflow: the pair is (-0, -0) / (+0, +0)
    assert x.abs().max() == 65519.0 and torch.isfinite(x).all()
    return x


@pytest.fixture(scope="module")
def pairs():
    """(x0, x, to_sp32(x0), to_sp32(x)): the raw tensor, the same made exactly representable as pairs (and free of -0.0), and
    what a store site must write for each (int16 [64, 512], CPU)."""
    x0 = _input()
    x = from_sp32(to_sp32(x0)) + 0.0  # -0.0 (a split -0.0, or a value that underflows both halves) -> +0.0
    want = to_sp32(x)
    assert torch.equal(from_sp32(want), x)  # x IS a pair: reading it back loses nothing
    assert not torch.signbit(x[x == 0]).any()
    return x0, x, to_sp32(x0), want


def _same_bits(got, want):
    got = got.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {want.numel()} halves differ, first at {bad[0].tolist()}: " \
                             f"{got[tuple(bad[0])].item() & 0xffff:#06x} against {want[tuple(bad[0])].item() & 0xffff:#06x}"


def test_split_weights_writes_the_python_pair(engine, pairs):
    x0, x, want0, want = pairs
    engine.x3_overflow_clear()
    _same_bits(engine.split_weights(x0.to(engine.device)).reshape(M, 2 * C), want0)
    _same_bits(engine.split_weights(x.to(engine.device)).reshape(M, 2 * C), want)
    assert engine.x3_overflow_count() == 0


def test_maxpool2_sp32_identity_writes_the_python_pair(engine, pairs):
    x0, x, want0, want = pairs
    read = from_sp32(want0)  # what the kernel loads from the raw tensor's pairs; keeps the -0.0 of the (-0, -0) pairs
    assert torch.signbit(read[read == 0]).any() and not torch.signbit(read[read == 0]).all()
    # output grid 8 x 8 positions of 256 channels; every 2 x 2 input window holds its output's pair four times
    up = want0.reshape(1, 8, 8, 2 * C).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
    engine.x3_overflow_clear()
    y = engine.maxpool2(up.to(engine.device), sp32=True)
    _same_bits(y.reshape(M, 2 * C), to_sp32(read))
    assert engine.x3_overflow_count() == 0


@pytest.mark.parametrize("dtype", [4, 5, 7, 9])
def test_conv_gemm_identity_writes_the_python_pair(engine, pairs, dtype):
    x0, x, want0, want = pairs
    dev = engine.device
    eye = torch.eye(C, dtype=torch.float32, device=dev)
    w = engine.split_weight_rows(eye) if dtype in (4, 5) else engine.weight_frags(eye)
    xd = x.to(dev).contiguous() if dtype == 4 else want.to(dev)
    d = _desc(batch=M, cin=C, x_stride_b=C, x_stride_h=C, x_stride_w=C, n=C, y_ld=C, r_ld=C)
    y = torch.full((M, 2 * C), -3, dtype=torch.int16, device=dev)
    engine.x3_overflow_clear()
    engine.conv_gemm(d, dtype, xd, w, None, None, None, y)
    _same_bits(y, want)
    assert engine.x3_overflow_count() == 0
