"""The stage-3 tail (csrc/fused.hip bneck_tail2_kernel) through its kernel-level entry avcer_bneck_tail:
    OUT = relu(T2 W3^T + b3 + X),  T1N = relu(OUT W1N^T + b1n),  planes 256,
at M = 1 ... 300 positions -- the forward passes reach the kernel only above 16384.  The sizes sit on either side of one wave's 16
positions and of one block's 128, plus two full blocks with 44 ragged rows."""
import functools

import pytest
import torch

from avcer_amd._lib import AvcerError
from avcer_amd.sp32 import from_sp32, to_sp32
from test_gpu_kernels import _desc, _tol

pytestmark = pytest.mark.gpu

P = 256
SIZES = [1, 15, 16, 17, 127, 128, 129, 300]


@functools.lru_cache(maxsize=1)
def _case():
    """Inputs as in test_bneck_chain_vs_float64 (activations rand * 2, weights randn / sqrt(K), biases randn * 0.3: everything far
    from the 65504 range limit) for the largest M, and the float64 reference of the values the kernel sees (the sp32 inputs
    decoded).  Rows are independent, so every smaller M is a prefix of both."""
    g = torch.Generator().manual_seed(256 + 300)
    m = max(SIZES)
    t2, x = to_sp32(torch.rand(m, P, generator=g) * 2), to_sp32(torch.rand(m, 4 * P, generator=g) * 2)
    w3 = torch.randn(4 * P, P, generator=g) / P ** 0.5
    w1n = torch.randn(P, 4 * P, generator=g) / (4 * P) ** 0.5
    b3, b1n = torch.randn(4 * P, generator=g) * 0.3, torch.randn(P, generator=g) * 0.3
    out = torch.relu(from_sp32(t2).double() @ w3.double().t() + b3.double() + from_sp32(x).double())
    t1n = torch.relu(out @ w1n.double().t() + b1n.double())
    return t2, x, w3, w1n, b3, b1n, out, t1n


def _device_case(engine, m):
    t2, x, w3, w1n, b3, b1n, _, _ = _case()
    dev = engine.device
    return (t2[:m].contiguous().to(dev), x[:m].contiguous().to(dev), engine.split_weight_rows(w3), b3.to(dev),
            engine.split_weight_rows(w1n), b1n.to(dev))


def _tail(engine, m, t2, x, w3, b3, w1n, b1n):
    out = torch.full((m, 8 * P), 0x7fc0, dtype=torch.int16, device=engine.device)    # NaN-filled sp32
    t1n = torch.full((m, 2 * P), 0x7fc0, dtype=torch.int16, device=engine.device)
    engine.bneck_tail(P, m, t2, x, out, t1n, w3, b3, w1n, b1n)
    torch.cuda.synchronize()
    return out.cpu(), t1n.cpu()


@pytest.mark.parametrize("m", SIZES)
def test_bneck_tail_vs_float64(engine, m):
    out, t1n = _tail(engine, m, *_device_case(engine, m))
    ref_out, ref_t1n = (r[:m] for r in _case()[6:])
    e0 = (from_sp32(out).double() - ref_out).abs().max().item()
    e1 = (from_sp32(t1n).double() - ref_t1n).abs().max().item()
    print(f"bneck_tail M={m}: max|out err| {e0:.2e} (max|out| {ref_out.abs().max().item():.2f}, bound {_tol(5, ref_out):.2e}), "
          f"max|t1n err| {e1:.2e} (max|t1n| {ref_t1n.abs().max().item():.2f}, bound {_tol(5, ref_t1n):.2e})")
    # The bound test_gpu_kernels._tol grants dtype 5: 8e-5 x max|ref| (4.2e-4 ... 5.6e-4 for out, 3.1e-4 ... 4.7e-4 for t1n here).
    # Measured on an MI355X, max|out err| / max|t1n err|: M = 1: 1.03e-6 / 1.97e-6; M = 15, 16, 17: 1.95e-6 / 3.34e-6;
    # M = 127, 128, 129: 2.65e-6 / 4.45e-6; M = 300: 2.65e-6 / 4.81e-6 -- two orders inside the bound, at the sp32 encoding's own step
    # (2^-22 relative) for outputs of magnitude 5-7
    assert e0 < _tol(5, ref_out) and e1 < _tol(5, ref_t1n)


@pytest.mark.parametrize("m", SIZES)
def test_bneck_tail_is_bit_identical_to_the_pair(engine, m):
    """Below kTailPairRows positions run_bneck_stage (csrc/visual.hip) issues the same two contractions as two avcer_conv_gemm
    launches and states that they are the same arithmetic: conv3 with the residual x and ReLU, then the next block's conv1 on OUT,
    dtype 5, no scale vector.  Both raw int16 outputs must be equal."""
    t2, x, w3, b3, w1n, b1n = args = _device_case(engine, m)
    out, t1n = _tail(engine, m, *args)
    dev = engine.device
    p_out = torch.full((m, 8 * P), 0x7fc0, dtype=torch.int16, device=dev)
    p_t1n = torch.full((m, 2 * P), 0x7fc0, dtype=torch.int16, device=dev)
    d3 = _desc(batch=m, cin=P, x_stride_b=P, x_stride_h=P, x_stride_w=P, n=4 * P, y_ld=4 * P, r_ld=4 * P, act=1)
    engine.conv_gemm(d3, 5, t2, w3, None, b3, x, p_out)
    d1 = _desc(batch=m, cin=4 * P, x_stride_b=4 * P, x_stride_h=4 * P, x_stride_w=4 * P, n=P, y_ld=P, r_ld=P, act=1)
    engine.conv_gemm(d1, 5, p_out, w1n, None, b1n, None, p_t1n)
    torch.cuda.synchronize()
    assert torch.equal(out, p_out.cpu())
    assert torch.equal(t1n, p_t1n.cpu())


def test_bneck_tail_argument_errors(engine):
    """planes other than 256, no positions and a missing t1n are AVCER_EINVAL with a message; nothing is launched."""
    m = 16
    t2, x, w3, b3, w1n, b1n = _device_case(engine, m)
    out = torch.zeros(m, 8 * P, dtype=torch.int16, device=engine.device)
    t1n = torch.zeros(m, 2 * P, dtype=torch.int16, device=engine.device)
    torch.cuda.synchronize()
    engine.gemm_stats(reset=True)
    for planes, rows, t1n_arg, msg in ((128, m, t1n, "planes 128"), (P, 0, t1n, "bad arguments"), (P, m, None, "bad arguments")):
        with pytest.raises(AvcerError, match=msg) as e:
            engine.bneck_tail(planes, rows, t2, x, out, t1n_arg, w3, b3, w1n, b1n)
        assert e.value.code == -1
    assert engine.gemm_stats()[0] == 0
    torch.cuda.synchronize()
    assert not out.any() and not t1n.any()
