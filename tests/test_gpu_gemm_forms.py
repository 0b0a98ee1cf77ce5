"""The forms of avcer_conv_gemm that the layer-sized shapes of test_gpu_kernels.py never reach (csrc/gemm.hip).

A. conv_gemm_kernel<MODE, OUT, 128>: launch_t takes the 128-wide tile only for N % 128 == 0, K > 128 and more than block_slots / 4
   tiles, about 2.1 M outputs in one launch.  avcer_conv_desc.tile_n forces the width, so every case here runs dtypes 0-6 at
   tile_n = 64 AND 128 on shapes of a few hundred rows: each width against float64 torch on the operands as the kernel saw them
   (decoded bf16 / sp32), within the _tol table of test_gpu_kernels.py, and the two widths BIT-IDENTICAL on the raw output storage
   -- an element's K order does not depend on the tile width, which is what include/avcer_hip.h promises of tile_n.  Outputs are
   prefilled with NaN (0x7fc0 halves for sp32), so a tile that is never written fails the float64 comparison.
B. The straddling gather (cin not a multiple of the K-step, AVCER_ISSUE_TILES' last branch): a lane's channel index moves into the
   next filter tap at most ONCE, which is enough only while bk - vec - gcd(cin, bk) < cin.  The cins for which it is enough are
   held to float64 F.conv2d with zero padding and with channel padding in every pixel (x_stride_w > cin; a dense layout hides a
   wrong tap behind the same linear address); the others must be refused with AVCER_EINVAL and leave the output alone."""
import pytest
import torch
import torch.nn.functional as F

from avcer_amd._lib import AvcerError
from test_gpu_kernels import A_KIND, CONVS, O_KIND, _act, _dec, _desc, _enc, _run, _tol

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128)
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "sp32": torch.int16}
ALL = [0, 1, 2, 3, 4, 5, 6]
NAN = float("nan")


def _fill(kind, shape, dev):
    """A NaN-filled output in the storage of `kind`; `shape` counts elements (an sp32 element is two int16)."""
    if kind == "sp32":
        return torch.full((*shape[:-1], 2 * shape[-1]), 0x7fc0, dtype=torch.int16, device=dev)
    return torch.full(tuple(shape), NAN, dtype=TORCH[kind], device=dev)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _both_widths(engine, d, dtype, x, w, scale, bias, res, out_shape, ref_of, x2=None, off=0):
    """_run of test_gpu_kernels.py with a raw NaN prefill, at tile_n = 64 and 128.  w f32 [groups * n][K]; out_shape = the output
    tensor in elements, whose channels [off, off + groups * n) the launch writes; ref_of(x, x2, w, r) -> float64 reference of those
    channels from the decoded operands.  Asserts each width against it, the fill in every other channel, and equal bits."""
    dev = engine.device
    ak, ok = A_KIND[dtype], O_KIND[dtype]
    xd = _enc(x, ak, dev)
    x2d = None if x2 is None else _enc(x2, ak, dev)
    wd = w.to(dev, torch.bfloat16 if ak == "bf16" else torch.float32).contiguous()
    w_arg = engine.split_weight_rows(wd) if dtype >= 3 else wd
    sd = None if scale is None else scale.to(dev, torch.float32)
    bd = None if bias is None else bias.to(dev, torch.float32)
    rd = None if res is None else _enc(res, ok, dev)
    ref = ref_of(_dec(xd, ak).double(), None if x2d is None else _dec(x2d, ak).double(), wd.double().cpu(),
                 None if rd is None else _dec(rd, ok).double())
    tol = _tol(dtype, ref)
    ntot = d.n * max(1, d.groups)
    mul = 2 if ok == "sp32" else 1
    fill = _bits(_fill(ok, out_shape, "cpu"))
    raw = {}
    for tn in WIDTHS:
        d.tile_n = tn
        yd = _fill(ok, out_shape, dev)
        if x2d is None:
            engine.conv_gemm(d, dtype, xd, w_arg, sd, bd, rd, yd)
        else:
            engine.conv_gemm_dual(d, dtype, xd, x2d, w_arg, sd, bd, rd, yd)
        torch.cuda.synchronize()
        raw[tn] = yd.cpu()
        got = _dec(raw[tn], ok).double()[..., off:off + ntot]
        assert got.shape == ref.shape
        err = (got - ref).abs().max().item()
        print(f"dtype {dtype} tile_n {tn}: max|err| {err:.3e} (tol {tol:.3e}), unwritten {int(torch.isnan(got).sum())}")
        assert err < tol, (tn, err, tol)                          # a NaN left in the output fails here
        b = _bits(raw[tn])
        assert torch.equal(b[..., :mul * off], fill[..., :mul * off]), tn
        assert torch.equal(b[..., mul * (off + ntot):], fill[..., mul * (off + ntot):]), tn
    differ = int((_bits(raw[64]) != _bits(raw[128])).sum())
    assert differ == 0, f"{differ} storage words differ between tile_n 64 and 128"


def _linear_case(engine, dtype, m, k, n, strided=False, act=1, res_after=0, has_scale=True, has_bias=True, has_res=True):
    g = torch.Generator().manual_seed(m + k + n + 7 * act)
    x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
    scale, bias = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    ld, off = (n + 64, 32) if strided else (n, 0)
    res = torch.randn(m, ld, generator=g)
    d = _desc(batch=m, cin=k, x_stride_b=k, x_stride_h=k, x_stride_w=k, n=n, y_ld=ld, y_coff=off, r_ld=ld, r_coff=off, act=act,
              res_after_act=res_after)

    def ref_of(xd, _, wd, rd):
        v = xd @ wd.t()
        if has_scale:
            v = v * scale.double()
        if has_bias:
            v = v + bias.double()
        r = rd[:, off:off + n] if has_res else 0.0
        return _act(v, act) + r if res_after else _act(v + r, act)

    _both_widths(engine, d, dtype, x, w, scale if has_scale else None, bias if has_bias else None, res if has_res else None, (m, ld),
                 ref_of, off=off)


# ----------------------------------------------------------------------------- A. both tile widths
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m,k,n", [(129, 192, 128), (300, 192, 384), (1, 256, 256)])
def test_linear_ragged_m(engine, dtype, m, k, n, strided):
    """N = 384: three 128-wide column tiles; M = 129: a one-row tile; M = 1: a single row; K = 192: three bf16 K-steps, six f32.
    Strided: y_ld = r_ld = n + 64, y_coff = r_coff = 32, the 64 gap columns keep their fill."""
    _linear_case(engine, dtype, m, k, n, strided)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("act,res_after,has_scale,has_bias,has_res",
                         [(2, 1, True, True, True), (3, 1, True, True, True), (1, 0, False, True, True), (2, 1, True, False, True),
                          (3, 0, True, True, False)],
                         ids=["gelu+r", "gelu_fast+r", "no_scale", "no_bias", "no_residual"])
def test_epilogue_variants(engine, dtype, act, res_after, has_scale, has_bias, has_res):
    """act 2 / 3 with the residual behind the activation, and a launch without scale, without bias, without residual."""
    _linear_case(engine, dtype, 300, 192, 128, False, act, res_after, has_scale, has_bias, has_res)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m", [1100, 1409])
def test_block_order(engine, dtype, m):
    """ntm = 9 / 12 row tiles: the last group of the gm = 8 sweep holds 1 / 4 of them; nwg = 36 / 18 and 48 / 24 across the two
    widths, so the XCD remap runs with nwg % 8 != 0 and == 0, ntn >= 2 either way.  A tile visited twice leaves another unwritten."""
    _linear_case(engine, dtype, m, 64, 256)


def _conv_case(engine, dtype, cfg):
    b, h, w_, c, kh, kw, s, p, dil, n, act = cfg
    g = torch.Generator().manual_seed(sum(v if isinstance(v, int) else sum(v) for v in cfg))
    x = torch.randn(b, h, w_, c, generator=g)
    w = torch.randn(n, kh * kw * c, generator=g) / (kh * kw * c) ** 0.5
    scale, bias = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    (p, pw), (dil, dw) = (p, dil) if isinstance(p, tuple) else ((p, p), (dil, dil))
    oh = (h + 2 * p - dil * (kh - 1) - 1) // s + 1
    ow = (w_ + 2 * pw - dw * (kw - 1) - 1) // s + 1
    res = torch.randn(b, oh, ow, n, generator=g)
    d = _desc(batch=b, in_h=h, in_w=w_, out_h=oh, out_w=ow, cin=c, kh=kh, kw=kw, stride_h=s, stride_w=s, pad_h=p, pad_w=pw, dil_h=dil,
              dil_w=dw, x_stride_b=h * w_ * c, x_stride_h=w_ * c, x_stride_w=c, n=n, y_ld=n, r_ld=n, act=act)

    def ref_of(xd, _, wd, rd):
        v = F.conv2d(xd.permute(0, 3, 1, 2), wd.reshape(n, kh, kw, c).permute(0, 3, 1, 2), None, s, (p, pw), (dil, dw))
        return _act(v.permute(0, 2, 3, 1) * scale.double() + bias.double() + rd, act)

    _both_widths(engine, d, dtype, x, w, scale, bias, res, (b, oh, ow, n), ref_of)


# cin a whole number of K-steps (32 elements; bf16: 64): ONE step is the uniform gather in (ky, kx, chunk) order, more than one
# the tap_inner order (launch_conv_gemm)
_PADDED = [(dt, c) for dt in (0, 3, 4, 5, 6) for c in (32, 64)] + [(dt, c) for dt in (1, 2) for c in (64, 128)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype,cin", _PADDED)
def test_padded_3x3(engine, dtype, cin, stride):
    """2 x 9 x 9, zero padding 1, stride 1 and 2, n = 128: 162 / 50 positions, every one next to a border."""
    _conv_case(engine, dtype, (2, 9, 9, cin, 3, 3, stride, 1, 1, 128, 1))


@pytest.mark.parametrize("dtype", ALL)
def test_dilated_fc6(engine, dtype):
    """dil_h 6 / pad_h 6 against dil_w 1 / pad_w 1, n = 256."""
    _conv_case(engine, dtype, CONVS[-1])


@pytest.mark.parametrize("dtype", [0, 2, 3, 6])
def test_grouped_launch(engine, dtype):
    """blockIdx.y times a 128-wide tile: two groups of 64 channels, 8 taps in time, zero padding 4, 128 outputs per group."""
    b, s, groups, cin, k, n = 2, 37, 2, 64, 8, 128
    g = torch.Generator().manual_seed(17)
    x = torch.randn(b, s, groups * cin, generator=g)
    w = torch.randn(groups * n, k * cin, generator=g) / (k * cin) ** 0.5      # [out][k][in / groups]
    bias = torch.randn(groups * n, generator=g)
    res = torch.randn(b, s, groups * n, generator=g)
    d = _desc(batch=b, in_h=s, in_w=1, out_h=s, out_w=1, cin=cin, kh=k, kw=1, pad_h=k // 2, x_stride_b=s * groups * cin,
              x_stride_h=groups * cin, x_stride_w=groups * cin, n=n, y_ld=groups * n, r_ld=groups * n, act=2, res_after_act=1, groups=groups)

    def ref_of(xd, _, wd, rd):
        v = F.conv1d(xd.permute(0, 2, 1), wd.reshape(groups * n, k, cin).permute(0, 2, 1), bias.double(), padding=k // 2,
                     groups=groups)[:, :, :s]
        return F.gelu(v).permute(0, 2, 1) + rd

    _both_widths(engine, d, dtype, x, w, None, bias, res, (b, s, groups * n), ref_of)


@pytest.mark.parametrize("dtype", [0, 1, 3, 5])
def test_dual_source(engine, dtype):
    """avcer_conv_gemm_dual at the shape of test_dual_source_fused_1x1: K = [T2 (64) | X at stride 2 (128)], n = 256."""
    b, h, p_, cin, n, st = 2, 14, 64, 128, 256, 2
    oh = (h - 1) // st + 1
    g = torch.Generator().manual_seed(21)
    x = torch.randn(b, h, h, cin, generator=g)
    t2 = torch.randn(b, oh, oh, p_, generator=g)
    w = torch.cat([torch.randn(n, p_, generator=g) / p_ ** 0.5, torch.randn(n, cin, generator=g) / cin ** 0.5], dim=1)
    bias = torch.randn(n, generator=g)
    d = _desc(batch=b, in_h=oh, in_w=oh, out_h=oh, out_w=oh, cin=p_, x_stride_b=oh * oh * p_, x_stride_h=oh * p_, x_stride_w=p_, n=n,
              y_ld=n, r_ld=n, act=1, x2_cin=cin, x2_stride=st, x2_stride_b=h * h * cin, x2_stride_h=h * cin, x2_stride_w=cin)

    def ref_of(td, xd, wd, _):
        return F.relu(td @ wd[:, :p_].t() + xd[:, ::st, ::st, :] @ wd[:, p_:].t() + bias.double())

    _both_widths(engine, d, dtype, t2, w, None, bias, None, (b, oh, oh, n), ref_of, x2=x)


@pytest.mark.parametrize("dtype", [0, 1, 5])
def test_sub_sampled_residual(engine, dtype):
    """r_sub = 2 at the shape of test_gpu_kernels.py's test of that name: 3 x 7 x 7 outputs add rows (2 oy, 2 ox) of a 13 x 13 grid."""
    b, h, k, n = 3, 13, 64, 256
    oh = (h + 1) // 2
    g = torch.Generator().manual_seed(31 + dtype)
    t2 = torch.randn(b, oh, oh, k, generator=g)
    x = torch.randn(b, h, h, n, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    scale, bias = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    d = _desc(batch=b, in_h=oh, in_w=oh, out_h=oh, out_w=oh, cin=k, x_stride_b=oh * oh * k, x_stride_h=oh * k, x_stride_w=k, n=n, y_ld=n,
              r_ld=n, act=1, r_sub=2, r_h=h, r_w=h)

    def ref_of(td, _, wd, rd):
        return F.relu(td @ wd.t() * scale.double() + bias.double() + rd[:, ::2, ::2])

    _both_widths(engine, d, dtype, t2, w, scale, bias, x, (b, oh, oh, n), ref_of)


# ----------------------------------------------------------------------------- B. the straddling gather
def _straddle_desc(cin, pitch, kh, kw, n, b=2, h=6, w_=7):
    oh, ow = h + 2 - (kh - 1), w_ + 2 - (kw - 1)
    return _desc(batch=b, in_h=h, in_w=w_, out_h=oh, out_w=ow, cin=cin, kh=kh, kw=kw, pad_h=1, pad_w=1, x_stride_b=h * w_ * pitch,
                 x_stride_h=w_ * pitch, x_stride_w=pitch, n=n, y_ld=n, r_ld=n, act=1), (b, h, w_, oh, ow)


# one wrap suffices: bk - vec - gcd(cin, bk) < cin with (bk, vec) = (32, 4) for f32 input, (64, 8) for bf16.  Four taps make K a
# whole number of K-steps for these cins; 28 (f32) and 56 (bf16), the cins closest to the bound (24 < 28, 48 < 56), need eight
_STRADDLE = ([(dt, c, kh, kw) for dt in (0, 3) for c in (16, 24, 48) for kh, kw in ((2, 2), (4, 1))] +
             [(dt, c, kh, kw) for dt in (1, 2) for c in (32, 48) for kh, kw in ((2, 2), (4, 1))] +
             [(0, 28, 2, 4), (3, 28, 2, 4), (1, 56, 2, 4), (2, 56, 2, 4)])


@pytest.mark.parametrize("dtype,cin,kh,kw", _STRADDLE)
def test_straddling_gather(engine, dtype, cin, kh, kw):
    """2 x 6 x 7 pixels of cin + 8 elements (the 8 behind the channels are NaN: nothing may read them), zero padding 1, four taps
    as 2 x 2 (a K-step crosses kx, and for cin 24 / 48 the kx wrap into the next ky) and 4 x 1 (every crossing is one into the next
    ky), eight as 2 x 4.  Against float64 F.conv2d at both tile widths, which also agree bit for bit."""
    n, pitch = 128, cin + 8
    d, (b, h, w_, oh, ow) = _straddle_desc(cin, pitch, kh, kw, n)
    g = torch.Generator().manual_seed(100 * dtype + cin + kh)
    x = torch.full((b, h, w_, pitch), NAN)
    x[..., :cin] = torch.randn(b, h, w_, cin, generator=g)
    w = torch.randn(n, kh * kw * cin, generator=g) / (kh * kw * cin) ** 0.5
    scale, bias = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    res = torch.randn(b, oh, ow, n, generator=g)
    ref, got = None, {}
    for tn in WIDTHS:
        d.tile_n = tn
        y, xd, wd, rd = _run(engine, d, dtype, x, w, scale, bias, res, torch.full((b, oh, ow, n), NAN))
        if ref is None:
            ref = F.conv2d(xd[..., :cin].permute(0, 3, 1, 2), wd.reshape(n, kh, kw, cin).permute(0, 3, 1, 2), None, 1, 1)
            ref = F.relu(ref.permute(0, 2, 3, 1) * scale.double() + bias.double() + rd)
        err = (y.double() - ref).abs().max().item()
        print(f"dtype {dtype} cin {cin} {kh}x{kw} tile_n {tn}: max|err| {err:.3e} (tol {_tol(dtype, ref):.3e})")
        assert err < _tol(dtype, ref), (tn, err)
        got[tn] = y
    assert torch.equal(got[64], got[128])


# two wraps would be needed: bk - vec - gcd(cin, bk) >= cin; taps chosen so that K is a whole number of K-steps
_REFUSED = [(0, 4, 2, 4), (0, 8, 2, 2), (3, 8, 2, 2), (0, 12, 2, 4), (0, 20, 2, 4), (3, 20, 2, 4),
            (1, 8, 2, 4), (1, 16, 2, 2), (2, 16, 2, 2), (1, 24, 2, 4), (1, 40, 2, 4), (2, 40, 2, 4)]


@pytest.mark.parametrize("dtype,cin,kh,kw", _REFUSED)
def test_cin_that_needs_two_wraps_is_refused(engine, dtype, cin, kh, kw):
    """AVCER_EINVAL naming cin and the K-step, and not one byte of the output written."""
    n = 128
    bk = 64 if A_KIND[dtype] == "bf16" else 32
    assert (kh * kw * cin) % bk == 0
    d, (b, h, w_, oh, ow) = _straddle_desc(cin, cin, kh, kw, n)
    dev = engine.device
    g = torch.Generator().manual_seed(cin)
    xd = _enc(torch.randn(b, h, w_, cin, generator=g), A_KIND[dtype], dev)
    wd = (torch.randn(n, kh * kw * cin, generator=g) / 8).to(dev, xd.dtype)
    w_arg = engine.split_weight_rows(wd) if dtype >= 3 else wd
    y0 = torch.randn(b, oh, ow, n, generator=g)
    yd = _enc(y0, O_KIND[dtype], dev)
    before = yd.cpu().clone()
    for tn in (0,) + WIDTHS:
        d.tile_n = tn
        with pytest.raises(AvcerError, match=rf"cin={cin} .*K-step of {bk} ") as e:
            engine.conv_gemm(d, dtype, xd, w_arg, None, None, None, yd)
        assert e.value.code == -1                                 # AVCER_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(_bits(yd.cpu()), _bits(before))
