"""Does every kernel-level entry write ONLY its output, and ALL of it?  Each case hands the entry an output that lives between two
guard bands (tests/guard_band.py: at least 256 output rows on either side), runs it on two different fill patterns and once more
into an exactly sized tensor, and requires: guards and gap elements (the columns outside [y_coff, y_coff + n) of a strided output,
the rows of other levels in a shared tensor) untouched, every output element written, the same bits in all three runs, the inputs
unchanged.  The VALUES are the business of the parity tests (test_gpu_kernels.py, test_gpu_gemm_wd.py, test_gpu_bneck_tail.py, ...);
here they are only required to be finite where that is cheap to ask.  Shapes are the smallest at which the tile logic still has a
ragged edge; where an Engine wrapper allocates the output itself, the C entry is called directly so that the guarded buffer is
used.  No entry had to be narrowed: every strided form asked for is accepted as it is."""
import pytest
import torch

from avcer_amd._lib import SPLIT_TRAILER
from avcer_amd.engine import _ptr
from avcer_amd.sp32 import from_sp32, to_sp32
from guard_band import Band, check, columns
from test_gpu_kernels import A_KIND, O_KIND, _desc, _enc

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "sp32": torch.int16}
PAD, COFF = 64, 32          # the strided form: y_ld = n + 64, y_coff = 32 (and the residual likewise)


def _call(engine, name, *args):
    engine._check(getattr(engine.lib, name)(engine.ctx, *args, engine._stream()))


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 12345)


def _sp(g, *shape, dev):
    return to_sp32(torch.rand(*shape, generator=g) * 2).to(dev)


# ----------------------------------------------------------------------------- avcer_conv_gemm / avcer_conv_gemm_dual
def _conv_bounds(engine, d, dtype, x, w, strided, x2=None):
    """d: the case's descriptor without its output / residual strides; x (and x2) f32 in the input's layout, w f32 [groups * n][K].
    Always with scale, bias and a residual of the output's storage kind."""
    dev = engine.device
    ak, ok = A_KIND[dtype], O_KIND[dtype]
    ntot = d.n * max(1, d.groups)
    m = d.batch * d.out_h * d.out_w
    ld, off = (ntot + PAD, COFF) if strided else (ntot, 0)
    d.y_ld, d.y_coff, d.r_ld, d.r_coff = ld, off, ld, off
    g = _gen(dtype, m, ntot, strided)
    xd = _enc(x, ak, dev)
    x2d = None if x2 is None else _enc(x2, ak, dev)
    wd = w.to(dev, torch.bfloat16 if ak == "bf16" else torch.float32).contiguous()
    w_arg = wd if dtype < 3 else (engine.weight_frags(wd) if dtype >= 7 else engine.split_weight_rows(wd))
    scale, bias = (torch.rand(ntot, generator=g) + 0.5).to(dev), torch.randn(ntot, generator=g).to(dev)
    r_rows = m if d.r_sub <= 1 else d.batch * d.r_h * d.r_w
    rd = _enc(torch.randn(r_rows, ld, generator=g), ok, dev)
    mul = 2 if ok == "sp32" else 1          # an sp32 element is two int16
    band = Band("y", (m, mul * ld), TORCH[ok], written=columns(mul * ld, mul * off, mul * ntot))
    inputs = [xd, w_arg, scale, bias, rd] + ([] if x2d is None else [x2d])

    def run(outs):
        if x2d is None:
            engine.conv_gemm(d, dtype, xd, w_arg, scale, bias, rd, outs[0])
        else:
            engine.conv_gemm_dual(d, dtype, xd, x2d, w_arg, scale, bias, rd, outs[0])

    y, = check(run, [band], inputs, device=dev)
    y = y[:, mul * off:mul * (off + ntot)]
    got = from_sp32(y) if ok == "sp32" else y.float()
    assert torch.isfinite(got).all() and got.abs().max() > 0.1


def _linear(m, k, n, **kw):
    return _desc(batch=m, cin=k, x_stride_b=k, x_stride_h=k, x_stride_w=k, n=n, act=1, **kw)


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype,tile_m,tile_n", [(t, 0, 0) for t in range(7)] + [(7, 112, 0), (7, 128, 0), (8, 112, 0), (8, 128, 0)] +
                         [(t, 0, 128) for t in range(7)],
                         ids=[f"{t}-0" for t in range(7)] + ["7-112", "7-128", "8-112", "8-128"] + [f"{t}-0-n128" for t in range(7)])
def test_conv_gemm_linear(engine, dtype, tile_m, tile_n, strided):
    """M = 129: one row past a 128-row tile (dtypes 7 / 8: 17 past a 112-row one).  K = 64, N = 256.  tile_n = 0 is the library's
    choice, 64-wide tiles at this K; n128 forces conv_gemm_kernel<.., 128> of dtypes 0-6 (two column tiles, LDS-staged drain of
    128 columns in the f32 / bf16 modes)."""
    m, k, n = 129, 64, 256
    g = _gen(m, k, n)
    _conv_bounds(engine, _linear(m, k, n, tile_m=tile_m, tile_n=tile_n), dtype, torch.randn(m, k, generator=g),
                 torch.randn(n, k, generator=g) / k ** 0.5, strided)


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("tile_m", [16, 32, 64])
@pytest.mark.parametrize("m", [1, 17, 49])
@pytest.mark.parametrize("dtype", [9, 10])
def test_conv_gemm_skinny(engine, dtype, m, tile_m, strided):
    """The one-wave-per-tile form: 1, 17 and 49 positions against wave tiles of 16, 32 and 64.  K = 128, N = 64."""
    k, n = 128, 64
    g = _gen(m, k, n)
    _conv_bounds(engine, _linear(m, k, n, tile_m=tile_m), dtype, torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5,
                 strided)


@pytest.mark.parametrize("dtype", [5, 9])
def test_conv_gemm_grouped(engine, dtype):
    """One launch of four groups of 64 channels (the pos-conv's kind: taps in time, zero padding, GELU then residual) into rows
    of 256 + 64 elements: the 32 elements in front of the groups and the 32 behind them are gaps."""
    b, s, groups, cin, k = 2, 37, 4, 64, 4
    ctot = groups * cin
    g = _gen(b, s, k)
    d = _desc(batch=b, in_h=s, in_w=1, out_h=s, out_w=1, cin=cin, kh=k, kw=1, pad_h=k // 2, x_stride_b=s * ctot, x_stride_h=ctot,
              x_stride_w=ctot, n=64, act=2, res_after_act=1, groups=groups)
    _conv_bounds(engine, d, dtype, torch.randn(b, s, ctot, generator=g), torch.randn(ctot, k * cin, generator=g) / (k * cin) ** 0.5, True)


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", [5, 7, 9])
def test_conv_gemm_padded_3x3(engine, dtype, strided):
    """2 x 9 x 9 x 64 -> 256: every position next to a border, 162 positions."""
    b, h, c, n = 2, 9, 64, 256
    g = _gen(b, h, c, n)
    d = _desc(batch=b, in_h=h, in_w=h, out_h=h, out_w=h, cin=c, kh=3, kw=3, pad_h=1, pad_w=1, x_stride_b=h * h * c, x_stride_h=h * c,
              x_stride_w=c, n=n, act=1)
    _conv_bounds(engine, d, dtype, torch.randn(b, h, h, c, generator=g), torch.randn(n, 9 * c, generator=g) / (9 * c) ** 0.5, strided)


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", [5, 9])
def test_conv_gemm_sub_sampled_residual(engine, dtype, strided):
    """r_sub = 2: 3 x 7 x 7 outputs add the rows (2 oy, 2 ox) of a 3 x 13 x 13 residual."""
    b, h, k, n = 3, 13, 64, 256
    oh = (h + 1) // 2
    g = _gen(b, h, k, n)
    d = _desc(batch=b, in_h=oh, in_w=oh, out_h=oh, out_w=oh, cin=k, x_stride_b=oh * oh * k, x_stride_h=oh * k, x_stride_w=k, n=n, act=1,
              r_sub=2, r_h=h, r_w=h)
    _conv_bounds(engine, d, dtype, torch.randn(b, oh, oh, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5, strided)


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", [5, 7])
def test_conv_gemm_dual(engine, dtype, strided):
    """conv3 + downsample of a stage's first block as one contraction, 3 x 7 x 7 outputs: K = [T2 (64) | X at stride 2 (128)]."""
    b, oh, p_, cin, n = 3, 7, 64, 128, 256
    h = 2 * oh
    g = _gen(b, oh, p_, cin)
    d = _desc(batch=b, in_h=oh, in_w=oh, out_h=oh, out_w=oh, cin=p_, x_stride_b=oh * oh * p_, x_stride_h=oh * p_, x_stride_w=p_, n=n, act=1,
              x2_cin=cin, x2_stride=2, x2_stride_b=h * h * cin, x2_stride_h=h * cin, x2_stride_w=cin)
    _conv_bounds(engine, d, dtype, torch.randn(b, oh, oh, p_, generator=g), torch.randn(n, p_ + cin, generator=g) / (p_ + cin) ** 0.5, strided,
                 x2=torch.randn(b, h, h, cin, generator=g))


# ----------------------------------------------------------------------------- fused kernels (csrc/fused.hip)
_CHAINS = {
    "p64-next": dict(planes=64, nb=2, hw=9, nxt=True),
    "p64-out_step2": dict(planes=64, nb=2, hw=9, nxt=False, out_step=2),       # compact 5 x 5 output of an odd grid
    "p64-downsample": dict(planes=64, nb=2, hw=9, nxt=True, ds=True),
    "p64-spatial-tile": dict(planes=64, nb=1, hw=55, nxt=True, frags=True),
    "p128-next": dict(planes=128, nb=1, hw=7, nxt=True),
}


@pytest.mark.parametrize("form", list(_CHAINS))
def test_bneck_chain(engine, form):
    """avcer_bneck_chain: `out` and, where the form has one, `t1n`.  162 and 49 positions against 128-position blocks, 50 compact
    positions of the strided form, and the 11 x 11 tiles of the spatial-tile form with their seven idle rows each."""
    c = dict(out_step=1, ds=False, frags=False)
    c.update(_CHAINS[form])
    planes, nb, hw, nxt = c["planes"], c["nb"], c["hw"], c["nxt"]
    dev = engine.device
    g = _gen(planes, nb, hw, c["out_step"], c["ds"])
    p4 = 4 * planes
    t1, x = _sp(g, nb, hw, hw, planes, dev=dev), _sp(g, nb, hw, hw, 64 if c["ds"] else p4, dev=dev)
    w2m = (torch.randn(planes, 9 * planes, generator=g) / (3 * planes ** 0.5)).to(dev)
    w2, w2f = engine.split_weight_rows(w2m), (engine.weight_frags(w2m) if c["frags"] else None)
    w3 = engine.split_weight_rows(torch.randn(p4, planes + (64 if c["ds"] else 0), generator=g) / planes ** 0.5)
    w1 = engine.split_weight_rows(torch.randn(planes, p4, generator=g) / p4 ** 0.5) if nxt else None
    b2, b3 = ((torch.randn(n, generator=g) * 0.3).to(dev) for n in (planes, p4))
    b1 = (torch.randn(planes, generator=g) * 0.3).to(dev) if nxt else None
    oh = (hw - 1) // c["out_step"] + 1
    bands = [Band("out", (nb * oh * oh, 2 * p4), torch.int16)] + ([Band("t1n", (nb * hw * hw, 2 * planes), torch.int16)] if nxt else [])

    def run(outs):
        engine.bneck_chain(planes, nb, hw, hw, t1, x, outs[0], outs[1] if nxt else None, w2, b2, w3, b3, w1, b1,
                           ds_cin=64 if c["ds"] else 0, out_step=c["out_step"], w2_frags=w2f)

    got = check(run, bands, [t for t in (t1, x, w2, w2f, w3, w1, b2, b3, b1) if t is not None], device=dev)
    assert all(torch.isfinite(from_sp32(t)).all() for t in got)


@pytest.mark.parametrize("m", [1, 129, 300])
def test_bneck_tail(engine, m):
    """avcer_bneck_tail: `out` is stored through a buffer descriptor whose byte count is the launcher's (rows past M rely on it
    alone), `t1n` behind a row test.  One position, one past a 128-position block, two blocks and 44 rows."""
    dev = engine.device
    g = _gen(m, 256)
    t2, x = _sp(g, m, 256, dev=dev), _sp(g, m, 1024, dev=dev)
    w3 = engine.split_weight_rows(torch.randn(1024, 256, generator=g) / 16)
    w1n = engine.split_weight_rows(torch.randn(256, 1024, generator=g) / 32)
    b3, b1n = (torch.randn(1024, generator=g) * 0.3).to(dev), (torch.randn(256, generator=g) * 0.3).to(dev)

    def run(outs):
        engine.bneck_tail(256, m, t2, x, outs[0], outs[1], w3, b3, w1n, b1n)

    got = check(run, [Band("out", (m, 2048), torch.int16), Band("t1n", (m, 512), torch.int16)], [t2, x, w3, w1n, b3, b1n], device=dev)
    assert all(torch.isfinite(from_sp32(t)).all() for t in got)


def test_stem_pool(engine):
    """avcer_stem_pool at one frame: 55 x 55 x 64 sp32 from the planar fp16 hi / lo image."""
    dev = engine.device
    g = _gen(230)
    img = torch.zeros(1, 230, 230, 4)
    img[:, 2:226, 2:226, :3] = torch.randn(1, 224, 224, 3, generator=g) * 60.0
    hi = img.to(torch.float16)
    lo = (img - hi.float()).to(torch.float16)
    planes = torch.stack([hi.view(torch.int16), lo.view(torch.int16)]).to(dev)
    w = engine.split_weight_rows(torch.randn(64, 224, generator=g) / 147 ** 0.5)
    scale, bias = (torch.rand(64, generator=g) + 0.5).to(dev), (torch.randn(64, generator=g) * 0.2).to(dev)

    def run(outs):
        _call(engine, "avcer_stem_pool", _ptr(planes), 230 * 230 * 4 * 2, _ptr(w), _ptr(scale), _ptr(bias), _ptr(outs[0]), 1)

    got, = check(run, [Band("y", (55 * 55, 128), torch.int16)], [planes, w, scale, bias], device=dev)
    assert torch.isfinite(from_sp32(got)).all()


def test_stem_pool_u8(engine):
    """avcer_stem_pool_u8 at one u8 frame of 150 x 131 (the NEAREST resize happens inside)."""
    dev = engine.device
    g = _gen(150, 131)
    frames = torch.randint(0, 256, (1, 150, 131, 3), generator=g, dtype=torch.uint8).to(dev)
    w = engine.split_weight_rows(torch.randn(64, 224, generator=g) / 147 ** 0.5)
    scale, shifts = (torch.rand(64, generator=g) + 0.5).to(dev), (torch.randn(9, 64, generator=g) * 0.2).to(dev)

    def run(outs):
        _call(engine, "avcer_stem_pool_u8", _ptr(frames), 1, 150, 131, _ptr(w), _ptr(scale), _ptr(shifts), _ptr(outs[0]))

    got, = check(run, [Band("y", (55 * 55, 128), torch.int16)], [frames, w, scale, shifts], device=dev)
    assert torch.isfinite(from_sp32(got)).all()


# ----------------------------------------------------------------------------- attention, GRU
@pytest.mark.parametrize("kinds", [(0, 0), (1, 1), (0, 2)], ids=["f32", "bf16", "x3"])
@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("entry,s", [("avcer_attention", 1), ("avcer_attention", 99), ("avcer_attention", 129),
                                     ("avcer_attention_long", 129), ("avcer_attention_long", 257)])
def test_attention(engine, entry, s, d, kinds):
    """Two row blocks of two heads: a ragged last query block and key tile in both the whole-head and the streamed kernels."""
    n, heads = 2, 2
    e = heads * d
    in_kind, out_kind = kinds
    dev = engine.device
    qkv = torch.randn(n, s, 3 * e, generator=_gen(s, d)).to(dev, torch.bfloat16 if in_kind == 1 else torch.float32)
    band = Band("out", (n * s, 2 * e if out_kind == 2 else e), {0: torch.float32, 1: torch.bfloat16, 2: torch.int16}[out_kind])

    def run(outs):
        _call(engine, entry, _ptr(qkv), _ptr(outs[0]), n, s, heads, d, d ** -0.5, in_kind, out_kind)

    got, = check(run, [band], [qkv], device=dev)
    assert torch.isfinite(from_sp32(got) if out_kind == 2 else got.float()).all()


@pytest.mark.parametrize("mode", [0, 2], ids=["f32", "x3"])
def test_gru_layer(engine, mode):
    """avcer_gru_layer at three windows of five steps (one block holds 16 windows: 13 idle)."""
    n, s = 3, 5
    dev = engine.device
    g = _gen(n, s, mode)
    xp = (torch.randn(n, s, 768, generator=g) * 0.6).to(dev)
    w, b = ((torch.rand(768, 256, generator=g) - 0.5) / 8).to(dev), ((torch.rand(768, generator=g) - 0.5) / 8).to(dev)

    def run(outs):
        _call(engine, "avcer_gru_layer", _ptr(xp), _ptr(w), _ptr(b), n, s, 256, mode, _ptr(outs[0]))

    got, = check(run, [Band("h_seq", (n * s, 256), torch.float32)], [xp, w, b], device=dev)
    assert torch.isfinite(got).all() and got.abs().max() <= 1.0


# ----------------------------------------------------------------------------- the detectors' kernels
@pytest.mark.parametrize("mode", [0, 2], ids=["f32", "x3"])
@pytest.mark.parametrize("cin,cout,stride", [(8, 16, 1), (16, 32, 2)])
def test_dwsep(engine, cin, cout, stride, mode):
    """One conv_dw block on 2 x 5 x 7: a single ragged 8 x 8 tile per frame; stride 2 gives 3 x 4 outputs."""
    nb, h, w = 2, 5, 7
    dev = engine.device
    g = _gen(cin, cout, stride)
    x = torch.randn(nb, h, w, cin, generator=g).to(dev)
    dw_w, dw_s, dw_b = (torch.randn(*sh, generator=g).to(dev) for sh in ((9, cin), (cin,), (cin,)))
    pad = torch.zeros((cout + 63) // 64 * 64, (cin + 31) // 32 * 32)
    pad[:cout, :cin] = torch.randn(cout, cin, generator=g) / cin ** 0.5
    pw = engine.split_weight_rows(pad) if mode == 2 else pad.to(dev)
    pw_s, pw_b = (torch.randn(cout, generator=g).to(dev) for _ in range(2))
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1

    def run(outs):
        _call(engine, "avcer_dwsep", cin, cout, stride, mode, nb, h, w, _ptr(x), _ptr(dw_w), _ptr(dw_s), _ptr(dw_b), _ptr(pw), _ptr(pw_s),
              _ptr(pw_b), _ptr(outs[0]))

    got, = check(run, [Band("y", (nb * oh * ow, cout), torch.float32)], [x, dw_w, dw_s, dw_b, pw, pw_s, pw_b], device=dev)
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("kind", [0, 2], ids=["f32", "sp32"])
def test_s3fd_stem(engine, kind):
    dev = engine.device
    g = _gen(5, 7, kind)
    frames = torch.randint(0, 256, (1, 5, 7, 3), generator=g, dtype=torch.uint8).to(dev)
    wt, bias = (torch.randn(27, 64, generator=g) / 27 ** 0.5).to(dev), torch.randn(64, generator=g).to(dev)

    def run(outs):
        _call(engine, "avcer_s3fd_stem", _ptr(frames), 1, 5, 7, 0, _ptr(wt), _ptr(bias), _ptr(outs[0]), kind)

    band = Band("y", (35, 128), torch.int16) if kind == 2 else Band("y", (35, 64), torch.float32)
    got, = check(run, [band], [frames, wt, bias], device=dev)
    assert torch.isfinite(from_sp32(got) if kind == 2 else got).all()


@pytest.mark.parametrize("kind", [0, 2], ids=["f32", "sp32"])
@pytest.mark.parametrize("ceil_mode", [0, 1], ids=["floor", "ceil"])
def test_maxpool2(engine, ceil_mode, kind):
    """1 x 5 x 7 x 32: both extents odd, so the floor form drops a row and a column and the ceil form pools over the edge."""
    h, w, c = 5, 7, 32
    dev = engine.device
    x = torch.randn(1, h, w, c, generator=_gen(h, w, kind))
    xd = to_sp32(x).to(dev) if kind == 2 else x.to(dev)
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if ceil_mode else (h // 2, w // 2)

    def run(outs):
        _call(engine, "avcer_maxpool2", _ptr(xd), _ptr(outs[0]), 1, h, w, c, ceil_mode, kind)

    band = Band("y", (oh * ow, 2 * c), torch.int16) if kind == 2 else Band("y", (oh * ow, c), torch.float32)
    got, = check(run, [band], [xd], device=dev)
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=bool(ceil_mode)).permute(0, 2, 3, 1).reshape(oh * ow, c)
    assert torch.equal(from_sp32(got), from_sp32(to_sp32(ref))) if kind == 2 else torch.equal(got, ref)


@pytest.mark.parametrize("kind,n_out,l2norm", [(0, 8, True), (2, 8, True), (0, 6, False), (2, 6, False)])
def test_s3fd_head(engine, kind, n_out, l2norm):
    """One level of 3 x 5 positions inside loc / conf tensors of 40 priors per frame, from row 7 on, two frames: rows 0-6 and
    22-39 of either frame belong to other levels and are gaps.  The inverse-norm scratch of the normalised levels is guarded too."""
    nb, h, w, c, row0, priors = 2, 3, 5, 256, 7, 40
    dev = engine.device
    g = _gen(kind, n_out)
    x = torch.randn(nb, h, w, c, generator=g)
    xd = to_sp32(x).to(dev) if kind == 2 else x.to(dev)
    wt, bias = (torch.randn(9, c, n_out, generator=g) / (9 * c) ** 0.5).to(dev), torch.randn(n_out, generator=g).to(dev)
    rows = torch.zeros(priors, 1, dtype=torch.bool)
    rows[row0:row0 + h * w] = True
    bands = [Band("loc", (nb, priors, 4), torch.float32, written=rows), Band("conf", (nb, priors, 2), torch.float32, written=rows)]
    if l2norm:
        bands.append(Band("inv_norm", (nb * h * w,), torch.float32))

    def run(outs):
        _call(engine, "avcer_s3fd_head", _ptr(xd), kind, _ptr(outs[2]) if l2norm else None, _ptr(wt), _ptr(bias), nb, h, w, c, n_out, row0,
              priors, _ptr(outs[0]), _ptr(outs[1]))

    loc, conf = check(run, bands, [xd, wt, bias], device=dev)[:2]
    assert torch.isfinite(loc[:, row0:row0 + h * w]).all()
    assert (conf[:, row0:row0 + h * w].sum(-1) - 1).abs().max() < 1e-5        # softmaxed pairs


# ----------------------------------------------------------------------------- splits and copies
@pytest.mark.parametrize("numel", [32, 96])
def test_split_weights(engine, numel):
    dev = engine.device
    w = torch.randn(numel, generator=_gen(numel)).to(dev)

    def run(outs):
        _call(engine, "avcer_split_weights", _ptr(w), _ptr(outs[0]), numel)

    got, = check(run, [Band("out", (numel // 32, 64), torch.int16)], [w], device=dev)
    assert torch.equal(got, to_sp32(w.cpu().reshape(-1, 32)))


@pytest.mark.parametrize("n,k", [(32, 32), (64, 96)])
def test_split_weight_rows_and_weight_frags(engine, n, k):
    """Both write n * k * 4 bytes and the trailer of AVCER_SPLIT_TRAILER bytes behind them: the payload is exactly that, every byte of
    the trailer included."""
    dev = engine.device
    w = (torch.randn(n, k, generator=_gen(n, k)) * 0.03).to(dev)
    band = Band("out", (n * k * 2 + SPLIT_TRAILER // 2,), torch.int16, row_bytes=k * 4)
    assert band.nbytes == n * k * 4 + SPLIT_TRAILER

    def run_rows(outs):
        _call(engine, "avcer_split_weight_rows", _ptr(w), _ptr(outs[0]), n, k)

    rows, = check(run_rows, [band], [w], device=dev)
    assert torch.equal(rows, engine.split_weight_rows(w).cpu())
    rows_d = rows.to(dev)

    def run_frags(outs):
        _call(engine, "avcer_weight_frags", _ptr(rows_d), _ptr(outs[0]), n, k)

    frags, = check(run_frags, [band], [rows_d], device=dev)
    assert torch.equal(frags[n * k * 2:], rows[n * k * 2:])                  # the same trailer
    assert torch.equal(frags[:n * k * 2].sort().values, rows[:n * k * 2].sort().values)   # a permutation of the same halves


def test_gather_windows(engine):
    dev = engine.device
    g = _gen(512)
    feats = torch.randn(7, 512, generator=g).to(dev)
    idx = torch.tensor([[0] * 10, list(range(-3, 7)), [6] * 5 + [2] * 5], dtype=torch.int32).clamp_(min=0).to(dev)

    def run(outs):
        _call(engine, "avcer_gather_windows", _ptr(feats), _ptr(idx), 3, _ptr(outs[0]))

    got, = check(run, [Band("out", (3 * 10, 512), torch.float32)], [feats, idx], device=dev)
    assert torch.equal(got, torch.relu(feats.cpu()[idx.cpu().long().reshape(-1)]))


def test_crop_tiles(engine):
    """Three rects: a whole frame resized, a 1 x 1 crop replicated, an empty one (a zero tile, but a WRITTEN one)."""
    dev = engine.device
    frames = torch.randint(0, 256, (2, 40, 50, 3), generator=_gen(40, 50), dtype=torch.uint8).to(dev)
    rects = torch.tensor([[0, 0, 0, 50, 40], [1, 5, 7, 6, 8], [0, 10, 10, 10, 20]], dtype=torch.int32).to(dev)

    def run(outs):
        _call(engine, "avcer_crop_tiles", _ptr(frames), 2, 40, 50, _ptr(rects), 3, 0, _ptr(outs[0]))

    got, = check(run, [Band("tiles", (3 * 224, 224 * 3), torch.uint8)], [frames, rects], device=dev)
    got = got.reshape(3, 224, 224, 3)
    assert (got[1] == frames[1, 7, 5].cpu()).all() and not got[2].any() and got[0].any()
