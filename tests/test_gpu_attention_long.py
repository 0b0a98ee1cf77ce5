"""avcer_attention_long (csrc/attention.hip) against float64: softmax(Q K^T * scale) V with key tiles of KT = 128 keys streamed
through LDS and a running softmax per query row, one workgroup per (window, head, block of QB = 128 queries), in the three
arithmetic forms: exact f32 on the VALU, bf16 MFMA, x3 MFMA (f32 in, sp32 out).

Bounds.  Up to 256 tokens: the measure and the figures of test_gpu_kernels.test_attention_f32_and_x3_against_float64 (rel rms
< 1e-6, max|err| < 4e-6) and of test_attention_bf16_against_float64 (what the bf16 storage allows).  Past 256 tokens nobody had
measured, so the reference's own arithmetic is measured beside the kernel: torch float32 eager softmax(Q K^T s) V on the CPU
against float64 on the same inputs, and the bound is max(the figure above, 2 x that error) -- the factor 2 because the order of
summation differs within one precision class; the bf16 form by the same rule against torch bfloat16 eager.

Measured on the MI355X (d = 64, n = 2; rel rms / max|err| against float64; the test prints every figure before it asserts):
  keys    f32 form           x3 form            torch float32 eager (its double is the bound past 256 keys)
  256     3.6e-7 / 1.6e-6    4.1e-7 / 1.4e-6    -
  257     3.7e-7 / 1.9e-6    4.0e-7 / 1.1e-6    5.6e-7 rel rms
  1000    4.2e-7 / 1.7e-6    5.5e-7 / 1.9e-6    7.1e-7 / 2.3e-6
  5000    5.1e-7 / 1.9e-6    8.6e-7 / 3.6e-6    8.8e-7 / 2.3e-6 (n = 1) .. 3.6e-6 (n = 2)
  bf16 form: max|err| 7e-3 at every length, bound 4e-2 .. 5e-2.  Score ramp (early tiles underflow): 2.0e-5 / 1.4e-4 (f32) and
  2.3e-5 / 1.8e-4 (x3) against torch's own 3.7e-5 / 2.3e-4: scores up to 270 lose absolute precision in every float32 form.
"""
import functools

import pytest
import torch

from avcer_amd.sp32 import from_sp32

pytestmark = pytest.mark.gpu

KT, QB = 128, 128  # AVCER_ATT_LONG_KT, AVCER_ATT_LONG_QB (include/avcer_hip.h)
HEADS = 2
SIZES = sorted({1, 16, 255, 256, 257, KT - 1, KT, KT + 1, 2 * KT + 17, QB + 1, 1000, 5000})


def _eager(qkv, n, s, d, scale, dtype):
    """softmax(Q K^T * scale) V per head in `dtype` on the CPU, [n, s, HEADS * d]; one (window, head) at a time: 5000 x 5000 scores"""
    e = HEADS * d
    out = torch.empty(n, s, e, dtype=dtype)
    x = qkv.to(dtype)
    for b in range(n):
        for h in range(HEADS):
            q, k, v = (x[b, :, i * e + h * d:i * e + (h + 1) * d] for i in range(3))
            out[b, :, h * d:(h + 1) * d] = torch.softmax(q @ k.T * scale, -1) @ v
    return out


def _measure(got, ref):
    err = got.double() - ref
    return (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item(), err.abs().max().item()


def _reference(qkv, n, s, d):
    """What every form is held to on this input: float64 of the inputs and of their bf16 rounding, and the bounds"""
    scale = 1.0 / d ** 0.5
    ref = _eager(qkv, n, s, d, scale, torch.float64)
    qb = qkv.to(torch.bfloat16)
    refb = _eager(qb.double(), n, s, d, scale, torch.float64)
    rel_bound, max_bound = 1e-6, 4e-6
    bf_bound = (refb - ref).abs().max().item() + 2.0 ** -7 * refb.abs().max().item()
    if s > 256:
        t_rel, t_max = _measure(_eager(qkv, n, s, d, scale, torch.float32), ref)
        rel_bound, max_bound = max(rel_bound, 2 * t_rel), max(max_bound, 2 * t_max)
        tb_max = _measure(_eager(qb, n, s, d, scale, torch.bfloat16), refb)[1]
        bf_bound = max(bf_bound, 2 * tb_max)
        print(f"torch eager s={s} d={d} n={n}: fp32 rel rms {t_rel:.2e} max|err| {t_max:.2e}; bf16 max|err| {tb_max:.2e}")
    return dict(scale=scale, ref=ref, qb=qb, refb=refb, rel_bound=rel_bound, max_bound=max_bound, bf_bound=bf_bound)


@functools.lru_cache(maxsize=None)
def _random_case(s, d, n):
    g = torch.Generator().manual_seed(7 * s + d + n)
    qkv = torch.randn(n, s, 3 * HEADS * d, generator=g)
    qkv[..., :HEADS * d] *= 2.0                                      # scores up to ~ +-10
    return qkv, _reference(qkv, n, s, d)


def _run(engine, qkv, n, s, d, scale):
    """The three forms on the GPU: (f32 out, x3 out, bf16 out) on the host"""
    dev, e = engine.device, HEADS * d
    qd = qkv.to(dev)
    o32 = torch.full((n, s, e), float("nan"), device=dev)
    engine.attention_long(qd, o32, n, s, HEADS, d, scale, 0, 0)
    osp = torch.full((n, s, 2 * e), 0x7e00, dtype=torch.int16, device=dev)
    engine.attention_long(qd, osp, n, s, HEADS, d, scale, 0, 2)
    obf = torch.full((n, s, e), float("nan"), dtype=torch.bfloat16, device=dev)
    engine.attention_long(qkv.to(torch.bfloat16).to(dev), obf, n, s, HEADS, d, scale, 1, 1)
    torch.cuda.synchronize()
    return o32.cpu(), from_sp32(osp.cpu()), obf.cpu()


def _check(engine, qkv, r, n, s, d, tag):
    o32, ox3, obf = _run(engine, qkv, n, s, d, r["scale"])
    figures = {"f32": _measure(o32, r["ref"]), "x3": _measure(ox3, r["ref"]), "bf16": _measure(obf, r["refb"])}
    print(f"attention_long {tag} s={s} d={d} n={n}: " + ", ".join(f"{k} rel rms {a:.2e} max|err| {b:.2e}" for k, (a, b) in figures.items())
          + f" (bounds {r['rel_bound']:.2e} / {r['max_bound']:.2e}; bf16 max|err| {r['bf_bound']:.2e})")
    for name in ("f32", "x3"):
        rel, worst = figures[name]
        assert rel < r["rel_bound"] and worst < r["max_bound"], (name, s, d, n, rel, worst)
    assert torch.isfinite(obf.float()).all()
    assert figures["bf16"][1] < r["bf_bound"], ("bf16", s, d, n, figures["bf16"])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("s", SIZES)
def test_three_forms_against_float64(engine, s, d, n):
    qkv, r = _random_case(s, d, n)
    _check(engine, qkv, r, n, s, d, "random")


# ---- adversarial rows, at 2 KT + 17 keys (two full key tiles and a masked tail) and at QB + 1 queries' worth of blocks
S_ADV = 2 * KT + 17


def _base(d, seed, q_gain=0.5):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(2, S_ADV, 3 * HEADS * d, generator=g)
    qkv[..., :HEADS * d] *= q_gain
    return qkv


def _parts(qkv, d):
    e = HEADS * d
    n, s, _ = qkv.shape
    return tuple(qkv[..., i * e:(i + 1) * e].view(n, s, HEADS, d) for i in range(3))


@pytest.mark.parametrize("d", [64, 32])
def test_row_maximum_only_in_the_last_key_tile(engine, d):
    """Every query's largest score is against the LAST key (tail tile), every earlier score at least 80 below it: two tiles'
    sums are rescaled by exp(-80) or less when the third arrives."""
    qkv = _base(d, 11)
    q, k, _ = _parts(qkv, d)
    q[..., 0] = 16.0
    k[..., 0] = 0.0
    k[:, -1] = 0.0
    k[:, -1, :, 0] = 6.0 * d ** 0.5                                # score 96 against the last key; the others are O(1)
    scores = torch.einsum("nqhd,nkhd->nhqk", q.double(), k.double()) / d ** 0.5
    top = scores.topk(2, -1).values
    assert (scores.argmax(-1) == S_ADV - 1).all() and (top[..., 0] - top[..., 1]).min() > 80
    _check(engine, qkv, _reference(qkv, 2, S_ADV, d), 2, S_ADV, d, "last-key peak")


@pytest.mark.parametrize("d", [64, 32])
def test_all_keys_equal(engine, d):
    qkv = _base(d, 12, 2.0)
    _, k, _ = _parts(qkv, d)
    k[:] = k[:, :1]
    _check(engine, qkv, _reference(qkv, 2, S_ADV, d), 2, S_ADV, d, "equal keys")


@pytest.mark.parametrize("d", [64, 32])
def test_early_tiles_underflow(engine, d):
    """Scores grow by 1 per key: against the last tile's maximum the first tile's weights are below exp(-140), 0 in float32."""
    qkv = _base(d, 13)
    q, k, _ = _parts(qkv, d)
    q[..., 0] = 8.0
    k[..., 0] = (torch.arange(S_ADV, dtype=torch.float32) * d ** 0.5 / 8.0)[None, :, None]
    r = _reference(qkv, 2, S_ADV, d)
    _check(engine, qkv, r, 2, S_ADV, d, "ramp")


@pytest.mark.parametrize("d", [64, 32])
def test_nan_window_and_overflow_count(engine, d):
    """An all-NaN window gives NaN outputs and leaves the x3 range counter at 0 (the reference's result for an empty window); its
    neighbour is untouched.  A finite |v| >= 65520 raises the counter; normal inputs leave it at 0."""
    qkv = _base(d, 14, 2.0)
    r = _reference(qkv[:1].clone(), 1, S_ADV, d)
    qkv[1] = float("nan")
    engine.x3_overflow_clear()
    o32, ox3, obf = _run(engine, qkv, 2, S_ADV, d, r["scale"])
    assert engine.x3_overflow_count() == 0
    for name, o in (("f32", o32), ("x3", ox3), ("bf16", obf)):
        assert torch.isnan(o[1].float()).all(), name
    for name, o, ref in (("f32", o32, r["ref"]), ("x3", ox3, r["ref"])):
        rel, worst = _measure(o[:1], ref)
        assert rel < r["rel_bound"] and worst < r["max_bound"], (name, rel, worst)
    big = _base(d, 15, 2.0)
    _parts(big, d)[2][0, 5, 1, 3] = 70000.0
    _run(engine, big, 2, S_ADV, d, r["scale"])
    assert engine.x3_overflow_count() > 0
    _run(engine, _base(d, 15, 2.0), 2, S_ADV, d, r["scale"])
    assert engine.x3_overflow_count() == 0


def test_argument_errors(engine):
    from avcer_amd._lib import AvcerError

    x = torch.zeros(1, 64, 3 * 64, device=engine.device)
    for s, d, kinds in ((5001, 64, (0, 0)), (0, 64, (0, 0)), (64, 48, (0, 0)), (64, 64, (0, 1)), (64, 64, (2, 2))):
        with pytest.raises(AvcerError):
            engine.attention_long(x, x, 1, s, 1, d, 0.125, *kinds)


@pytest.mark.parametrize("kinds", [(0, 0), (0, 2), (1, 1)], ids=["f32", "x3", "bf16"])
@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("s", [1, 17, 99, KT])
def test_one_key_tile_is_the_whole_head_kernel(engine, s, d, kinds):
    """Up to KT keys the streamed kernels see one key tile: the factor on the running sums is exp(-inf) = 0 on zeros, the image
    has the 8 MFMA key tiles of the whole-head kernel at s <= 128, and every sum is formed in the same order, so engine.attention
    and engine.attention_long return the same bits."""
    n, (ik, ok) = 2, kinds
    qkv = _random_case(s, d, n)[0]
    x = (qkv.to(torch.bfloat16) if ik == 1 else qkv).to(engine.device)
    shape, dtype = ((n, s, 2 * HEADS * d), torch.int16) if ok == 2 else ((n, s, HEADS * d), torch.bfloat16 if ok == 1 else torch.float32)
    outs = []
    for fn in (engine.attention, engine.attention_long):
        o = torch.zeros(shape, dtype=dtype, device=engine.device)
        fn(x, o, n, s, HEADS, d, 1.0 / d ** 0.5, ik, ok)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
