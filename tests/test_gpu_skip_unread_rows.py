"""The block in front of a strided last block stores only the rows that block reads (csrc/fused.hip KEEP, csrc/visual.hip
run_bneck_stage, avcer_set_skip_unread_rows).

Kernel level: the fused chain and the stage-3 tail with keep = 2 against the full-store launch of the entries every other test
binds (avcer_bneck_chain, avcer_bneck_tail).  OUT starts as a sentinel bit pattern; kept rows (even y, even x of every image) must
be bit-equal to the full store, T1N bit-equal everywhere, every other row of OUT still the sentinel.  One case per form of the
kernels that can sit in front of a strided block; shapes are the smallest that still cross an image border inside a 128-row
block, leave a ragged last block and have odd extents.

Network level: x3 forward passes with the switch on and off give the same bits, and an armed debug tap still gets whole tensors."""
import pytest
import torch

from avcer_amd import synth
from avcer_amd.engine import MODE_F16X3, AvcerError

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A  # as fp16 pairs: 203.25 + 203.25 in every channel of a row, which no computed row holds


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 777)


def _sp(g, *shape, dev):
    from avcer_amd.sp32 import to_sp32

    return to_sp32(torch.rand(*shape, generator=g) * 2).to(dev)


def _kept(nb, h, w, dev):
    """bool [nb * h * w]: the positions (2 oy, 2 ox) of every image."""
    y, x = torch.arange(h, device=dev)[:, None], torch.arange(w, device=dev)[None, :]
    return ((y % 2 == 0) & (x % 2 == 0)).expand(nb, h, w).reshape(-1)


def _compare(nb, h, w, run_full, run_keep, c_out, c_t1n, dev):
    m = nb * h * w
    outs = []
    for run in (run_full, run_keep):
        out = torch.full((m, 2 * c_out), SENTINEL, dtype=torch.int16, device=dev)
        t1n = torch.full((m, 2 * c_t1n), SENTINEL, dtype=torch.int16, device=dev)
        run(out, t1n)
        torch.cuda.synchronize()
        outs.append((out, t1n))
    (out_f, t1n_f), (out_k, t1n_k) = outs
    kept = _kept(nb, h, w, dev)
    assert 0 < int(kept.sum()) == nb * ((h + 1) // 2) * ((w + 1) // 2) < m
    # the full store wrote every row, so the sentinel tells a dropped row from a stored one
    assert bool((out_f != SENTINEL).any(dim=1).all()) and bool((t1n_f != SENTINEL).any(dim=1).all())
    assert torch.equal(out_k[kept], out_f[kept])
    assert torch.equal(t1n_k, t1n_f)
    assert bool((out_k[~kept] == SENTINEL).all())


_CHAINS = {
    "p64-spatial-tile-1": dict(planes=64, nb=1, h=55, w=55, frags=True),
    "p64-spatial-tile-2": dict(planes=64, nb=2, h=55, w=55, frags=True),
    "p64-gather": dict(planes=64, nb=3, h=7, w=9),      # 189 rows: a ragged second block, image borders inside both
    "p128-patch": dict(planes=128, nb=1, h=28, w=28),   # 784 rows, resident halo patch
    "p128-gather": dict(planes=128, nb=3, h=6, w=5),    # 90 rows: too few for the patch
}


@pytest.mark.parametrize("form", list(_CHAINS))
def test_chain_keeps_the_even_rows(engine, form):
    c = dict(frags=False)
    c.update(_CHAINS[form])
    planes, nb, h, w = c["planes"], c["nb"], c["h"], c["w"]
    dev, p4 = engine.device, 4 * c["planes"]
    g = _gen(planes, nb, h, w)
    t1, x = _sp(g, nb, h, w, planes, dev=dev), _sp(g, nb, h, w, p4, dev=dev)
    w2m = (torch.randn(planes, 9 * planes, generator=g) / (3 * planes ** 0.5)).to(dev)
    w2, w2f = engine.split_weight_rows(w2m), (engine.weight_frags(w2m) if c["frags"] else None)
    w3 = engine.split_weight_rows(torch.randn(p4, planes, generator=g) / planes ** 0.5)
    w1 = engine.split_weight_rows(torch.randn(planes, p4, generator=g) / p4 ** 0.5)
    b2, b3, b1 = ((torch.randn(n, generator=g) * 0.3).to(dev) for n in (planes, p4, planes))

    def full(out, t1n):
        engine.bneck_chain(planes, nb, h, w, t1, x, out, t1n, w2, b2, w3, b3, w1, b1, w2_frags=w2f)

    def keep(out, t1n):
        engine.bneck_chain_keep(planes, nb, h, w, t1, x, out, t1n, w2, b2, w3, b3, w1, b1, 2, w2_frags=w2f)

    _compare(nb, h, w, full, keep, p4, planes, dev)


@pytest.mark.parametrize("nb,h,w", [(1, 14, 14), (3, 5, 7)])  # 196 rows against 128-row blocks; 105 rows of odd extents
def test_tail_keeps_the_even_rows(engine, nb, h, w):
    dev, m = engine.device, nb * h * w
    g = _gen(nb, h, w, 256)
    t2, x = _sp(g, m, 256, dev=dev), _sp(g, m, 1024, dev=dev)
    w3 = engine.split_weight_rows(torch.randn(1024, 256, generator=g) / 16)
    w1n = engine.split_weight_rows(torch.randn(256, 1024, generator=g) / 32)
    b3, b1n = (torch.randn(1024, generator=g) * 0.3).to(dev), (torch.randn(256, generator=g) * 0.3).to(dev)

    def full(out, t1n):
        engine.bneck_tail(256, m, t2, x, out, t1n, w3, b3, w1n, b1n)

    def keep(out, t1n):
        engine.bneck_tail_keep(256, nb, h, w, t2, x, out, t1n, w3, b3, w1n, b1n, 2)

    _compare(nb, h, w, full, keep, 1024, 256, dev)


def test_keep_step_one_is_the_full_store_and_others_are_refused(engine):
    dev, nb, h, w, planes = engine.device, 1, 3, 3, 64
    g = _gen(1, 3, 3)
    t1, x = _sp(g, nb, h, w, planes, dev=dev), _sp(g, nb, h, w, 256, dev=dev)
    w2 = engine.split_weight_rows(torch.randn(planes, 9 * planes, generator=g) / 24)
    w3 = engine.split_weight_rows(torch.randn(256, planes, generator=g) / 8)
    w1 = engine.split_weight_rows(torch.randn(planes, 256, generator=g) / 16)
    b2, b3, b1 = ((torch.randn(n, generator=g) * 0.3).to(dev) for n in (planes, 256, planes))
    outs = [torch.full((9, 512), SENTINEL, dtype=torch.int16, device=dev) for _ in range(2)]
    t1ns = [torch.full((9, 128), SENTINEL, dtype=torch.int16, device=dev) for _ in range(2)]
    engine.bneck_chain(planes, nb, h, w, t1, x, outs[0], t1ns[0], w2, b2, w3, b3, w1, b1)
    engine.bneck_chain_keep(planes, nb, h, w, t1, x, outs[1], t1ns[1], w2, b2, w3, b3, w1, b1, 1)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(t1ns[0], t1ns[1])
    with pytest.raises(AvcerError):
        engine.bneck_chain_keep(planes, nb, h, w, t1, x, outs[1], t1ns[1], w2, b2, w3, b3, w1, b1, 3)
    with pytest.raises(AvcerError):  # no next conv1: not a block that sits in front of a strided one
        engine.bneck_chain_keep(planes, nb, h, w, t1, x, outs[1], None, w2, b2, w3, b3, None, None, 2)
    t2, xt = _sp(g, 9, 256, dev=dev), _sp(g, 9, 1024, dev=dev)
    with pytest.raises(AvcerError):
        engine.bneck_tail_keep(256, nb, h, w, t2, xt, outs[1], t1ns[1], w3, b3, w1, b1, 0)


# ----------------------------------------------------------------------------- network level
@pytest.fixture()
def switch(engine_static):
    """The shared engine with the switch restored to its default (on), and the lanes to theirs, afterwards."""
    try:
        yield engine_static
    finally:
        engine_static.set_skip_unread_rows(True)
        engine_static.set_static_lanes(2)


# 3 frames: the chains of stages 1-2 (stage 3's 588 positions run as two contractions).  84 frames on one lane: 16 464 positions
# in stage 3, the first size at which the forward pass takes the fused tail.
@pytest.mark.parametrize("n", [3, 84])
def test_forward_is_bit_identical_with_the_switch_on_and_off(switch, n):
    eng = switch
    eng.set_static_lanes(1)
    frames = torch.from_numpy(synth.face_frames(2468, n))
    other = torch.from_numpy(synth.face_frames(1357, n))
    res = {}
    for on in (False, True):
        eng.set_skip_unread_rows(False)
        eng.static_forward(other, MODE_F16X3)  # every workspace row now holds another input's values, the rows a pass leaves out too
        eng.set_skip_unread_rows(on)
        res[on] = [t.clone() for t in eng.static_forward(frames, MODE_F16X3)]
        torch.cuda.synchronize()
    for a, b in zip(res[False], res[True]):
        assert torch.isfinite(a).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name,hw,c", [("blk1_1", 55, 256), ("blk2_2", 28, 512)])
def test_an_armed_tap_still_gets_the_whole_tensor(switch, name, hw, c):
    """With a tap armed every row is stored whatever the switch says: the tapped output of the block in front of the strided one
    is the same with the switch on as with it off, at every position -- after a pass over OTHER frames that left its own values
    in the workspace rows a row-skipping pass would not overwrite."""
    eng = switch
    n = 3
    frames = torch.from_numpy(synth.face_frames(2468, n))
    other = torch.from_numpy(synth.face_frames(1357, n))
    got = {}
    for on in (False, True):
        eng.set_skip_unread_rows(False)
        eng.static_forward(other, MODE_F16X3)
        eng.set_skip_unread_rows(on)
        dst = eng.debug_tap(name, n * hw * hw * c * 2, dtype=torch.int16)
        eng.static_forward(frames, MODE_F16X3)
        torch.cuda.synchronize()
        assert eng.debug_tap_copied() == n * hw * hw * c * 4, name
        got[on] = dst.clone().view(n * hw * hw, 2 * c)
    assert torch.equal(got[False], got[True])
    assert bool((got[True] != 0).any(dim=1).all())  # every row was written by this pass (debug_tap hands out zeros)
