"""RetinaFace-R50 detector stage by stage against the float64 oracle (oracle/retina.py retina_forward64), at 1080p among other
sizes, and across the pass and lane boundaries of the benchmark's call and of 1080p batches (detect.hip face_forward_lane /
face_forward_impl).  A fresh Engine per module: passes of up to 273 frames grow the detector's workspace slots to tens of GB, which
the session engine must not keep."""
import re
import time

import numpy as np
import pytest
import torch

from avcer_amd import face_tiles as ft
from avcer_amd import synth
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine
from avcer_amd.sp32 import raw_to_f32
from oracle import retina as orf

pytestmark = pytest.mark.gpu

PASS_LIMIT = 0xF0000000        # detect.hip face_forward_lane: every gathered operand of a pass stays below the 4 GiB descriptor range
TAIL_PAIR_ROWS = 16384         # net.h kTailPairRows: stage-3 tails of more positions run bneck_tail2_kernel
MODES = {MODE_FP32: "fp32", MODE_F16X3: "x3"}


@pytest.fixture(scope="module")
def sd_retina():
    return synth.to_torch(synth.retina_state_dict(42))


@pytest.fixture(scope="module")
def eng(sd_retina):
    e = Engine(0)
    try:
        e.load_face(sd_retina)
        yield e
    finally:
        e.close()


def _grids(h, w):
    """Stem output, max-pool output and the extents of layer2 .. layer4 (the pyramid), as face_forward_lane computes them."""
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    mh, mw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    lv, (fh, fw) = [], (mh, mw)
    for _ in range(3):
        fh, fw = (fh - 1) // 2 + 1, (fw - 1) // 2 + 1
        lv.append((fh, fw))
    return (oh, ow), (mh, mw), lv


def _per_frame_bytes(h, w):
    (oh, ow), (mh, mw), _ = _grids(h, w)
    return max((2 * (oh - 1) + 8) * (2 * (ow - 1) + 8) * 4, oh * ow * 64, mh * mw * 256) * 4


def _passes(h, w, n, lanes):
    """Frames per pass in each lane: face_forward_impl's lane split and pass cap, face_forward_lane's pass size."""
    nb_max = max(1, PASS_LIMIT // _per_frame_bytes(h, w))
    if lanes == 1 or n < 16:
        caps = [(n, n)]
    else:
        n0 = (n + 1) // 2
        passes = -(-n0 // nb_max)
        cap = -(-n0 // passes)
        caps = [(n0, cap), (n - n0, cap)]
    out = []
    for frames, cap in caps:
        nb = max(1, min(frames, cap, nb_max))
        out.append([min(nb, frames - s) for s in range(0, frames, nb)])
    return out


def _edges(schedules):
    """First and last frame of every pass of every schedule."""
    e = set()
    for lanes in schedules:
        f0 = 0
        for lane in lanes:
            for nb in lane:
                e |= {f0, f0 + nb - 1}
                f0 += nb
    return sorted(e)


# ------------------------------------------------------------------------------------------------------------ stage taps
def _tap_list(mode, stage3_rows):
    """(library tap, oracle tap) pairs the forward of `mode` fills (visual.hip run_bneck_stage / detect.hip face_forward_lane): in x3 mode the
    chains of stages 1-2 tap their block output and the next block's conv1 output, the stage-3 tails only when bneck_tail2_kernel
    runs (more than TAIL_PAIR_ROWS positions); conv2 of layer1.0 is a tensor of its own only off the chain."""
    x3 = mode == MODE_F16X3
    taps = [("face_pool", "pool"), ("face_l1b0_c1", "c1:l1.0.")]
    if not x3:
        taps.append(("face_l1b0_c2", "l1b0_c2"))
    taps.append(("face_l1b0", "blk1_0"))
    for li, (_, blocks, _) in enumerate(orf.STAGES, start=1):
        for b in range(blocks):
            taps.append((f"face_blk{li}_{b}", f"blk{li}_{b}"))
            p, nxt = f"l{li}.{b}.", f"c1:l{li}.{b + 1}."
            if x3 and (li == 1 or (li == 2 and b >= 1)):
                taps.append((f"face_chain_out:{p}", f"blk{li}_{b}"))
                if b + 1 < blocks:
                    taps.append((f"face_chain_t1n:{p}", nxt))
            if x3 and li == 3 and 1 <= b < blocks - 1 and stage3_rows > TAIL_PAIR_ROWS:
                taps += [(f"face_tail_out:{p}", f"blk{li}_{b}"), (f"face_tail_t1n:{p}", nxt)]
    taps += [("face_layer1", "layer1"), ("face_body1", "body1"), ("face_body2", "body2"), ("face_body3", "body3"),
             ("face_lat1", "lat1"), ("face_lat2", "lat2"), ("face_lat3", "lat3"), ("face_sum2", "sum2"), ("face_fpn2", "fpn2"),
             ("face_fpn1", "fpn1"), ("face_ssh1", "ssh1")]
    return taps


def _tap(eng, name, frames, mode, ref_nhwc):
    """Frame 0's part of one debug tap (an armed tap forces one lane; the copy is the first bytes of the NHWC batch)."""
    x3 = mode == MODE_F16X3
    dst = eng.debug_tap(name, ref_nhwc.numel() * (2 if x3 else 1), dtype=torch.int16 if x3 else torch.float32)
    eng.face_forward(frames, mode)
    torch.cuda.synchronize()
    assert eng.debug_tap_copied() == ref_nhwc.numel() * 4, name
    got = raw_to_f32(dst.cpu(), tuple(ref_nhwc.shape)) if x3 else dst.cpu().view(ref_nhwc.shape)
    return got.double()


def _family(tap):
    """Tap name (without "face_") -> "s1" .. "s4" (stem + max-pool with stage 1), "lat" (laterals) or "fpn" (merge2's input, the
    merged levels and SSH)."""
    if tap in ("sum2", "fpn2", "fpn1", "ssh1"):
        return "fpn"
    if tap.startswith("lat"):
        return "lat"
    if tap in ("pool", "layer1") or tap.startswith("l1b0"):
        return "s1"
    m = re.search(r"blk(\d)_|:l(\d)\.|body(\d)", tap)
    return "s" + (m.group(1) or m.group(2) or str(int(m.group(3)) + 1))


# max|err| / max|ref|, about 4x the worst tap of the family over the three sizes; ceiling 5e-5 in both f32-grade modes (DESIGN
# section 6).  Rounding one stage-3 conv's weights to fp16 on the oracle side (an x3 contraction without its lo term) lifts that
# block's tap to 7.2e-5 and every later tap above its bound.
TAP_BOUND = {
    MODE_FP32: {"s1": 4e-6,     # measured 1.0e-6 (l1b0_c2, 1080p)
                "s2": 4e-6,     # measured 8.8e-7 (blk2_0, 1080p)
                "s3": 5e-6,     # measured 1.3e-6 (blk3_0, 1080p)
                "s4": 7e-6,     # measured 1.7e-6 (blk4_0, 1080p)
                "lat": 1e-5,    # measured 2.4e-6 (lat3, 1080p)
                "fpn": 1.4e-5},  # measured 3.4e-6 (fpn1, 1080p)
    MODE_F16X3: {"s1": 3e-6,    # measured 6.5e-7 (chain_t1n:l1.1., 1080p)
                 "s2": 4e-6,    # measured 9.4e-7 (chain_t1n:l2.2., 1080p)
                 "s3": 6e-6,    # measured 1.4e-6 (tail_t1n:l3.4., 1080p)
                 "s4": 7e-6,    # measured 1.7e-6 (blk4_0, 1080p)
                 "lat": 1e-5,   # measured 2.3e-6 (lat3, 1080p)
                 "fpn": 1.2e-5},  # measured 2.8e-6 (fpn1, 1080p)
}


def test_stage_taps_against_float64_oracle(eng, sd_retina):
    """Every detector tap of frame 0 at 75 x 101 (odd extents at every level), 360 x 640 (the benchmark's frames) and 1920 x 1080
    (whole video frames: pyramid 135 x 240 -> 68 x 120 -> 34 x 60, nearest-upsample ratios 68/135 and 34/68), in the exact-f32 and
    the x3 mode, against the float64 oracle.  1080p runs three frames, so that stage 3 holds 24480 positions and its tails run
    bneck_tail2_kernel (one frame takes the tail pair, as the two smaller sizes do)."""
    t_start = time.time()
    worst, outputs = {m: {} for m in MODES}, {}
    for (h, w, n) in ((75, 101, 1), (360, 640, 1), (1080, 1920, 3)):
        frames = synth.video_frames(1080 + h, n, h, w)
        ref = {}
        rl, rc, rm = orf.retina_forward64(sd_retina, frames[0], ref)
        _, _, lv = _grids(h, w)
        stage3 = n * lv[1][0] * lv[1][1]
        for mode in MODES:
            for lib, orc in _tap_list(mode, stage3):
                r = ref[orc][0].permute(1, 2, 0).contiguous()
                got = _tap(eng, lib, frames, mode, r)
                rel = ((got - r).abs().max() / r.abs().max()).item()
                key = lib[len("face_"):]
                if rel >= worst[mode].get(key, (-1.0,))[0]:
                    worst[mode][key] = (rel, f"{h}x{w}")
            if (h, w) == (1080, 1920):
                loc, conf, lm = (t[0].cpu().double() for t in eng.face_forward(frames, mode))
                dc = (conf - rc[0]).abs().max().item()
                dl = ((loc - rl[0]).abs().max() / rl[0].abs().max()).item()
                dm = ((lm - rm[0]).abs().max() / rm[0].abs().max()).item()
                outputs[mode] = (dc, dl, dm)
                print(f"1080p {MODES[mode]} outputs: max|dconf| {dc:.2e}, loc {dl:.2e}, landms {dm:.2e} (relative)")
        del ref
    for mode, taps in worst.items():
        top = max(taps.items(), key=lambda kv: kv[1][0])
        print(f"{MODES[mode]} worst tap {top[0]} {top[1][0]:.2e} at {top[1][1]}; per tap:",
              {k: f"{v[0]:.1e}@{v[1]}" for k, v in taps.items()})
    print(f"stage taps: {time.time() - t_start:.1f} s")
    for mode, taps in worst.items():
        bad = {k: v for k, v in taps.items() if v[0] >= TAP_BOUND[mode][_family(k)]}
        assert not bad, (MODES[mode], bad)
    for mode, (dc, dl, dm) in outputs.items():
        # measured 1.3e-5 / 4.4e-6 / 3.1e-6 (fp32), 9.4e-6 / 3.4e-6 / 2.6e-6 (x3)
        assert dc < 1e-4 and dl < 2e-5 and dm < 2e-5, (MODES[mode], dc, dl, dm)


# ------------------------------------------------------------------------------------------------------- passes and lanes
def _forward(eng, frames, mode, lanes):
    eng.set_static_lanes(lanes)
    try:
        return [t.clone() for t in eng.face_forward(frames, mode)]
    finally:
        eng.set_static_lanes(2)


def _check_schedules(eng, sd_retina, frames, modes, sampled, oracle_frames):
    """Serial and two-lane calls give the same bits; each sampled frame alone gives its rows; the x3 rows agree with the
    exact-f32 mode under the gates of test_gpu_retina.py, and the oracle frames with the float64 oracle."""
    for mode in modes:
        serial = _forward(eng, frames, mode, 1)
        two = _forward(eng, frames, mode, 2)
        for a, b, what in zip(serial, two, ("loc", "conf", "landms")):
            assert torch.equal(a, b), (MODES[mode], what, "serial != two lanes")
        for i in sampled:
            one = eng.face_forward(frames[i:i + 1], mode)
            for a, b, what in zip(one, serial, ("loc", "conf", "landms")):
                assert torch.equal(a[0], b[i]), (MODES[mode], what, "frame", i)
            if mode == MODE_F16X3:
                l32, c32, m32 = (t[0].cpu() for t in eng.face_forward(frames[i:i + 1], MODE_FP32))
                loc, conf, lm = (t[i].cpu() for t in serial)
                assert (conf - c32).abs().max() < 1e-4 and (loc - l32).abs().max() < 1e-3 and (lm - m32).abs().max() < 1e-3, i
            if i in oracle_frames:
                rl, rc, rm = (t[0].float() for t in orf.retina_forward64(sd_retina, frames[i]))
                loc, conf, lm = (t[i].cpu() for t in serial)
                assert (conf - rc).abs().max() < 1e-4 and (loc - rl).abs().max() < 1e-3 and (lm - rm).abs().max() < 1e-3, i
        del serial, two


def _check_predictor(eng, sd_retina, frames, sampled):
    """RetinaFacePredictor.batch over the whole call (two lanes) against per-frame predictor calls: same rows, ties included."""
    pred = ft.RetinaFacePredictor(eng, sd_retina, threshold=0.3, mode=MODE_F16X3)
    together = pred.batch(frames, rgb=False)
    assert len(together) == len(frames)
    for i in sampled:
        np.testing.assert_array_equal(together[i], pred(frames[i], rgb=False))
    return sum(len(together[i]) for i in sampled)


def _device_used_gb():
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2 ** 30


def test_benchmark_call_passes_and_lanes(eng, sd_retina):
    """The benchmark's detector call: 750 frames of 640 x 360 in the x3 mode.  Serial, passes of 273 / 273 / 204 frames (layer 1's
    output of a full pass is 4 025 548 800 bytes, past 2^31 and 1 MB below the pass limit); two lanes, passes of 188 / 187 in
    each, so stage 3 runs bneck_tail2_kernel on 173 000 positions."""
    t0 = time.time()
    h, w, n = 360, 640, 750
    serial, two = _passes(h, w, n, 1), _passes(h, w, n, 2)
    assert serial == [[273, 273, 204]] and two == [[188, 187], [188, 187]], (serial, two)
    _, (mh, mw), lv = _grids(h, w)
    assert 2 ** 31 < 273 * mh * mw * 256 * 4 == 4025548800 < PASS_LIMIT
    assert 188 * lv[1][0] * lv[1][1] > TAIL_PAIR_ROWS
    sampled = _edges([serial, two])
    assert sampled == [0, 187, 188, 272, 273, 374, 375, 545, 546, 562, 563, 749], sampled
    frames = synth.video_frames(77, n, h, w)
    _check_schedules(eng, sd_retina, frames, (MODE_F16X3,), sampled, (272, 749))
    found = _check_predictor(eng, sd_retina, frames, sampled)
    print(f"640x360 x {n}: {time.time() - t0:.1f} s, device memory in use {_device_used_gb():.1f} GiB, "
          f"{found} detections in the sampled frames")


def test_1080p_passes_and_lanes(eng, sd_retina):
    """40 frames of 1920 x 1080 in both parity modes: serial, passes of 30 + 10 frames (3.98 GB of layer-1 output in the first);
    two lanes of one 20-frame pass each."""
    t0 = time.time()
    h, w, n = 1080, 1920, 40
    serial, two = _passes(h, w, n, 1), _passes(h, w, n, 2)
    assert serial == [[30, 10]] and two == [[20], [20]], (serial, two)
    _, (mh, mw), _ = _grids(h, w)
    assert 2 ** 31 < 30 * mh * mw * 256 * 4 < PASS_LIMIT
    sampled = [0, 19, 20, 29, 30, 39]
    assert set(_edges([serial, two])) == set(sampled)
    frames = synth.video_frames(1920, n, h, w)
    _check_schedules(eng, sd_retina, frames, (MODE_F16X3, MODE_FP32), sampled, (29,))
    found = _check_predictor(eng, sd_retina, frames, sampled)
    print(f"1920x1080 x {n}: {time.time() - t0:.1f} s, device memory in use {_device_used_gb():.1f} GiB, "
          f"{found} detections in the sampled frames")
