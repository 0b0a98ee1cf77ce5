"""The S3FD detector launch by launch against float64 (detect.hip face_s3fd_forward_lane): every one of its 24 launches in front of
the heads -- the stem, 18 contractions, 5 pools -- is tapped whole for two 239 x 431 frames, in the exact-f32 and the x3 mode, and

  (a) compared with the float64 oracle (tests/s3fd_ref.py s3fd_forward64), max|err| / max|ref| per tap.  The bound is 8 x what the
      float32 CPU restatement shows on the same frames against the same oracle, computed where the test runs; the pools are also
      required exact (torch.equal with max_pool2d of the library's own tapped input);
  (b) each contraction judged from the library's OWN tapped input, decoded to float64, that one layer in float64, per element
          |got - ref| <= (K + 2) 2^-24 (sum |x||w| + |b|)
                         + in x3: 2 * 2^-22 sum |x||w|  (the weight pair's representation, the dropped lo * lo product)
                         + in x3: 2^-22 |ref| + 2^-25   (the sp32 store)
      which needs no measurement and separates a launch's own error from what it inherits;
  (c) the kernel family of every contraction, from the launch log: the staged and the skinny x3 form serve this call, a third frame
      brings in the weights-direct one, and what it computes is tied bit for bit to the taps of (a) and (b);
  (d) loc / conf of the call against float64 under (a)'s rule, the gates 1e-4 / 1e-3, no x3 overflow;
  (e) at 1920 x 1080, where a pass holds 3 frames: 7 frames (passes of 3, 3, 1 in one lane) and 16 frames (two lanes of 8, passes of
      3, 3, 2), the first and last frame of every pass bit-identical to the same frame run alone.

239 x 431: both floor pools in front of vgg.16 drop a row and a column (239 -> 119 -> 59, 431 -> 215 -> 107), vgg.16 (ceil_mode)
overhangs both ways (59 -> 30, 107 -> 54), fc6's map is 7 x 13, so its dilated taps read data in both directions with different
counts, ex1 strides an odd map (7 x 13 -> 4 x 7), ex3 an even and an odd extent (4 x 7 -> 2 x 4).

Figures measured on an MI355X.  (a): max|err| / max|ref| against float64, the device in both modes and the float32 CPU
restatement, whose figure x 8 is the bound: the device needs at most 4.7 x (f32 mode, fc6) and 4.8 x (x3, vgg.24) of it, no tap
needs the whole margin.  (b): worst err / bound per launch.  Last column: the form that served the contraction in x3 in the
two-frame call and in the three-frame call of (c) (S = LDS-staged conv_gemm_kernel, W = weights-direct conv_gemm_wd_kernel,
K = skinny conv_gemm_skinny_kernel; the f32 mode runs conv_gemm_kernel throughout):
  launch       output [c,h,w]   (a) f32    (a) x3     CPU f32    (b) f32  (b) x3   x3 form, 2 / 3 frames
  conv1        64, 239, 431     2.19e-07   2.66e-07   2.73e-07   0.1651   0.1621   - / -
  out:vgg2.w   64, 239, 431     8.27e-07   6.81e-07   3.20e-07   0.0112   0.0087   S / S
  pool1        64, 119, 215     8.27e-07   6.81e-07   3.20e-07   0.0000   0.0000   - / -
  out:vgg5.w   128, 119, 215    1.23e-06   7.48e-07   4.80e-07   0.0079   0.0047   S / S
  out:vgg7.w   128, 119, 215    1.56e-06   1.16e-06   4.20e-07   0.0053   0.0038   S / S
  pool2        128, 59, 107     1.56e-06   1.16e-06   4.20e-07   0.0000   0.0000   - / -
  out:vgg10.w  256, 59, 107     1.71e-06   1.29e-06   5.38e-07   0.0045   0.0030   S / W
  out:vgg12.w  256, 59, 107     2.03e-06   1.60e-06   4.55e-07   0.0022   0.0018   S / W
  out:vgg14.w  256, 59, 107     2.13e-06   1.94e-06   5.83e-07   0.0019   0.0016   S / W
  pool3        256, 30, 54      2.13e-06   1.86e-06   5.47e-07   0.0000   0.0000   - / -
  out:vgg17.w  512, 30, 54      2.50e-06   2.64e-06   5.51e-07   0.0025   0.0022   S / S
  out:vgg19.w  512, 30, 54      2.88e-06   2.70e-06   6.66e-07   0.0011   0.0009   S / S
  out:vgg21.w  512, 30, 54      3.32e-06   2.83e-06   8.10e-07   0.0009   0.0008   S / S
  pool4        512, 15, 27      2.74e-06   2.77e-06   8.10e-07   0.0000   0.0000   - / -
  out:vgg24.w  512, 15, 27      2.68e-06   2.97e-06   6.14e-07   0.0009   0.0007   K / S
  out:vgg26.w  512, 15, 27      3.42e-06   3.07e-06   8.11e-07   0.0010   0.0007   K / S
  out:vgg28.w  512, 15, 27      3.56e-06   3.19e-06   8.11e-07   0.0009   0.0008   K / S
  pool5        512, 7, 13       3.56e-06   3.15e-06   8.11e-07   0.0000   0.0000   - / -
  out:vgg31.w  1024, 7, 13      2.24e-06   1.91e-06   4.81e-07   0.0008   0.0007   K / K
  out:vgg33.w  1024, 7, 13      2.27e-06   2.25e-06   8.51e-07   0.0035   0.0033   K / K
  out:ex0.w    256, 7, 13       3.43e-06   2.60e-06   9.85e-07   0.0031   0.0023   K / K
  out:ex1.w    512, 4, 7        2.45e-06   2.51e-06   6.90e-07   0.0015   0.0016   K / K
  out:ex2.w    128, 4, 7        3.01e-06   2.61e-06   7.64e-07   0.0050   0.0045   K / K
  out:ex3.w    256, 2, 4        2.61e-06   2.27e-06   6.14e-07   0.0017   0.0015   K / K
(d) the call's outputs, same metric: loc 4.43e-06 (f32) / 3.54e-06 (x3) against the CPU's 1.04e-06, conf 6.53e-06 / 6.10e-06 against
2.16e-06; as absolute differences loc 1.8e-05 / 1.4e-05 and conf 6.5e-06 / 6.1e-06, against the gates 1e-3 / 1e-4.

What the checks catch.  Each departure below was planted in the ORACLE through its hook (never in a kernel) and the comparison run
against the device's taps; (a) must fail at the changed launch and behind it, never in front of it; (b) judges every launch from
its own input, so it fails at the changed launch alone.
  departure                                   (a) fails at (both modes)                          (a) figure there   (b) err / bound there
  1 fc6 with dilation 5, padding 5            out:vgg31.w and all 5 taps behind, none in front    8.3e-1             1130
  2 vgg.24 without its last input column      out:vgg24.w and all 9 behind, none in front         5.0e-1             291
  3 ex1 at the odd positions                  out:ex1.w, out:ex2.w, out:ex3.w, none in front      6.3e-1             1680
  4 pool2 ceil_mode, cropped at the front     pool2 and all 18 behind, none in front              6.8e-1             not equal (pools are exact)
  5 vgg.12 without its bias                   out:vgg12.w and all 16 behind, none in front        6.0e-3             23.8
  6 out:vgg19.w rounded to 11 significant     out:vgg19.w and all 12 behind, none in front        4.5e-4             0.24: (b) does NOT see it
    bits (a lost lo half)
Departure 4 as first worded -- pool2 with ceil_mode and the extra row and column cropped off again at the END -- is no departure:
ceil_mode only appends a row and a column (119 x 215 -> 60 x 108), cropping them gives the floor pool's 59 x 107 values bit for bit,
and every check passes, as it must.  The table's row crops the FIRST row and column instead (a pool shifted by one window).
Departure 6 planted at each contraction in turn and judged by (b), err / bound (f32 mode; x3 within 2 %): K = 576: 4.9 (vgg2), 2.6
(vgg5); K = 512: 4.3 (ex2); K = 1024: 1.5 (fc7), 1.1 (ex0); K = 1152: 1.3 (vgg7), 1.2 (vgg10), 1.3 (ex3) -- seen; K = 2304: 0.54
(vgg12), 0.57 (vgg14), 0.46 (vgg17), 0.59 (ex1); K = 4608: 0.20 .. 0.31 (vgg19 .. fc6) -- NOT seen.  (b)'s bound grows with
(K + 2) 2^-24 sum |x||w| against the departure's 2^-12 |ref|, and sum |x||w| is several times |ref|: from K = 2304 on the worst-case
bound is wider than a lost lo half, so (b) sees it only up to K = 1152 and (a), at 4.5e-4 against a bound of 5.3e-6, is the check
that holds there.  The kernels themselves sit at 0.0007 .. 0.011 of (b)'s bound (the stem at 0.17).
"""
import numpy as np
import pytest
import torch

import s3fd_ref
from avcer_amd import synth
from avcer_amd.engine import MODE_F16X3, MODE_FP32, Engine
from avcer_amd.sp32 import raw_to_f32

pytestmark = pytest.mark.gpu

H, W, N = 239, 431, 2
MODES = {MODE_FP32: "fp32", MODE_F16X3: "x3"}
U = 2.0 ** -24     # unit roundoff of f32
MARGIN = 8.0       # device bound = MARGIN x the float32 CPU restatement's figure (the GRU test's margin for a compounding comparison)
FORMS = {"conv_gemm_kernel": "S", "conv_gemm_wd_kernel": "W", "conv_gemm_skinny_kernel": "K"}


@pytest.fixture(scope="module")
def sd_s3fd():
    return synth.to_torch(synth.s3fd_state_dict(42))


@pytest.fixture(scope="module")
def eng(sd_s3fd):
    """A fresh engine: a full 1080p pass grows the detector's workspace to 3 GiB per lane, which the session engine must not keep."""
    e = Engine(0)
    try:
        e.load_face(sd_s3fd)
        yield e
    finally:
        e.close()


@pytest.fixture(scope="module")
def frames():
    return synth.video_frames(239431, N, H, W)


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope="module")
def oracle(sd_s3fd, frames):
    """The float64 run (every launch's output, loc, conf) and, per tap, what the float32 run of the same function shows against it."""
    t64, t32 = {}, {}
    loc, conf, _ = s3fd_ref.s3fd_forward64(sd_s3fd, frames, t64)
    l32, c32, _ = s3fd_ref.s3fd_forward64(sd_s3fd, frames, t32, dtype=torch.float32)
    cpu = {k: _rel(t32[k], t64[k]) for k in s3fd_ref.LAUNCHES}
    cpu["loc"], cpu["conf"] = _rel(l32, loc), _rel(c32, conf)
    return dict(taps={k: t64[k] for k in s3fd_ref.LAUNCHES}, loc=loc, conf=conf, cpu=cpu)


def read_tap(eng, frames_dev, mode, name, shape, whole=True):
    """One launch's output, NCHW f32 on the host.  `shape` is the oracle's [n,c,h,w]; the tap is armed for 64 bytes more than that,
    so a library tensor of another size shows in the copied byte count (whole=False: the call has more frames than `shape`, the
    first n are read)."""
    n, c, h, w = shape
    numel = n * c * h * w
    x3 = mode == MODE_F16X3
    over = 1 if whole else 0
    raw = eng.debug_tap(name if name.startswith("out:") else "s3fd_" + name, numel * (2 if x3 else 1) + over * (32 if x3 else 16),
                        torch.int16 if x3 else torch.float32)
    eng.face_forward(frames_dev, mode)
    torch.cuda.synchronize()
    assert eng.debug_tap_copied() == numel * 4, (name, eng.debug_tap_copied(), numel * 4)
    raw = raw.cpu()[:numel * (2 if x3 else 1)]
    t = raw_to_f32(raw, (n, h, w, c)) if x3 else raw.reshape(n, h, w, c)
    return t.permute(0, 3, 1, 2).contiguous()


def device_taps(eng, frames, mode, shapes):
    fd = torch.from_numpy(np.ascontiguousarray(frames)).to(eng.device)
    return {k: read_tap(eng, fd, mode, k, shapes[k]) for k in s3fd_ref.LAUNCHES}


@pytest.fixture(scope="module")
def dev(eng, frames, oracle):
    shapes = {k: tuple(v.shape) for k, v in oracle["taps"].items()}
    eng.x3_overflow_count(reset=True)
    return {mode: device_taps(eng, frames, mode, shapes) for mode in MODES}


def tap_figures(taps, ref):
    """(a): max|err| / max|ref| per launch, in launch order."""
    return {k: _rel(taps[k], ref[k]) for k in s3fd_ref.LAUNCHES}


def launch_ratios(sd, taps, frames, mode, hook=None, only=None):
    """(b): per launch, the worst |got - ref| / bound over all elements, `ref` being that ONE launch in float64 on the library's own
    tapped input; a pool's entry is 0.0 if it equals max_pool2d of its tapped input bit for bit, inf if not."""
    x3 = mode == MODE_F16X3
    out = {}
    for spec in (s3fd_ref.STEM,) + tuple(s3fd_ref.contractions()):
        name, src = spec[:2]
        if src in s3fd_ref.POOL_INPUT and (only is None or src in only):
            if hook is not None and hasattr(hook, "prev"):
                hook.prev = taps[s3fd_ref.POOL_INPUT[src]]
            want = s3fd_ref.pool64(src, taps[s3fd_ref.POOL_INPUT[src]], hook)
            out[src] = 0.0 if torch.equal(taps[src], want.to(taps[src].dtype)) else float("inf")
        if only is not None and name not in only:
            continue
        x = torch.cat([s3fd_ref.preprocess(f, False, torch.float64) for f in frames]) if src is None else taps[src].double()
        if hook is not None and hasattr(hook, "prev"):
            hook.prev = x
        ref, sxw, babs, k = s3fd_ref.launch64(sd, spec, x, hook)
        bound = (k + 2) * U * (sxw + babs)
        if x3:
            bound = bound + (2 * 2.0 ** -22 * sxw if src is not None else 0.0) + 2.0 ** -22 * ref.abs() + 2.0 ** -25
        out[name] = float(((taps[name].double() - ref).abs() / bound).max())
    return out


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
def test_every_tap_against_the_float64_oracle(dev, oracle, mode):
    assert len(dev[mode]) == 24 and set(dev[mode]) == set(oracle["taps"]) == set(s3fd_ref.LAUNCHES)
    fig = tap_figures(dev[mode], oracle["taps"])
    bad = {}
    for k, v in fig.items():
        cpu = oracle["cpu"][k]
        print(f"(a) {MODES[mode]:4s} {k:12s} {tuple(dev[mode][k].shape)!s:20s} device {v:.2e}  cpu f32 {cpu:.2e}  x{v / cpu:5.2f}")
        if not v <= MARGIN * cpu:
            bad[k] = (v, cpu)
    assert not bad, (MODES[mode], bad)
    for p, src in s3fd_ref.POOL_INPUT.items():
        assert torch.equal(dev[mode][p], s3fd_ref.pool64(p, dev[mode][src])), (MODES[mode], p)


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES.values()))
def test_every_contraction_from_its_own_input_under_the_derived_bound(dev, sd_s3fd, frames, mode):
    ratios = launch_ratios(sd_s3fd, dev[mode], frames, mode)
    assert len(ratios) == 24
    for k, v in ratios.items():
        print(f"(b) {MODES[mode]:4s} {k:12s} worst err / bound {v:.4f}")
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (MODES[mode], bad)


# ---------------------------------------------------------------------------------------------------------------- (c)
def contraction_forms(eng, frames, mode):
    """Kernel family of each of the 18 contractions of one call, in launch order (the stem, the pools and the heads are not
    contraction launches and do not enter the log)."""
    fd = torch.from_numpy(np.ascontiguousarray(frames)).to(eng.device)
    eng.face_forward(fd, mode)      # weights prepared, workspace sized
    torch.cuda.synchronize()
    eng.profile_enable(True)
    try:
        eng.face_forward(fd, mode)
        log = eng.profile_read_launches()
    finally:
        eng.profile_enable(False)
    return [(l["family"], l["m"], l["n"], l["k"]) for l in log]


def test_which_form_ran(eng, sd_s3fd, frames, oracle, dev):
    """The two-frame call runs the LDS-staged form (conv1_2 .. conv4_3) and the skinny one (conv5_1 .. extras.3); no layer of it
    takes the weights-direct form.  The smallest call that brings it in is THREE frames of 239 x 431: conv3_1 .. conv3_3 (18 939
    positions x 256 channels) then run weights-direct, conv5_1 .. conv5_3 (1215 positions) move from the skinny to the staged form,
    fc6 .. extras.3 stay skinny.  The forms are bit-identical by contract, so every layer whose form differs between the two calls
    is tapped in the three-frame call and its first two frames must equal, bit for bit, the taps that (a) and (b) checked."""
    specs = s3fd_ref.contractions()
    three = np.concatenate([frames, synth.video_frames(239432, 1, H, W)])
    forms = {}
    for mode in MODES:
        for call, n in ((frames, 2), (three, 3)):
            log = contraction_forms(eng, call, mode)
            assert len(log) == len(specs) == 18, log
            for (fam, m, nn, k), spec in zip(log, specs):
                shape = oracle["taps"][spec[0]].shape
                wt = sd_s3fd[spec[2] + ".weight"]
                assert (m, nn, k) == (n * shape[2] * shape[3], wt.shape[0], wt[0].numel()), (spec[0], m, nn, k)
                print(f"(c) {MODES[mode]:4s} {n} frames {spec[0]:12s} M {m:6d} N {nn:4d} K {k:4d}  {fam}")
            forms[mode, n] = [l[0] for l in log]
    assert set(forms[MODE_FP32, 2]) == set(forms[MODE_FP32, 3]) == {"conv_gemm_kernel"}
    assert set(forms[MODE_F16X3, 2]) | set(forms[MODE_F16X3, 3]) == set(FORMS), forms
    moved = [spec[0] for spec, a, b in zip(specs, forms[MODE_F16X3, 2], forms[MODE_F16X3, 3]) if a != b]
    print("(c) x3 layers whose form differs between the calls:", moved)
    assert any(b == "conv_gemm_wd_kernel" for a, b in zip(forms[MODE_F16X3, 2], forms[MODE_F16X3, 3]) if a != b)
    td = torch.from_numpy(np.ascontiguousarray(three)).to(eng.device)
    for name in moved:
        got = read_tap(eng, td, MODE_F16X3, name, tuple(oracle["taps"][name].shape), whole=False)
        assert torch.equal(got, dev[MODE_F16X3][name]), name
    for mode in MODES:
        l2, c2, _ = eng.face_forward(frames, mode)
        l3, c3, _ = eng.face_forward(three, mode)
        assert torch.equal(l3[:2], l2) and torch.equal(c3[:2], c2), MODES[mode]


# ---------------------------------------------------------------------------------------------------------------- (d)
def test_heads_and_outputs(eng, frames, oracle, dev):
    for mode in MODES:
        loc, conf, lm = eng.face_forward(frames, mode)
        assert lm is None and tuple(loc.shape) == (N, s3fd_ref.num_priors(H, W), 4) == tuple(oracle["loc"].shape)
        loc, conf = loc.cpu(), conf.cpu()
        r_loc, r_conf = _rel(loc, oracle["loc"]), _rel(conf, oracle["conf"])
        d_loc, d_conf = float((loc.double() - oracle["loc"]).abs().max()), float((conf.double() - oracle["conf"]).abs().max())
        print(f"(d) {MODES[mode]:4s} loc {r_loc:.2e} (cpu f32 {oracle['cpu']['loc']:.2e}, max|d| {d_loc:.2e})  "
              f"conf {r_conf:.2e} (cpu f32 {oracle['cpu']['conf']:.2e}, max|d| {d_conf:.2e})")
        assert r_loc <= MARGIN * oracle["cpu"]["loc"] and r_conf <= MARGIN * oracle["cpu"]["conf"], (MODES[mode], r_loc, r_conf)
        assert d_conf < 1e-4 and d_loc < 1e-3
    assert eng.x3_overflow_count() == 0


# ---------------------------------------------------------------------------------------------------------------- (e)
def max_frames(h, w):
    """detect.hip face_s3fd_max_frames: conv1's maps of a pass (64 channels at full resolution, 4 bytes each) stay below 1.5 GiB."""
    return max(1, 0x60000000 // (h * w * 64 * 4))


def passes(h, w, n):
    """Frames per pass in each lane: face_forward_impl's split at 16 frames into halves with passes of equal size, the lane's cap."""
    cap = max_frames(h, w)
    if n < 16:
        lanes = [(n, n)]
    else:
        n0 = (n + 1) // 2
        p = -(-n0 // cap)
        lanes = [(n0, -(-n0 // p)), (n - n0, -(-n0 // p))]
    out = []
    for count, lane_cap in lanes:
        nb = min(count, lane_cap, cap)
        out.append([min(nb, count - s) for s in range(0, count, nb)])
    return out


def pass_edges(schedule):
    e, f0 = [], 0
    for lane in schedule:
        for nb in lane:
            e += [f0, f0 + nb - 1]
            f0 += nb
    return sorted(set(e))


def test_passes_and_lanes_at_1080p(eng):
    """Five distinct frames, frame i of a call = distinct frame i mod 5: no two passes and no two lanes of either call start with
    the same frame or hold the same sequence, so a pass that read or wrote at another pass's offset shows.  A full pass holds
    3 x 1080 x 1920 x 64 x 4 = 1.5 GiB per ping-pong buffer; the lone call's offsets are small, an independent witness."""
    h, w = 1080, 1920
    assert max_frames(h, w) == 3 and max_frames(360, 640) == 27
    assert 3 * h * w * 64 * 4 > 0x5E000000
    assert passes(h, w, 7) == [[3, 3, 1]] and passes(h, w, 16) == [[3, 3, 2], [3, 3, 2]]
    assert pass_edges(passes(h, w, 7)) == [0, 2, 3, 5, 6]
    assert pass_edges(passes(h, w, 16)) == [0, 2, 3, 5, 6, 7, 8, 10, 11, 13, 14, 15]
    distinct = synth.video_frames(1080, 5, h, w)
    dd = torch.from_numpy(np.ascontiguousarray(distinct)).to(eng.device)
    for mode in MODES:
        alone = [[t.clone() for t in eng.face_forward(dd[j:j + 1], mode)[:2]] for j in range(5)]
        assert not torch.equal(alone[0][1], alone[1][1])
        for n in (7, 16):
            idx = [i % 5 for i in range(n)]
            call = dd[idx].contiguous()
            loc, conf, _ = eng.face_forward(call, mode)
            for i in pass_edges(passes(h, w, n)):
                assert torch.equal(loc[i], alone[idx[i]][0][0]), (MODES[mode], n, "loc", i)
                assert torch.equal(conf[i], alone[idx[i]][1][0]), (MODES[mode], n, "conf", i)
            if n == 7:
                l2, c2, _ = eng.face_forward(call.flip(-1).contiguous(), mode, rgb=True)
                assert torch.equal(l2, loc) and torch.equal(c2, conf), (MODES[mode], "rgb")
            del loc, conf
    assert eng.x3_overflow_count() == 0
    torch.cuda.synchronize()
