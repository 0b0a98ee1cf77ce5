"""The S3FD detector on the CPU: the restatement against the reference's own outputs, the priors, the packing, the ABI and the
build hygiene of csrc/s3fd.hip."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import detect_edge_cases as ec
import s3fd_ref
from avcer_amd import _lib, build, packing, synth
from avcer_amd import face_tiles as ft

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "s3fd_net.npz"))
DET = np.load(os.path.join(HERE, "golden", "s3fd_detect.npz"))
SD = synth.to_torch(synth.s3fd_state_dict(42))
TAPS = ("conv1", "pool3", "conv3_3", "conv4_3", "conv5_3", "fc7", "ex1", "ex3")
# sha256 of to_blob(pack_face(...)) of the two RetinaFace synth dicts as the commit before the S3FD detector packed them
R50_BLOB_SHA256 = "a89a2b022033c02e882bbdd6243c6c24bc2d469606383cff632a1ad16d75899b"
MNET_BLOB_SHA256 = "7fa4a7809673eedca1993960cab8f06e3c2471a7546fb134590e23fbaee8f44b"


def _frame(name):
    h, w = (int(v) for v in GOLD[f"{name}_size"])
    return synth.video_frames(900, 1, h, w)[0]


def test_state_dict_has_the_reference_shape_and_is_deterministic():
    a, b = synth.s3fd_state_dict(42), synth.s3fd_state_dict(42)
    assert len(a) == 65 and sum(int(np.size(v)) for v in a.values()) == 22459110
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["vgg.2.weight"], synth.s3fd_state_dict(43)["vgg.2.weight"])
    for name, init in (("L2Norm3_3", 10), ("L2Norm4_3", 8), ("L2Norm5_3", 5)):
        assert 0.8 * init <= a[name + ".weight"].min() and a[name + ".weight"].max() <= 1.2 * init


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_restatement_matches_the_reference_class(name):
    """f32 rounding of the same graph, the project's oracle gate (1e-6), and the reference's own detections at threshold 0.5."""
    taps = {}
    frame = _frame(name)
    loc, conf, fmaps = s3fd_ref.s3fd_forward(SD, s3fd_ref.preprocess(frame), taps)
    np.testing.assert_allclose(conf[0].numpy(), GOLD[f"{name}_conf"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(loc[0].numpy(), GOLD[f"{name}_loc"], rtol=0, atol=1e-6 * max(1.0, float(np.abs(GOLD[f"{name}_loc"]).max())))
    for k in TAPS:
        scale = max(1.0, float(GOLD[f"{name}_{k}_stats"][1]))
        np.testing.assert_allclose(taps[k].reshape(-1)[:16].numpy(), GOLD[f"{name}_{k}_head16"], rtol=0, atol=1e-6 * scale)
        np.testing.assert_allclose(float(taps[k].abs().max()), GOLD[f"{name}_{k}_stats"][1], rtol=1e-6)
    h, w = frame.shape[:2]
    assert fmaps == ft.s3fd_feature_maps(h, w) and conf.shape[1] == s3fd_ref.num_priors(h, w) == {"a": 87, "b": 644, "c": 513}[name]
    dets = s3fd_ref.detect(GOLD[f"{name}_loc"], GOLD[f"{name}_conf"], GOLD[f"{name}_priors"], h, w, 0.5)
    np.testing.assert_array_equal(dets, GOLD[f"{name}_dets"])
    n_cand = int((GOLD[f"{name}_conf"][:, 1] > 0.05).sum())
    assert 0 < n_cand < conf.shape[1] // 4  # the synthetic heads leave a minority of priors above the floor, not all of them


def test_every_launch_is_tapped_and_the_old_names_are_aliases():
    taps, seen = {}, []
    s3fd_ref.s3fd_forward(SD, s3fd_ref.preprocess(_frame("a")), taps, hook=lambda name, t: seen.append(name) or t)
    assert tuple(sorted(seen)) == tuple(sorted(s3fd_ref.LAUNCHES)) and len(s3fd_ref.LAUNCHES) == 24
    assert seen[:3] == ["conv1", "out:vgg2.w", "pool1"] and seen[-1] == "out:ex3.w"
    for old, new in (("conv3_3", "out:vgg14.w"), ("conv4_3", "out:vgg21.w"), ("conv5_3", "out:vgg28.w"), ("fc7", "out:vgg33.w"),
                     ("ex1", "out:ex1.w"), ("ex3", "out:ex3.w")):
        assert taps[old] is taps[new]
    assert len(s3fd_ref.contractions()) == 18 and [c[1] for c in s3fd_ref.contractions()][:4] == ["conv1", "pool1", "out:vgg5.w", "pool2"]
    for i in range(3):
        assert taps[f"l2norm{i}"].shape == taps[("conv3_3", "conv4_3", "conv5_3")[i]].shape
    for i in range(6):
        assert taps[f"head_loc{i}"].shape[-1] == 4 and taps[f"head_conf{i}"].shape[-1] == 2
    # a hook's return value goes on: zeroing pool5 leaves fc6 with its bias alone
    z = {}
    s3fd_ref.s3fd_forward(SD, s3fd_ref.preprocess(_frame("a")), z, hook=lambda name, t: t * 0 if name == "pool5" else t)
    assert torch.equal(z["conv5_3"], taps["conv5_3"]) and not torch.equal(z["fc7"], taps["fc7"])
    want = torch.relu(SD["vgg.31.bias"]).view(1, -1, 1, 1).expand_as(z["out:vgg31.w"])
    assert torch.equal(z["out:vgg31.w"], want)


def test_float32_run_is_within_its_rounding_bound_of_the_float64_run_at_every_tap():
    """One 239 x 431 frame (fc6's map is 7 x 13: its dilated taps read data) through the restatement in float32 and in float64.
    u = 2^-24.
      * Each launch by itself, rigorously: a float32 sum of K products and a bias in ANY order is within (K + 2) u (sum |x||w| + |b|)
        of the exact one, so every contraction of the float32 run is within that of the float64 layer applied to the float32 run's
        own input; conv1 likewise from the integer pixels (K = 27); a pool of float32 values is exact.
      * Against the float64 run, where the launches compound: the worst-case propagation of the bound above multiplies by sum |w|
        per layer (about 80) and says nothing after three layers.  The bound used is the random-walk one: the K_l + 2 roundings of
        an output are independent and at most u of the partial sums, ReLU and max are 1-Lipschitz, and a layer hands relative
        errors on with gain at most 1 (it averages K independent ones), so
            max|err| / max|ref| <= u sqrt(sum over the launches up to this one of (K_l + 2)),
        1.5e-6 behind vgg.2 and 1.3e-5 behind extras.3.  Measured on this frame: 2.9e-7 (vgg.2) .. 9.6e-7 (vgg.28)."""
    u = 2.0 ** -24
    frame = synth.video_frames(239, 1, 239, 431)
    t64, t32 = {}, {}
    l64, c64, _ = s3fd_ref.s3fd_forward64(SD, frame, t64)
    l32, c32, _ = s3fd_ref.s3fd_forward64(SD, frame, t32, dtype=torch.float32)
    assert all(t32[k].dtype == torch.float32 and t64[k].dtype == torch.float64 for k in s3fd_ref.LAUNCHES)
    x0 = s3fd_ref.preprocess(frame[0], False, torch.float64)
    ref, sxw, babs, k0 = s3fd_ref.launch64(SD, s3fd_ref.STEM, x0)
    assert k0 == 27 and bool(((t32["conv1"].double() - ref).abs() <= (k0 + 2) * u * (sxw + babs)).all())
    assert torch.equal(ref, t64["conv1"])  # conv1's input is exact, so this rigorous bound IS its bound against the float64 run
    terms = k0 + 2
    compound = {"conv1": terms}
    for spec in s3fd_ref.contractions():
        name, src = spec[:2]
        if src.startswith("pool"):
            assert torch.equal(t32[src], s3fd_ref.pool64(src, t32[s3fd_ref.POOL_INPUT[src]]))
            compound[src] = terms
        ref, sxw, babs, k = s3fd_ref.launch64(SD, spec, t32[src])
        own = ((t32[name].double() - ref).abs() / ((k + 2) * u * (sxw + babs))).max()
        assert float(own) <= 1.0, (name, float(own))
        terms += k + 2
        compound[name] = terms
    assert set(compound) == set(s3fd_ref.LAUNCHES)
    for name, n_terms in compound.items():
        if name == "conv1":
            continue
        rel = float((t32[name].double() - t64[name]).abs().max() / t64[name].abs().max())
        bound = u * n_terms ** 0.5
        print(f"{name:12s} float32 vs float64 {rel:.2e}  bound {bound:.2e}")
        assert rel <= bound, (name, rel, bound)
    assert float((c32.double() - c64).abs().max()) < 1e-5 and float((l32.double() - l64).abs().max() / l64.abs().max()) < 1e-5


@pytest.mark.parametrize("which", ["full", "trunc"])
def test_detect_restatement_reproduces_the_reference(which):
    h, w = (int(v) for v in DET["size"])
    top = int(DET[f"{which}_nms_top_k"])
    for t in range(4):
        got = s3fd_ref.detect(DET["loc"][t], DET["conf"][t], DET["priors"], h, w, float(DET["threshold"]), nms_top_k=top)
        np.testing.assert_array_equal(got, DET[f"{which}_dets{t}"])
        assert len(got) == DET[f"{which}_counts"][t]
    assert DET["full_counts"][1] == 0 and int((DET["conf"][3, :, 1] > 0.05).sum()) > 64


@pytest.mark.parametrize("name", ec.S_CASES)
def test_detect_restatement_on_non_finite_degenerate_and_boundary_cases(name):
    """tests/golden/detect_edges.npz: Detect and the predictor's loop on NaN / inf scores, NaN boxes, a box whose area overflows,
    zero-size and inverted boxes (S3FD's areas have no "+1": 0 / 0 between two zero-size twins), an overlap exactly on nms_thresh and
    scores exactly on the two thresholds.  The boxes are dyadic, so the rows are exact: float32 reproduces every case bit for bit, and
    float64 does where nothing ties and nothing sits on a comparison."""
    kind, loc, conf, priors, size, par, want = ec.s3fd_case(name)
    assert kind in ("plain", "boundary", "tie_rule") and par["nms_top_k"] <= 6144 and par["top_k"] <= 1024
    assert all(ec.same_bits(g, w) for g, w in zip(ec.s3fd_oracle(name, np.float32), want))
    if kind == "plain":
        assert all(ec.same_bits(g, w) for g, w in zip(ec.s3fd_oracle(name, np.float64), want))


@pytest.mark.parametrize("variant", ec.B_VARIANTS)
def test_detect_restatement_on_overflowing_decodes(variant):
    E = ec.E
    h, w = (int(v) for v in E["sb_size"])
    want = E[f"sb_rows_{variant}"]
    got = s3fd_ref.detect(E["sb_loc"], E[f"sb_conf_{variant}"], E["sb_priors"], h, w, float(E["sb_threshold"]))
    assert ec.same_bits(got, want)   # (float64 is no yardstick here: e^100 is finite in it, and the NaN corner never appears)


def test_prior_boxes_equal_the_reference_bit_for_bit():
    for name in ("a", "b", "c"):
        got = ft.s3fd_prior_boxes(tuple(int(v) for v in GOLD[f"{name}_size"]))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, GOLD[f"{name}_priors"])
    np.testing.assert_array_equal(ft.s3fd_prior_boxes((77, 101)), DET["priors"])


def test_num_priors_rule():
    lib = ctypes.CDLL(build.build())
    lib.avcer_s3fd_num_priors.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.avcer_s3fd_num_priors.restype = ctypes.c_int
    for (h, w), want in (((32, 32), 87), ((75, 101), 600), ((65, 97), 513), ((360, 640), 19175), ((77, 101), 644)):
        assert lib.avcer_s3fd_num_priors(h, w) == want
        assert s3fd_ref.num_priors(h, w) == want
        assert sum(a * b for a, b in ft.s3fd_feature_maps(h, w)) == want == len(ft.s3fd_prior_boxes((h, w)))
    assert lib.avcer_s3fd_num_priors(0, 5) == 0


def test_face_kind_tells_the_three_detectors_apart():
    dicts = ((synth.retina_state_dict(42), 1), (synth.retina_mnet_state_dict(42), 2), (synth.s3fd_state_dict(42), 3))
    for sd, kind in dicts:
        assert packing.face_kind(sd) == kind
        assert packing.face_kind({"module." + k: v for k, v in sd.items()}) == kind
    assert (packing.FACE_KIND_R50, packing.FACE_KIND_MNET, packing.FACE_KIND_S3FD) == (1, 2, 3)
    with pytest.raises(ValueError):
        packing.face_kind({"vgg.0.weight": np.zeros((64, 3, 3, 3), np.float32)})  # no L2Norm: not an S3FD dict


def test_the_retinaface_blobs_are_byte_identical():
    for sd, sha in ((synth.retina_state_dict(42), R50_BLOB_SHA256), (synth.retina_mnet_state_dict(42), MNET_BLOB_SHA256)):
        assert hashlib.sha256(packing.to_blob(packing.pack_face(sd))).hexdigest() == sha


def test_pack_face_s3fd_records_the_kind_and_accepts_the_checkpoint_spellings():
    sd = synth.s3fd_state_dict(42)
    pk = packing.pack_face(sd)
    assert float(pk["s3fd.kind"][0]) == 3.0 and "mnet.kind" not in pk
    want = packing.to_blob(pk)
    assert packing.to_blob(packing.pack_face({"module." + k: v for k, v in sd.items()})) == want
    assert packing.to_blob(packing.pack_face(SD)) == want  # torch tensors
    # every contraction of the trunk has the shape the library's split copies exist for
    for k, v in pk.items():
        if k.endswith(".w"):
            assert v.ndim == 2 and v.shape[0] % 64 == 0 and v.shape[1] % 32 == 0, (k, v.shape)


def _head_kernel64(x_nhwc, wt, b, l2):
    """What s3fd_head_kernel computes from the PACKED tensors, in float64 numpy: every tap times its position's inverse norm (the
    L2Norm weight is already in `wt`), the [9][c][n_out] layout, bias, level 0's max-out, the softmax."""
    n, h, w, c = x_nhwc.shape
    no = wt.shape[2]
    x = x_nhwc.astype(np.float64)
    if l2:
        x = x * (1.0 / (np.sqrt((x * x).sum(-1, keepdims=True)) + 1e-10))
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((n, h, w, no)) + b.astype(np.float64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + w] @ wt[ky * 3 + kx].astype(np.float64)
    loc, cf = out[..., :4], out[..., 4:]
    if no == 8:
        cf = np.stack([cf[..., :3].max(-1), cf[..., 3]], -1)
    e = np.exp(cf - cf.max(-1, keepdims=True))
    return loc.reshape(n, -1, 4), (e / e.sum(-1, keepdims=True)).reshape(n, -1, 2)


def test_packed_heads_reproduce_the_restatement_in_float64():
    """L2Norm folded into the heads' input-channel axis, loc and conf merged, the head kernel's layout: evaluated in float64 numpy
    on the restatement's own float64 head inputs, equal to its head outputs at float64 rounding (the fold re-associates one product
    per channel and is stored as f32: 6e-8 relative per weight)."""
    pk = packing.pack_face(synth.s3fd_state_dict(42))
    sd64 = {k: v.double() for k, v in SD.items()}
    taps = {}
    x = s3fd_ref.preprocess(_frame("b"), False, torch.float64)
    want_loc, want_conf, fmaps = s3fd_ref.s3fd_forward(sd64, x, taps)
    raw = [taps["conv3_3"], taps["conv4_3"], taps["conv5_3"], taps["fc7"], taps["ex1"], taps["ex3"]]
    row0 = 0
    for i, src in enumerate(raw):
        wt = pk[f"head{i}.wt"]
        assert wt.shape == (9, src.shape[1], 8 if i == 0 else 6) and wt.dtype == np.float32
        loc, conf = _head_kernel64(src.permute(0, 2, 3, 1).numpy(), wt, pk[f"head{i}.b"], i < 3)
        rows = slice(row0, row0 + fmaps[i][0] * fmaps[i][1])
        assert np.abs(loc[0] - want_loc[0, rows].numpy()).max() < 2e-6 * max(1.0, float(want_loc.abs().max()))
        assert np.abs(conf[0] - want_conf[0, rows].numpy()).max() < 2e-6
        row0 = rows.stop
    assert row0 == want_loc.shape[1]


def test_abi_and_symbols():
    header = open(os.path.join(HERE, "..", "include", "avcer_hip.h")).read()
    assert re.search(r"#define AVCER_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    lib = build.build()
    defined = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in ("avcer_s3fd_num_priors", "avcer_s3fd_detect", "avcer_s3fd_stem", "avcer_maxpool2", "avcer_s3fd_head"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\b{name}\b", defined), name
    assert "s3fd.hip" in build.SOURCES


def test_s3fd_kernels_use_no_scratch_and_do_not_spill():
    """Every kernel of s3fd.hip and of detect_tail.hip (Detect, with RetinaFace's tail), and the detector's 2 x 2 pool, which is the
    shared maxpool_kernel of kernels.hip (all of its instances)."""
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        pytest.skip("hipcc not available")
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
    # s3fd.hip: stem and inverse norm x two storages, the head x two storages x 8 / 6 outputs; detect_tail.hip: decode, order and NMS
    # x two detectors and RetinaFace's counting kernel; kernels.hip: the pool, 2 x 2 on f32 / sp32 and 3 x 3 on f32 / bf16
    bad = []
    for src, only, count in (("s3fd.hip", "", 2 + 2 + 4), ("detect_tail.hip", "", 3 * 2 + 1), ("kernels.hip", "maxpool_kernel", 2 + 2)):
        out = os.path.join(tempfile.mkdtemp(prefix="avcer_asm_"), src + ".s")
        r = subprocess.run([exe] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, src)],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        kernels = re.findall(r"- \.agpr_count:.*?\.wavefront_size", open(out).read(), re.S)
        g = lambda k, key: re.search(r"\." + key + r":\s+(\S+)", k).group(1)
        kernels = [k for k in kernels if only in g(k, "name")]
        assert len(kernels) == count, (src, [g(k, "name") for k in kernels])
        for k in kernels:
            if int(g(k, "private_segment_fixed_size")) or int(g(k, "vgpr_spill_count")) or int(g(k, "sgpr_spill_count")):
                bad.append((g(k, "name"), g(k, "private_segment_fixed_size"), g(k, "vgpr_spill_count"), g(k, "sgpr_spill_count")))
    assert not bad, bad
