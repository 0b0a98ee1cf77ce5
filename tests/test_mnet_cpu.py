"""The MobileNet-0.25 RetinaFace detector on the CPU: the restatement against the reference's own outputs, the packing, the ABI and
the build hygiene of csrc/mnet.hip."""
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mnet_ref
from avcer_amd import _lib, build, packing, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "face_net_mnet.npz"))
SD = synth.to_torch(synth.retina_mnet_state_dict(42))
# sha256 of to_blob(pack_face(retina_state_dict(42))) as the commit before the MobileNet variant packed it
R50_BLOB_SHA256 = "a89a2b022033c02e882bbdd6243c6c24bc2d469606383cff632a1ad16d75899b"


def _frame(name):
    h, w = (int(v) for v in GOLD[f"{name}_size"])
    return synth.video_frames(900, 1, h, w)[0]


def test_state_dict_has_the_reference_shape():
    sd = synth.retina_mnet_state_dict(42)
    assert len(sd) == 300 and sum(int(np.size(v)) for v in sd.values()) == 433343


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_restatement_matches_the_reference_class(name):
    """f32 rounding of the same graph: the gate of test_oracle_retina.py."""
    taps = {}
    loc, conf, lm = mnet_ref.mnet_forward(SD, mnet_ref.preprocess(_frame(name)), taps)
    for got, key in ((loc, "loc"), (conf, "conf"), (lm, "landms")):
        np.testing.assert_allclose(got[0].numpy(), GOLD[f"{name}_{key}"], rtol=0, atol=2e-5)
    for k in ("body1", "body2", "body3", "fpn1", "fpn2", "fpn3", "ssh1"):
        np.testing.assert_allclose(taps[k].reshape(-1)[:16].numpy(), GOLD[f"{name}_{k}_head16"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(float(taps[k].abs().max()), GOLD[f"{name}_{k}_stats"][1], rtol=1e-5)
    assert conf.shape[1] == {"a": 504, "b": 354, "c": 86}[name]


def test_pack_face_detects_the_kind_and_records_it():
    mn = packing.pack_face(synth.retina_mnet_state_dict(42))
    assert packing.face_kind(synth.retina_mnet_state_dict(42)) == 2 and float(mn["mnet.kind"][0]) == 2.0
    r50 = synth.retina_state_dict(42)
    assert packing.face_kind(r50) == 1
    blob = packing.to_blob(packing.pack_face(r50))
    assert hashlib.sha256(blob).hexdigest() == R50_BLOB_SHA256  # the R50 path packs the bytes it always did
    assert b"mnet.kind" not in blob[:200000]
    with pytest.raises(ValueError):
        packing.pack_face({"fpn.output1.0.weight": np.zeros((64, 64, 1, 1), np.float32)})


def test_pack_face_mnet_accepts_the_checkpoint_spellings():
    sd = synth.retina_mnet_state_dict(42)
    want = packing.to_blob(packing.pack_face(sd))
    assert packing.to_blob(packing.pack_face({"module." + k: v for k, v in sd.items()})) == want
    assert packing.to_blob(packing.pack_face({"state_dict": sd})) == want
    assert packing.to_blob(packing.pack_face({"state_dict": {"module." + k: v for k, v in sd.items()}})) == want
    assert packing.to_blob(packing.pack_face(SD)) == want  # torch tensors


def _packed_forward64(pk, x):
    """The network evaluated from the PACKED tensors alone, in float64, the way csrc/mnet.hip reads them: folded BatchNorm, tap-major
    depthwise weights, zero-padded pointwise matrices, transposed neck weights, SSH branches stored at channel offsets 0 / 32 / 48 of
    one 64-channel tensor, the three heads of a level as one 32-column matrix."""
    t = {k: torch.from_numpy(np.asarray(v)).double() for k, v in pk.items()}
    leaky = lambda v: F.leaky_relu(v, 0.1)
    aff = lambda v, p: v * t[p + "s"].view(1, -1, 1, 1) + t[p + "b"].view(1, -1, 1, 1)

    def conv_t(p, v, ks, act):
        wt = t[p + "wt"]  # [ks*ks*cin, cout]
        w = wt.view(ks, ks, v.shape[1], -1).permute(3, 2, 0, 1)
        y = aff(F.conv2d(v, w, padding=ks // 2), p)
        return leaky(y) if act == 4 else (F.relu(y) if act == 1 else y)

    x = leaky(aff(F.conv2d(x, t["stem.wt"].view(3, 3, 3, 8).permute(3, 2, 0, 1), stride=2, padding=1), "stem."))
    feats = []
    for i, (cin, cout, s) in enumerate(packing.MNET_BLOCKS, start=1):
        p = f"b{i}."
        dw = t[p + "dw.w"].T.reshape(cin, 1, 3, 3)
        y = leaky(aff(F.conv2d(x, dw, stride=s, padding=1, groups=cin), p + "dw."))
        pw = t[p + "pw.w"]
        assert pw.shape == ((cout + 63) // 64 * 64, (cin + 31) // 32 * 32)
        assert not pw[cout:].any() and not pw[:, cin:].any()  # the padding is exact zeros: it adds nothing to any sum
        ypad = F.pad(y, (0, 0, 0, 0, 0, pw.shape[1] - cin))    # the kernel's zero-padded contraction
        x = leaky(aff(F.conv2d(ypad, pw.view(*pw.shape, 1, 1))[:, :cout], p + "pw."))
        if i in (5, 11, 13):
            feats.append(x)
    o = [conv_t(f"fpn.o{i + 1}.", f, 1, 4) for i, f in enumerate(feats)]
    m2 = conv_t("fpn.m2.", o[1] + F.interpolate(o[2], size=o[1].shape[2:], mode="nearest"), 3, 4)
    m1 = conv_t("fpn.m1.", o[0] + F.interpolate(m2, size=o[0].shape[2:], mode="nearest"), 3, 4)
    loc, conf, lm = [], [], []
    for i, v in enumerate((m1, m2, o[2])):
        p = f"ssh{i + 1}."
        S = torch.zeros(v.shape[0], 64, *v.shape[2:], dtype=torch.float64)
        t51 = conv_t(p + "c51.", v, 3, 4)
        S[:, 0:32] = conv_t(p + "c3.", v, 3, 1)
        S[:, 32:48] = conv_t(p + "c52.", t51, 3, 1)
        S[:, 48:64] = conv_t(p + "c73.", conv_t(p + "c72.", t51, 3, 4), 3, 1)
        hd = torch.einsum("nchw,co->nhwo", S, t[f"head{i}.wt"]) + t[f"head{i}.b"]
        n = hd.shape[0]
        conf.append(hd[..., 0:4].reshape(n, -1, 2))
        loc.append(hd[..., 4:12].reshape(n, -1, 4))
        lm.append(hd[..., 12:32].reshape(n, -1, 10))
    return torch.cat(loc, 1), F.softmax(torch.cat(conf, 1), dim=-1), torch.cat(lm, 1)


def test_packed_network_equals_the_unpacked_one_in_float64():
    """The neck of this variant runs as direct convolutions of its true widths (32 / 16 / 16), so nothing of it is padded; what the
    packing does change -- the BatchNorm fold, the layouts, the zero padding of the pointwise matrices, the merged heads and the
    concatenation offsets -- is evaluated here in float64 against the restatement: equal to float64 rounding (the fold re-associates
    one product per channel), with the padding checked to be exact zeros."""
    pk = packing.pack_face(synth.retina_mnet_state_dict(42))
    fr = _frame("b")
    want = mnet_ref.mnet_forward64(SD, fr)
    got = _packed_forward64(pk, mnet_ref.preprocess(fr, torch.float64))
    for g, w in zip(got, want):
        # the packed scales are f32 roundings of the folded BatchNorm (as in every other model of the library): 6e-8 relative
        assert float((g - w).abs().max()) < 5e-6 * max(1.0, float(w.abs().max()))


def test_abi_and_symbols():
    header = open(os.path.join(HERE, "..", "include", "avcer_hip.h")).read()
    assert re.search(r"#define AVCER_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    lib = build.build()
    defined = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    for name in ("avcer_face_kind", "avcer_dwsep"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\b{name}\b", defined), name
    assert "mnet.hip" in build.SOURCES


def test_face_kind_of_a_null_context_is_zero():
    import ctypes

    lib = ctypes.CDLL(build.build())
    lib.avcer_face_kind.argtypes = [ctypes.c_void_p]
    lib.avcer_face_kind.restype = ctypes.c_int
    assert lib.avcer_face_kind(None) == 0


# ---- build hygiene of mnet.hip: the two scans tests/test_build_hygiene.py applies to the other sources, restated
@pytest.fixture(scope="module")
def mnet_asm():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        pytest.skip("hipcc not available")
    out = os.path.join(tempfile.mkdtemp(prefix="avcer_asm_"), "mnet.hip.s")
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
    r = subprocess.run([exe] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "mnet.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def test_mnet_kernels_use_no_scratch_and_do_not_spill(mnet_asm):
    kernels = re.findall(r"- \.agpr_count:.*?\.wavefront_size", mnet_asm, re.S)
    assert len(kernels) == 9 * 2 + 1 + 2  # nine block shapes x two modes, the stem, the neck at 1x1 and 3x3
    bad = []
    for k in kernels:
        g = lambda key: re.search(r"\." + key + r":\s+(\S+)", k).group(1)
        if int(g("private_segment_fixed_size")) or int(g("vgpr_spill_count")) or int(g("sgpr_spill_count")):
            bad.append((g("name"), g("private_segment_fixed_size"), g("vgpr_spill_count"), g("sgpr_spill_count")))
    assert not bad, bad


def test_mnet_has_no_valu_write_right_behind_a_wide_buffer_store(mnet_asm):
    bad, kernel, prev = [], "?", None
    for line in mnet_asm.splitlines():
        t = line.strip()
        if not t or t.startswith((";", ".")):
            continue
        if t.endswith(":") and not t.startswith(".L"):
            kernel, prev = t[:-1], None
            continue
        if prev is not None and t.startswith("v_"):
            m = re.match(r"v_\w+\s+(v\[(\d+):(\d+)\]|v(\d+))", t)
            if m:
                lo, hi = (int(m.group(2)), int(m.group(3))) if m.group(2) else (int(m.group(4)), int(m.group(4)))
                if lo <= prev[1] and hi >= prev[0]:
                    bad.append((kernel, prev[2], t))
        prev = None
        m = re.match(r"buffer_store_dwordx[34]\s+v\[(\d+):(\d+)\]", t)
        if m:
            prev = (int(m.group(1)), int(m.group(2)), t)
    assert bad == []


def test_mnet_uses_no_inline_asm_loads():
    src = open(os.path.join(build.CSRC, "mnet.hip")).read()
    assert "asm" not in src.replace("asm volatile(\"\"", "")  # split_dev.h's empty asm (sp_value) is the only one it reaches
