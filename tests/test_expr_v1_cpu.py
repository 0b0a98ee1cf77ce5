"""The GRU-head audio model ExprModelV1 without a GPU: the CPU restatement (tests/expr_v1_oracle.py) against vectors of the
reference's own model (tests/golden/audio_model_v1.npz, made by tests/golden/make_golden_v1.py), the synthetic weights'
recurrence condition, the V1 packing, and the C ABI of the new entry points."""
import ctypes
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_v1_oracle as v1  # noqa: E402
from avcer_amd import packing, synth  # noqa: E402
from oracle import audio as oa  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(t):
    t = t.detach().float()
    return np.array([t.mean().item(), t.abs().max().item(), t.std().item()])


@pytest.fixture(scope="module")
def sd_v1():
    return synth.to_torch(synth.audio_v1_state_dict(44))


@pytest.fixture(scope="module")
def window0(sd_v1):
    """The fixture's first 2 s window through the oracle: (trunk output [1,99,1024], GRU output [1,99,256])."""
    x = oa.normalize(synth.waveforms(6678, 2, 32000))[:1]
    with torch.no_grad():
        w = oa.wav2vec2_forward(sd_v1, torch.from_numpy(x))
        return w, v1.gru(sd_v1, w)


# ---- oracle against the reference (the bounds tests/test_oracle_audio.py applies to ExprModelV3)
@pytest.mark.parametrize("tag,seed,b,t", [("t32000", 6678, 2, 32000), ("t64000", 6679, 1, 64000)])
def test_oracle_matches_reference(golden, sd_v1, tag, seed, b, t):
    g = golden("audio_model_v1")
    x = oa.normalize(synth.waveforms(seed, b, t))
    taps = {}
    with torch.no_grad():
        lg = v1.expr_model_v1_forward(sd_v1, torch.from_numpy(x), taps)
    assert tuple(lg.shape) == tuple(g[f"{tag}_logits"].shape)  # (8,) at batch 1: `.squeeze()`
    got = {"w2v": taps["w2v"], "gru": taps["gru2"], "time_downsample": taps["pooled"][:, :, None]}
    for k, v in got.items():
        assert tuple(v.shape) == tuple(g[f"{tag}_{k}_shape"]), k
        np.testing.assert_allclose(v.reshape(-1)[:16].numpy(), g[f"{tag}_{k}_head16"], rtol=2e-4, atol=2e-5, err_msg=k)
        np.testing.assert_allclose(_stats(v), g[f"{tag}_{k}_stats"], rtol=1e-4, atol=1e-6, err_msg=k)
    err = np.abs(lg.numpy() - g[f"{tag}_logits"]).max()
    assert err < 2e-5, err
    np.testing.assert_allclose(taps["pooled"].squeeze().numpy(), g[f"{tag}_features"], rtol=2e-4, atol=2e-5)
    if tag == "t32000":
        np.testing.assert_allclose(taps["gru2"][0].numpy(), g["t32000_gru_window0"], rtol=2e-4, atol=2e-5)


def test_oracle_matches_reference_seven_classes(golden):
    g = golden("audio_model_v1")
    sd = synth.to_torch(synth.audio_v1_state_dict(45, 7))
    with torch.no_grad():
        lg = v1.expr_model_v1_forward(sd, torch.from_numpy(oa.normalize(synth.waveforms(6680, 2, 32000))))
    assert tuple(lg.shape) == (2, 7)
    err = np.abs(lg.numpy() - g["c7_t32000_logits"]).max()
    assert err < 2e-5, err


def test_one_row_call_returns_a_vector(golden, sd_v1):
    g = golden("audio_model_v1")
    assert tuple(g["t32000_one_row_shape"]) == (8,)
    with torch.no_grad():
        lg = v1.expr_model_v1_forward(sd_v1, torch.from_numpy(oa.normalize(synth.waveforms(6678, 2, 32000))[:1]))
    assert tuple(lg.shape) == (8,)
    assert np.abs(lg.numpy() - g["t32000_logits"][0]).max() < 2e-5


def test_float64_form_agrees(sd_v1):
    wav = synth.waveforms(6678, 2, 32000)[:1]
    with torch.no_grad():
        lg32 = v1.expr_model_v1_forward(sd_v1, torch.from_numpy(oa.normalize(wav)))
    lg64 = v1.expr_model_v1_forward64(oa.state_dict64(sd_v1), wav)
    assert lg64.dtype == torch.float64 and np.abs(lg64.numpy() - lg32.numpy()).max() < 2e-5


def test_gru_restatement_is_torch_gru(sd_v1, window0):
    """The gate-by-gate restatement against torch.nn.GRU itself on the fixture window."""
    w, got = window0
    ref = torch.nn.GRU(1024, 256, num_layers=2, batch_first=True)
    ref.load_state_dict({k[4:]: v for k, v in sd_v1.items() if k.startswith("gru.")}, strict=True)
    with torch.no_grad():
        want = ref.eval()(w)[0]
    assert np.abs(got.numpy() - want.numpy()).max() < 2e-6


# ---- the recurrence is exercised by the synthetic weights (a condition on them, not a tolerance)
def test_recurrent_term_carries_weight(sd_v1, window0):
    w, real = window0
    sd0 = dict(sd_v1)
    for l in (0, 1):
        sd0[f"gru.weight_hh_l{l}"] = torch.zeros_like(sd_v1[f"gru.weight_hh_l{l}"])
    with torch.no_grad():
        cut = v1.gru(sd0, w)
    d = (real - cut).abs().max().item()
    assert d >= 0.05, d


def test_token_order_matters(sd_v1, window0):
    w, real = window0
    with torch.no_grad():
        rev = v1.gru(sd_v1, torch.flip(w, dims=[1]))
    d = (real[:, -1] - rev[:, -1]).abs().max().item()
    assert d > 1e-3, d


# ---- packing
V1_HEAD = OrderedDict([
    ("gru1.wih.w", (768, 1024)), ("gru1.wih.b", (768,)), ("gru1.whh.w", (768, 256)), ("gru1.whh.b", (768,)),
    ("gru2.wih.w", (768, 256)), ("gru2.wih.b", (768,)), ("gru2.whh.w", (768, 256)), ("gru2.whh.b", (768,)),
    ("td0.w", (256, 1280)), ("td0.s", (256,)), ("td0.b", (256,)), ("td4.w", (256, 768)), ("td4.s", (256,)), ("td4.b", (256,)),
    ("fd.w", (8, 256)), ("fd.b", (8,))])


def _is_trunk(name):
    return name.startswith(("fe", "fp.", "pos.", "enc"))


def test_v1_pack_names_and_shapes():
    sd = synth.audio_v1_state_dict(44)
    p = packing.pack_audio(sd)
    p3 = packing.pack_audio(synth.audio_state_dict(44))
    trunk = [k for k in p3 if _is_trunk(k)]
    assert list(p) == trunk + list(V1_HEAD)
    for k in trunk:  # the same trunk, bit for bit, at the same seed
        assert p[k].shape == p3[k].shape and p[k].tobytes() == p3[k].tobytes(), k
    for k, shape in V1_HEAD.items():
        assert p[k].shape == shape and p[k].dtype == np.float32, k
    np.testing.assert_array_equal(p["gru1.wih.b"], sd["gru.bias_ih_l0"])
    np.testing.assert_array_equal(p["gru2.whh.b"], sd["gru.bias_hh_l1"])
    np.testing.assert_array_equal(p["gru2.whh.w"], sd["gru.weight_hh_l1"])
    p7 = packing.pack_audio(synth.audio_v1_state_dict(45, 7))
    assert p7["fd.w"].shape == (7, 256) and p7["fd.b"].shape == (7,)


def test_checkpoint_spellings_pack_to_the_same_bytes():
    sd = synth.audio_v1_state_dict(44)
    want = packing.to_blob(packing.pack_audio(sd))
    assert packing.to_blob(packing.pack_audio({"epoch": 3, "model_state_dict": sd})) == want
    assert packing.to_blob(packing.pack_audio(OrderedDict(("module." + k, v) for k, v in sd.items()))) == want
    assert packing.to_blob(packing.pack_audio(synth.to_torch(sd))) == want


def test_v3_pack_is_unchanged():
    """The V3 layout tensor by tensor: names, order and bytes as before the GRU head existed (the list is the parent's)."""
    sd = synth.audio_state_dict(42)
    p = packing.pack_audio(sd)
    names = [k for k in p if not _is_trunk(k)]
    tl = [f"tl{l}.{s}" for l in (1, 2) for s in ("qkv.w", "o.w", "ln1.g", "ln1.b", "ff1.w", "ff1.b", "ff2.w", "ff2.b", "ln2.g", "ln2.b")]
    assert names == ["pe"] + tl + ["td0.w", "td0.s", "td0.b", "td4.w", "td4.s", "td4.b", "fd.w", "fd.b"]
    assert len(p) == 7 * 4 + 4 + 2 + 12 * 12 + 2 + len(names)
    np.testing.assert_array_equal(p["tl1.qkv.w"], np.concatenate([sd[f"tl1.self_attention.{n}.weight"] for n in ("query_w", "keys_w", "values_w")]))
    np.testing.assert_array_equal(p["tl2.ff2.b"], sd["tl2.feed_forward.layer_2.bias"])
    np.testing.assert_array_equal(p["td0.w"], sd["time_downsample.0.weight"].transpose(0, 2, 1).reshape(1024, -1))
    np.testing.assert_array_equal(p["td4.w"], sd["time_downsample.4.weight"].transpose(0, 2, 1).reshape(1024, -1))
    s0, b0 = packing._bn_fold(sd, "time_downsample.1", packing.AUDIO_BN_EPS, sd["time_downsample.0.bias"])
    assert p["td0.s"].tobytes() == s0.tobytes() and p["td0.b"].tobytes() == b0.tobytes()
    np.testing.assert_array_equal(p["fd.w"], sd["feature_downsample.weight"])
    np.testing.assert_array_equal(p["enc11.ff2.w"], sd["wav2vec2.encoder.layers.11.feed_forward.output_dense.weight"])
    assert p["pe"].shape == (packing.PE_ROWS, 1024)
    assert all(v.dtype == np.float32 for v in p.values())
    # and the whole blob: its SHA-256 as the commit before the GRU head packed it
    import hashlib
    assert hashlib.sha256(packing.to_blob(p)).hexdigest() == "06ddc4fff330e17a7f50c3c4fdd3f0bf6e6901e69d85a989c04fe07c532f09d8"


def test_headless_state_dict_is_refused():
    sd = OrderedDict((k, v) for k, v in synth.audio_v1_state_dict(44).items() if not k.startswith("gru."))
    with pytest.raises(KeyError, match="neither a GRU head"):
        packing.pack_audio(sd)
    both = synth.audio_state_dict(42)
    both["gru.weight_ih_l0"] = np.zeros((768, 1024), np.float32)
    with pytest.raises(KeyError, match="both"):
        packing.pack_audio(both)


# ---- ABI
def test_abi_8_and_new_symbols():
    from avcer_amd import _lib, build

    build.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avcer_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.LIB)
    assert int(re.search(r"#define AVCER_ABI_VERSION (\d+)", header).group(1)) == lib.avcer_abi_version() == _lib.ABI_VERSION == 8
    for name in ("avcer_audio_head_kind", "avcer_audio_forward_features", "avcer_gru_layer"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["avcer_audio_forward_features"][1]) == len(_lib.SIGNATURES["avcer_audio_forward"][1]) + 1
    assert len(_lib.SIGNATURES["avcer_gru_layer"][1]) == 10
    assert re.search(r"AVCER_FAM_GRU\s*=\s*6", header) and re.search(r"AVCER_FAM_COUNT\s*=\s*7", header)
    lib.avcer_audio_head_kind.restype = ctypes.c_int
    lib.avcer_audio_head_kind.argtypes = [ctypes.c_void_p]
    assert lib.avcer_audio_head_kind(None) == 0
