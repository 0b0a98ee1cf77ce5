"""Audio windows longer than 256 tokens without a GPU: the oracle (oracle/audio.py, tests/expr_v1_oracle.py) against the reference's
own ExprModelV3 and ExprModelV1 at 257 and 400 tokens (tests/golden/audio_long.npz, made by tests/golden/make_golden_audio_long.py),
the `pe_rows` argument of packing.pack_audio, the token arithmetic of a window and the early refusal of the host entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_v1_oracle as v1  # noqa: E402
from avcer_amd import audio_pipeline, packing, synth  # noqa: E402
from avcer_amd import dataset as adataset  # noqa: E402
from avcer_amd import run as arun  # noqa: E402
from oracle import audio as oa  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = ((82320, 257), (128080, 400))  # make_golden_audio_long.py
SEEDS = {"v3": (42, 7701), "v1": (44, 7801)}


@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("tag", ["v3", "v1"])
def test_oracle_reproduces_the_reference_past_256_tokens(golden, tag, li):
    g = golden("audio_long")
    t, tokens = LENGTHS[li]
    x = torch.from_numpy(oa.normalize(synth.waveforms(SEEDS[tag][1] + li, 2, t)))
    taps = {}
    with torch.no_grad():
        if tag == "v3":
            lg = oa.expr_model_v3_forward(synth.to_torch(synth.audio_state_dict(SEEDS[tag][0])), x, taps)
            got = {"w2v": taps["w2v"], "tl2": taps["tl2"]}
        else:
            lg = v1.expr_model_v1_forward(synth.to_torch(synth.audio_v1_state_dict(SEEDS[tag][0])), x, taps)
            got = {"w2v": taps["w2v"], "gru": taps["gru2"]}
    key = f"{tag}_t{t}"
    err = np.abs(lg.numpy() - g[f"{key}_logits"]).max()
    print(key, "max|dlogit| against the reference", err)
    assert tuple(lg.shape) == (2, 8) and err <= 1e-6, err
    for k, v in got.items():
        assert tuple(v.shape) == tuple(g[f"{key}_{k}_shape"]) and v.shape[1] == tokens, k
        assert np.abs(v.reshape(-1)[:16].numpy() - g[f"{key}_{k}_head16"]).max() <= 1e-6, k
        assert abs(v.abs().max().item() - float(g[f"{key}_{k}_absmax"])) <= 1e-6 * max(1.0, float(g[f"{key}_{k}_absmax"])), k


def test_pack_audio_pe_rows():
    sd = synth.audio_state_dict(42)
    p = packing.pack_audio(sd)
    assert p["pe"].shape == (packing.PE_ROWS, 1024) == (256, 1024)
    p1k = packing.pack_audio(sd, pe_rows=1024)
    assert p1k["pe"].shape == (1024, 1024) and list(p1k) == list(p)
    assert p1k["pe"][:256].tobytes() == p["pe"].tobytes()
    np.testing.assert_array_equal(p1k["pe"], sd["tl1.positional_encoding.pe"].reshape(-1, 1024)[:1024])
    for k in p:
        if k != "pe":
            assert p[k].tobytes() == p1k[k].tobytes(), k
    assert packing.pack_audio(sd, pe_rows=5000)["pe"].shape == (5000, 1024)
    for bad in (255, 5001, 0, 300.0, True):
        with pytest.raises(ValueError, match="pe_rows"):
            packing.pack_audio(sd, pe_rows=bad)
    # the GRU head has no positional buffer: the argument changes nothing
    sd1 = synth.audio_v1_state_dict(44)
    assert packing.to_blob(packing.pack_audio(sd1, pe_rows=1024)) == packing.to_blob(packing.pack_audio(sd1))


def test_window_tokens():
    """The extractor's seven convolutions: one token per 320 samples from 400 on"""
    assert [audio_pipeline.window_tokens(t) for t in (0, 399, 400, 719, 720, 16399, 16400, 32000, 64000, 82000, 82319, 82320, 128080)] == \
        [0, 0, 1, 1, 2, 50, 51, 99, 199, 256, 256, 257, 400]
    assert audio_pipeline.window_tokens(8 * 16000) == 399 and audio_pipeline.window_tokens(100 * 16000) == 4999
    assert audio_pipeline.window_tokens(5000 * 320 + 80) == 5000
    # the oracle's extractor agrees
    x = torch.zeros(1, 82320)
    with torch.no_grad():
        assert oa.feature_extractor(synth.to_torch(synth.audio_state_dict(42)), x).shape[1] == 257


class _Engine:
    """Stands in for an Engine whose loaded audio model accepts `limit` tokens; anything else it is asked for is work."""

    def __init__(self, limit):
        self.audio_max_tokens = limit

    def __getattr__(self, name):
        raise AssertionError(f"work was started: Engine.{name}")


def test_host_entry_points_refuse_a_long_window_before_any_work(tmp_path):
    eng = _Engine(256)
    wav = torch.zeros(16000 * 12)
    with pytest.raises(ValueError, match="max_tokens"):
        audio_pipeline.audio_forward(eng, wav, window=8)
    import wave

    with wave.open(str(tmp_path / "clip.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(b"\0\0" * 1600)
    with pytest.raises(ValueError, match="max_tokens"):
        audio_pipeline.preprocess_audio_and_predict(eng, str(tmp_path / "clip.mp4"), window=8)  # the WAV exists; nothing is read
    with pytest.raises(ValueError, match="max_tokens"):
        arun.run_inference(eng, np.zeros((4, 8, 8, 3), np.uint8), wav.numpy(), 25, detections=[np.zeros((0, 5))] * 4, window=8)
    with pytest.raises(ValueError, match="max_tokens"):
        adataset.run_dataset(eng, [], window=8)
    assert audio_pipeline.check_window(_Engine(399), 8, 16000) == 399
    with pytest.raises(ValueError, match="399 tokens.*max_tokens=398"):
        audio_pipeline.check_window(_Engine(398), 8, 16000)
    assert audio_pipeline.check_window(eng, 4, 16000) == 199 and audio_pipeline.check_window(eng, 5.125, 16000) == 256


def test_abi_symbols_of_the_long_path():
    from avcer_amd import _lib, build

    build.build()
    text = open(os.path.join(ROOT, "include", "avcer_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(build.LIB)
    assert lib.avcer_abi_version() == _lib.ABI_VERSION == 8
    for name in ("avcer_attention_long", "avcer_set_audio_max_tokens", "avcer_audio_max_tokens"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["avcer_attention_long"][1] == _lib.SIGNATURES["avcer_attention"][1]
    assert int(re.search(r"#define AVCER_AUDIO_MAX_TOKENS (\d+)", header).group(1)) == packing.PE_ROWS_MAX == 5000
    lib.avcer_audio_max_tokens.argtypes = [ctypes.c_void_p]
    assert lib.avcer_audio_max_tokens(None) == 0
    lib.avcer_set_audio_max_tokens.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.avcer_set_audio_max_tokens(None, 1024) != 0
