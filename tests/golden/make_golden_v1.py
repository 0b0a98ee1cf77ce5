#!/usr/bin/env python3
"""Generate tests/golden/audio_model_v1.npz by running the REFERENCE's own ExprModelV1 (imported from /root/reference/src) on
the synthetic weights and waveforms of avcer_amd/synth.py.  Run where the reference is checked out
(`python tests/golden/make_golden_v1.py`); nothing under tests/ reads the reference at test time.

Shares make_golden.py's configuration and shims (w2v_config, stats, head16; `init_weights()` a no-op because every weight is
overwritten by the strict load_state_dict).  transformers is imported before make_golden is, so no stub module is in the way.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import transformers  # noqa: F401  (before any stub module exists)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository root and the reference's src on sys.path)
from avcer_amd import synth  # noqa: E402


def main():
    from transformers import Wav2Vec2FeatureExtractor
    from transformers.models.wav2vec2.modeling_wav2vec2 import Wav2Vec2PreTrainedModel

    Wav2Vec2PreTrainedModel.init_weights = lambda self: None
    from architectures.audio_7_cl import ExprModelV1 as ExprModelV1_7
    from architectures.audio_8_cl import ExprModelV1 as ExprModelV1_8

    proc = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True,
                                    return_attention_mask=True)

    def norm(wv):
        return np.stack([np.asarray(proc(torch.from_numpy(r[None]), sampling_rate=16000)["input_values"][0])[0] for r in wv])

    out = {}
    model = ExprModelV1_8(mg.w2v_config())
    model.load_state_dict(synth.to_torch(synth.audio_v1_state_dict(44)), strict=True)
    model.eval()
    taps = {}
    hooks = [
        model.wav2vec2.encoder.register_forward_hook(lambda m, i, o: taps.__setitem__("w2v", o[0])),
        model.gru.register_forward_hook(lambda m, i, o: taps.__setitem__("gru", o[0])),
        model.time_downsample.register_forward_hook(lambda m, i, o: taps.__setitem__("time_downsample", o)),
    ]
    for tag, wv in (("t32000", synth.waveforms(6678, 2, 32000)), ("t64000", synth.waveforms(6679, 1, 64000))):
        x = norm(wv)
        taps.clear()
        with torch.no_grad():
            lg = model(torch.from_numpy(x))
        out[f"{tag}_logits"] = lg.numpy()
        out[f"{tag}_features"] = taps["time_downsample"].squeeze().numpy()  # what get_features returns beside the logits
        for k, v in taps.items():
            out[f"{tag}_{k}_stats"] = mg.stats(v)
            out[f"{tag}_{k}_head16"] = mg.head16(v)
            out[f"{tag}_{k}_shape"] = np.array(v.shape)
        if tag == "t32000":
            out["t32000_gru_window0"] = taps["gru"][0].numpy().copy()  # [99, 256]: the whole GRU output of the first window
        print(tag, "logits", lg.numpy().reshape(-1, 8)[0], "shape", tuple(lg.shape), "gru", tuple(taps["gru"].shape),
              mg.stats(taps["gru"]))
    with torch.no_grad():
        one = model(torch.from_numpy(norm(synth.waveforms(6678, 2, 32000))[:1]))
    out["t32000_one_row_shape"] = np.array(one.shape)
    for h in hooks:
        h.remove()

    model7 = ExprModelV1_7(mg.w2v_config())
    model7.load_state_dict(synth.to_torch(synth.audio_v1_state_dict(45, 7)), strict=True)
    model7.eval()
    with torch.no_grad():
        lg7 = model7(torch.from_numpy(norm(synth.waveforms(6680, 2, 32000))))
    out["c7_t32000_logits"] = lg7.numpy()
    print("7-class logits", lg7.numpy()[0])
    np.savez_compressed(os.path.join(HERE, "audio_model_v1.npz"), **out)
    print("bytes", os.path.getsize(os.path.join(HERE, "audio_model_v1.npz")))


if __name__ == "__main__":
    main()
