#!/usr/bin/env python3
"""Generate tests/golden/audio_long.npz: the REFERENCE's own ExprModelV3 and ExprModelV1 (imported from /root/reference/src) on
windows longer than 256 tokens -- T = 82 320 samples (257 tokens) and T = 128 080 (400 tokens), two windows each -- with the
synthetic weights and waveforms of avcer_amd/synth.py and eager attention, the way make_golden.py and make_golden_v1.py drive
them.  Run where the reference is checked out (`python tests/golden/make_golden_audio_long.py`); nothing under tests/ reads the
reference at test time.

Stored per model and length: the logits, and of the trunk's output (`w2v`) and the head's last sequence layer (`tl2` for V3, `gru`
for V1) the shape, the first 16 values and the largest magnitude.
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

LENGTHS = ((82320, 257), (128080, 400))  # samples, tokens
SEEDS = {"v3": (42, 7701), "v1": (44, 7801)}  # weights, waveforms (+ the length's index)


def main():
    from transformers import Wav2Vec2FeatureExtractor
    from transformers.models.wav2vec2.modeling_wav2vec2 import Wav2Vec2PreTrainedModel

    Wav2Vec2PreTrainedModel.init_weights = lambda self: None
    from architectures.audio_8_cl import ExprModelV1, ExprModelV3

    proc = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True,
                                    return_attention_mask=True)

    def norm(wv):
        return np.stack([np.asarray(proc(torch.from_numpy(r[None]), sampling_rate=16000)["input_values"][0])[0] for r in wv])

    out = {}
    for tag, cls, sd, head in (("v3", ExprModelV3, synth.audio_state_dict(SEEDS["v3"][0]), "tl2"),
                               ("v1", ExprModelV1, synth.audio_v1_state_dict(SEEDS["v1"][0]), "gru")):
        model = cls(mg.w2v_config())
        model.load_state_dict(synth.to_torch(sd), strict=True)
        model.eval()
        taps = {}
        hooks = [model.wav2vec2.encoder.register_forward_hook(lambda m, i, o: taps.__setitem__("w2v", o[0])),
                 getattr(model, head).register_forward_hook(
                     lambda m, i, o, head=head: taps.__setitem__(head, o[0] if isinstance(o, tuple) else o))]
        for li, (t, tokens) in enumerate(LENGTHS):
            x = norm(synth.waveforms(SEEDS[tag][1] + li, 2, t))
            taps.clear()
            with torch.no_grad():
                lg = model(torch.from_numpy(x))
            key = f"{tag}_t{t}"
            out[f"{key}_logits"] = lg.numpy()
            for k, v in taps.items():
                assert v.shape[1] == tokens, (k, tuple(v.shape))
                out[f"{key}_{k}_shape"] = np.array(v.shape)
                out[f"{key}_{k}_head16"] = mg.head16(v)
                out[f"{key}_{k}_absmax"] = np.array(v.detach().abs().max().item())
            print(key, "logits", lg.numpy()[0], {k: tuple(v.shape) for k, v in taps.items()})
        for h in hooks:
            h.remove()
    np.savez_compressed(os.path.join(HERE, "audio_long.npz"), **out)
    print("bytes", os.path.getsize(os.path.join(HERE, "audio_long.npz")))


if __name__ == "__main__":
    main()
