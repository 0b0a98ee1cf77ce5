#!/usr/bin/env python
"""Generate tests/golden/augment.npz by running the REFERENCE's own waveform augmentations and its MELD window planner (imported
from /root/reference/src/audio) on small synthetic inputs; only the inputs and what the reference returned are kept.

Run in the build container only (`python tests/golden/make_augment_golden.py`, needs pandas and torch); /root/reference does not
exist anywhere else, and no test imports this file.

What is called, unmodified and unbound, on a stub object that carries only the attributes the method reads:
  PolarityInversion.forward      src/audio/augmentation/wave_augmentation.py:14-24
  WhiteNoise.forward             src/audio/augmentation/wave_augmentation.py:40-53, under random.seed / np.random.seed; the value
                                 np.random.normal returned to it is recorded on its way through (a wrapper that passes arguments and
                                 result on unchanged), as is the draw random.uniform makes (random.random() under the same seed)
  MeldDataset.prepare_data       src/audio/data/meld_dataset.py:93-180, over a temporary label CSV and VAD pickle
Gain is torchaudio.transforms.Vol, and torchaudio is not installed here: it is not recorded; tests/test_augment_cpu.py compares
with the torch expressions its source consists of.
The modules import torchaudio, torchvision, transformers and a `config` module at their top; none of the three methods uses them,
so empty stand-in modules are put into sys.modules first.

The MELD planner returns each utterance's windows in the order of a Python set; they are stored sorted by (start_f, end_f), which is
the order avcer_amd.audio_corpus.meld_windows documents.

Cases.  Noise: windows of 1000, 1 and 4099 samples: a sine, a signal with padding zeros behind it, all zeros, one sample (std NaN),
values beyond +-1.  MELD (16 kHz, shift 2, min 2, max 4; 8, 7 and 6 classes): segments shorter than min_w_len (31999 samples), of
exactly min_w_len, between min and max with the tail fallback to the segment's start and the duplicate it creates (50000), longer
than max with a tail that falls back to end - max_w_len (150000), a multiple of the shift (128000), two and three segments in one
utterance, every emotion, the dia125_utt3 row and a row the VAD pickle does not list."""
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_AUDIO = "/root/reference/src/audio"


def _stand_ins():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    module("torchaudio")
    tv = module("torchvision")
    tv.transforms = module("torchvision.transforms")
    tv.transforms.transforms = module("torchvision.transforms.transforms", Compose=object)
    module("transformers", Wav2Vec2Processor=object)
    module("config", c_config={})
    sys.path.insert(0, REF_AUDIO)


def noise_cases():
    rs = np.random.RandomState(20240611)
    t = np.arange(1000) / 16000.0
    padded = np.zeros(1000, np.float32)
    padded[:371] = (0.05 * rs.randn(371)).astype(np.float32)
    return {
        "sine": (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.01 * rs.randn(1000)).astype(np.float32),
        "padded": padded,
        "zeros": np.zeros(1000, np.float32),
        "one": np.asarray([0.25], np.float32),
        "loud": (1.7 * rs.randn(4099)).astype(np.float32),
        "offset": (0.9 + 1e-3 * rs.randn(1000)).astype(np.float32),
    }


MELD_ROWS = [  # Dialogue_ID, Utterance_ID, Emotion, segments
    (0, 0, "neutral", [(0, 31999)]),
    (0, 1, "anger", [(1000, 33000)]),
    (0, 2, "joy", [(0, 50000)]),
    (1, 0, "sadness", [(2500, 152500)]),
    (1, 1, "surprise", [(0, 128000)]),
    (2, 0, "fear", [(0, 20000), (30000, 100000)]),
    (2, 7, "disgust", [(160, 40160), (48000, 80000), (90000, 250000)]),
    (3, 0, "neutral", [(0, 64000)]),
    (3, 1, "joy", [(5, 64006)]),
    (125, 3, "anger", [(0, 70000)]),       # the reference's broken file
    (9, 9, "joy", None),                   # not in the VAD pickle
]


def main():
    _stand_ins()
    from augmentation.wave_augmentation import PolarityInversion, WhiteNoise
    from data.meld_dataset import MeldDataset

    out = {}
    names = []
    real_normal = np.random.normal
    for i, (name, x) in enumerate(noise_cases().items()):
        names.append(name)
        audio = torch.from_numpy(x.copy())[None, :]          # [1, win], as torchaudio.load returns a mono file
        seen = []

        def recording_normal(*a, **k):
            v = real_normal(*a, **k)
            seen.append((a, v))
            return v

        random.seed(100 + i)
        u = random.random()
        random.seed(100 + i)
        np.random.seed(200 + i)
        np.random.normal = recording_normal
        try:
            stub = types.SimpleNamespace(min_snr=0.0001, max_snr=0.005)
            with np.errstate(all="ignore"):
                noised = WhiteNoise.forward(stub, audio)
        finally:
            np.random.normal = real_normal
        (args, drawn), = seen
        out[f"noise/{name}/x"] = x
        out[f"noise/{name}/u"] = np.float64(u)
        out[f"noise/{name}/std"] = np.float32(torch.std(audio).numpy())
        out[f"noise/{name}/noise_std"] = np.float64(args[1])
        out[f"noise/{name}/noise"] = np.asarray(drawn).astype(np.float32).reshape(-1)
        out[f"noise/{name}/out"] = noised.numpy().reshape(-1)
        out[f"polarity/{name}/out"] = PolarityInversion.forward(None, audio).numpy().reshape(-1)
    out["noise_cases"] = np.asarray(names)
    out["min_snr"], out["max_snr"] = np.float64(0.0001), np.float64(0.005)

    # ---- MELD
    csv_lines = ["Sr No.,Utterance,Speaker,Emotion,Sentiment,Dialogue_ID,Utterance_ID,Season,Episode,StartTime,EndTime"]
    vad = {}
    for k, (dia, utt, emo, segs) in enumerate(MELD_ROWS):
        csv_lines.append(f'{k + 1},"words, with a comma",Someone,{emo},neutral,{dia},{utt},1,1,"00:00:01,000","00:00:02,000"')
        if segs is not None:
            vad[f"dia{dia}_utt{utt}.wav"] = [{"start": a, "end": b} for a, b in segs]
    out["meld/csv"] = np.asarray("\n".join(csv_lines) + "\n")
    out["meld/vad_files"] = np.asarray(sorted(vad))
    out["meld/vad_segments"] = np.asarray([[j, s["start"], s["end"]] for j, fn in enumerate(sorted(vad)) for s in vad[fn]], dtype=np.int64)
    for classes in (8, 7, 6):
        with tempfile.TemporaryDirectory() as root:
            with open(os.path.join(root, "labels.csv"), "w") as f:
                f.write(str(out["meld/csv"]))
            with open(os.path.join(root, "vad.pickle"), "wb") as f:
                pickle.dump(vad, f)
            stub = types.SimpleNamespace(shift=2, min_w_len=2, max_w_len=4, sr=16000, num_classes=classes, meta=[], expr_labels=[],
                                         labels_file_path=os.path.join(root, "labels.csv"), vad_file_path=os.path.join(root, "vad.pickle"))
            stub.meld_to_abaw_labels = types.MethodType(MeldDataset.meld_to_abaw_labels, stub)
            MeldDataset.prepare_data(stub)
        assert [d["expr"] for d in stub.meta] == stub.expr_labels
        files = []
        for d in stub.meta:
            if d["wav_filename"] not in files:
                files.append(d["wav_filename"])          # the utterances in the dataset's order
        out[f"meld{classes}/files"] = np.asarray(files)
        for fn in files:
            mine = sorted((d for d in stub.meta if d["wav_filename"] == fn), key=lambda d: (d["start_f"], d["end_f"]))
            out[f"meld{classes}/{fn}/t"] = np.asarray([[d["start_t"], d["end_t"]] for d in mine], dtype=np.float64).reshape(-1, 2)
            out[f"meld{classes}/{fn}/f"] = np.asarray([[d["start_f"], d["end_f"], d["expr"]] for d in mine], dtype=np.int64).reshape(-1, 3)
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
