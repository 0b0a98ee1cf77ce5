"""CPU restatement of the GRU-head audio model ExprModelV1 (test helper; the wav2vec2 trunk comes from oracle/audio.py).

Functional torch, in the dtype of the state dict and the input: float32 as the reference runs it, float64 when both are double
(oracle.audio.state_dict64 / expr_model_v1_forward64: the high-precision side of tests/test_gpu_expr_v1.py).  Pinned against
golden vectors of the reference's own ExprModelV1 (tests/golden/make_golden_v1.py -> tests/golden/audio_model_v1.npz) by
tests/test_expr_v1_cpu.py.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import audio as oa

HIDDEN = 256


def gru_layer(xp, w_hh, b_hh):
    """The recurrence of one torch.nn.GRU layer, gate by gate (gate order r, z, n; h_0 = 0), on the input projections of all
    steps xp = x W_ih^T + b_ih [B,S,3H]:  r = s(xp_r + W_hr h + b_hr), z = s(xp_z + W_hz h + b_hz),
    n = tanh(xp_n + r * (W_hn h + b_hn)), h' = (1 - z) * n + z * h.  Returns the sequence [B,S,H].
    ref: architectures/audio_8_cl.py:26-32,64 (nn.GRU(input_size=1024, hidden_size=256, num_layers=2, batch_first=True))."""
    b, s, _ = xp.shape
    hd = w_hh.shape[1]
    h = torch.zeros(b, hd, dtype=xp.dtype)
    out = []
    for t in range(s):
        hp = h @ w_hh.t() + b_hh
        r = torch.sigmoid(xp[:, t, :hd] + hp[:, :hd])
        z = torch.sigmoid(xp[:, t, hd:2 * hd] + hp[:, hd:2 * hd])
        n = torch.tanh(xp[:, t, 2 * hd:] + r * hp[:, 2 * hd:])
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out, dim=1)


def gru(sd, x, taps=None):
    """Both layers of `gru` on x [B,S,1024] -> [B,S,256]; the dropout between them is inactive in eval mode.
    ref: architectures/audio_8_cl.py:26-32,64; audio_7_cl.py:26-32,64."""
    h = x
    for l in (0, 1):
        xp = h @ sd[f"gru.weight_ih_l{l}"].t() + sd[f"gru.bias_ih_l{l}"]
        h = gru_layer(xp, sd[f"gru.weight_hh_l{l}"], sd[f"gru.bias_hh_l{l}"])
        if taps is not None:
            taps[f"gru{l + 1}"] = h
    return h


def head_v1(sd, x, taps=None):
    """permute, time_downsample at width 256, squeeze, Linear(256, classes): the V3 head's arithmetic at another width.
    ref: architectures/audio_8_cl.py:35-50,66-71.  Returns [B,C] ((C,) when B == 1, as `.squeeze()` does)."""
    return oa.head(sd, x, taps)


def expr_model_v1_forward(sd, x, taps=None):
    """ExprModelV1.forward, architectures/audio_8_cl.py:61-72 (audio_7_cl.py:61-72 for the 7-class model).
    taps gets the trunk's taps, "gru1", "gru2", "td0", "mp", "td4", "pooled", "logits"."""
    h = oa.wav2vec2_forward(sd, x, taps)
    h = gru(sd, h, taps)
    return head_v1(sd, h, taps)


def expr_model_v1_forward64(sd64, wav, taps=None, norm: bool = True):
    """The whole model in float64 from the float32 waveform [B,T] (sd64 = oracle.audio.state_dict64(sd)): the extractor's
    normalisation (get_prob_audio_8_cl.py:88-89) unless norm is False, then expr_model_v1_forward (audio_8_cl.py:61-72)."""
    with torch.no_grad():
        x = oa.normalize64(wav) if norm else torch.as_tensor(np.asarray(wav, dtype=np.float32)).double()
        if taps is not None:
            taps["norm"] = x
        return expr_model_v1_forward(sd64, x, taps)


def audio_forward_v1(sd, wav: torch.Tensor, sr: int, fps: float, window: float = 4, step: float = 0.5, padding: str = "mean"):
    """EmotionRecognition.load_audio_features (get_prob_audio_8_cl.py:68-126) around ExprModelV1: the chunker of oracle/audio.py
    and the model one window at a time, as the reference calls it.  Returns (per-frame logits rows, frame indices)."""
    chunks, spans = oa.make_chunks(wav, sr, fps, window, step, padding)
    with torch.no_grad():
        lg = np.stack([expr_model_v1_forward(sd, torch.from_numpy(c[None])).numpy() for c in chunks])
    return oa.replicate_per_frame(lg, spans)
