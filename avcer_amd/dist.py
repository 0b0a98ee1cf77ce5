"""Clip sharding across the GPUs of one node and the single collective of the path.

Clips are independent: rank r processes the contiguous block [r*N/W, (r+1)*N/W) with the
weights replicated, and the only exchange is ONE all-gather of the per-clip record
{static_probs[T,7], dyn_logits[T,7], audio_logits[C]} (928 B per clip at T = 16 frames and 8 audio classes) before the fusion, which then runs
replicated.  backend "nccl" is RCCL over xGMI on ROCm; the same code runs on gloo/CPU tensors in the tests.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def shard_range(n: int, rank: int, world: int):
    """Contiguous block partition; the first n % world ranks get one extra clip."""
    q, r = divmod(n, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def pack_records(stat: torch.Tensor, dyn: torch.Tensor, aud: torch.Tensor) -> torch.Tensor:
    n = stat.shape[0]
    return torch.cat([stat.reshape(n, -1), dyn.reshape(n, -1), aud.reshape(n, -1)], dim=1).contiguous()


def unpack_records(rec: torch.Tensor, t: int, c: int):
    n = rec.shape[0]
    stat = rec[:, :t * 7].reshape(n, t, 7)
    dyn = rec[:, t * 7:2 * t * 7].reshape(n, t, 7)
    aud = rec[:, 2 * t * 7:2 * t * 7 + c].reshape(n, c)
    return stat, dyn, aud


def all_gather_records(rec: torch.Tensor, n_total: int, force: bool = False) -> torch.Tensor:
    """All-gather of row blocks produced with shard_range (uneven blocks are padded to the largest one).
    `force`: run the collective at world size 1 as well (tests/test_gpu_rccl.py: the RCCL path on a one-GPU box)."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not force):
        return rec
    world, rank = dist.get_world_size(), dist.get_rank()
    sizes = [shard_range(n_total, r, world) for r in range(world)]
    mx = max(b - a for a, b in sizes)
    pad = torch.zeros(mx, rec.shape[1], dtype=rec.dtype, device=rec.device)
    pad[:rec.shape[0]] = rec
    out = torch.empty(world * mx, rec.shape[1], dtype=rec.dtype, device=rec.device)
    dist.all_gather_into_tensor(out, pad)
    parts = [out[r * mx:r * mx + (b - a)] for r, (a, b) in enumerate(sizes)]
    return torch.cat(parts, dim=0)


# ------------------------------------------------------------------------------------------------ whole videos of unequal length
def video_cost(job, window: float = 4, detector=False, sr: int = 16000, step: float = 0.5) -> float:
    """Algorithmic GFLOP of one video, from its metadata alone (`job`: n_frames, height, width, fps, n_samples, wav_sr): the
    figure `shard_videos` balances.  This is WORK, not measured time: the three models run at different fractions of the
    machine's peak, so equal cost is not equal time; it is what every rank can compute identically without running anything.
    Terms: per frame 7.667 for the static CNN, plus 50.7 * H*W / (640*360) when a
    detector runs; per LSTM evaluation 0.0577; per audio window 44.891 + (91.299 - 44.891) * (window*sr - 32000) / 32000.
    `detector`: False, True (RetinaFace-R50: 50.7) or the detector's own GFLOP per 640 x 360 frame (MobileNet-0.25: 1.116, S3FD: 144.27;
    the predictor's `gflop_per_frame`).  Every frame is counted as present (the face track is not known before stage 0)."""
    from .audio_pipeline import resample_out_len, resample_plan
    from .video_pipeline import lstm_step

    t = int(job.n_frames)
    det_gflop = 50.7 if detector is True else float(detector or 0.0)
    per_frame = 7.667 + det_gflop * (job.height * job.width) / (640 * 360)
    n_lstm = len(range(0, t, max(lstm_step(job.fps), 1)))
    n = int(job.n_samples)
    if getattr(job, "wav_sr", None) is not None:
        plan = resample_plan(job.wav_sr, sr)
        n = resample_out_len(n, plan.o, plan.n)
    n_win = len(range(0, n + 1, int(step * sr)))
    per_window = 44.891 + (91.299 - 44.891) * (window * sr - 32000) / 32000
    return t * per_frame + n_lstm * 0.0577 + n_win * per_window


def shard_videos(costs, world: int):
    """Longest-processing-time-first assignment of videos to `world` ranks: videos in the order (-cost, index), each to the
    rank with the smallest load so far (ties: the lowest rank).  Returns one ascending index list per rank.  Deterministic:
    every rank derives the same assignment from the job metadata.  Maximum load <= (4/3 - 1/(3 world)) x the optimum (Graham)."""
    if world < 1:
        raise ValueError("shard_videos: world >= 1")
    load = [0.0] * world
    shards = [[] for _ in range(world)]
    for i in sorted(range(len(costs)), key=lambda i: (-float(costs[i]), i)):
        r = min(range(world), key=lambda r: (load[r], r))
        load[r] += float(costs[i])
        shards[r].append(i)
    return [sorted(s) for s in shards]


def all_gather_ragged(rows: torch.Tensor, force: bool = False):
    """All-gather of row blocks of unequal height: rows [k_r, d] on rank r (k_r = 0 allowed, d equal on all ranks) -> a list with
    one tensor [k_r, d] per rank.  Two collectives: the row counts (one int64 per rank), then the payload padded to the longest
    block.  World size 1: the identity unless `force`, like all_gather_records."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not force):
        return [rows]
    world = dist.get_world_size()
    rows = rows.contiguous()
    k = torch.tensor([rows.shape[0]], dtype=torch.int64, device=rows.device)
    ks = torch.empty(world, dtype=torch.int64, device=rows.device)
    dist.all_gather_into_tensor(ks, k)
    ks = [int(v) for v in ks.cpu()]
    mx = max(max(ks), 1)
    pad = torch.zeros((mx,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    pad[:rows.shape[0]] = rows
    out = torch.empty((world * mx,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    dist.all_gather_into_tensor(out, pad)
    return [out[r * mx:r * mx + ks[r]] for r in range(world)]


def merge_shards(parts, shards, counts):
    """Undo `shard_videos` on gathered tables: parts[r] holds the rows of rank r's videos (shards[r], ascending) one behind the
    other, counts[i] rows for video i (0 for a video that contributes none).  Returns the rows in video order."""
    pieces = {}
    for part, shard in zip(parts, shards):
        at = 0
        for i in shard:
            pieces[i] = part[at:at + int(counts[i])]
            at += int(counts[i])
        if at != part.shape[0]:
            raise ValueError(f"merge_shards: a rank sent {part.shape[0]} rows, its videos account for {at}")
    return torch.cat([pieces[i] for i in range(len(counts))], dim=0)
