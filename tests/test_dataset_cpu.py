"""Host side of the packed dataset path: the ragged LSTM plan, the video sharding rule and the ragged all-gather (gloo)."""
import itertools
import os
import re
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from avcer_amd import _lib
from avcer_amd import dist as adist
from avcer_amd.dataset import VideoJob, exchange_tables, ragged_plan
from avcer_amd.video_pipeline import plan_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_plan_equals_plan_clip_per_video():
    rng = np.random.default_rng(3)
    presents = [
        np.ones(40, bool),
        np.r_[np.zeros(7, bool), np.ones(20, bool)],                          # leading gap
        np.r_[np.ones(11, bool), np.zeros(6, bool), np.ones(13, bool)],       # inner gap
        np.zeros(9, bool),                                                    # all absent
        rng.random(61) > 0.3,
        np.ones(1, bool),
    ]
    fpss = [25, 29, 60, 30, 29, 25]
    s_src, d_src, win, n_feat = ragged_plan(presents, fpss)
    assert n_feat == sum(int(p.sum()) for p in presents) and len(s_src) == len(d_src) == sum(len(p) for p in presents)
    at = fb = wb = 0
    for present, fps in zip(presents, fpss):
        p = plan_clip(present, fps, fb, wb)
        t = len(present)
        assert list(s_src[at:at + t]) == p.static_src and list(d_src[at:at + t]) == p.dyn_src
        assert win[wb:wb + len(p.windows)].tolist() == p.windows
        # the same video planned alone, shifted by its bases
        q = plan_clip(present, fps)
        assert [i + fb if i >= 0 else -1 for i in q.static_src] == p.static_src
        assert [i + wb if i >= 0 else -1 for i in q.dyn_src] == p.dyn_src
        assert [[i + fb for i in w] for w in q.windows] == p.windows
        at, fb, wb = at + t, fb + int(present.sum()), wb + len(p.windows)
    assert wb == len(win) and win.dtype == np.int32 and (win.size == 0 or win.max() < n_feat)
    assert (s_src[sum(len(p) for p in presents[:3]):][:9] == -1).all()        # the all-absent video: zero rows


def test_shard_videos_properties():
    costs = [3.0, 9.5, 1.0, 4.0, 4.0, 2.5, 7.0]
    for world in (1, 2, 3, 4, 8, 16):
        shards = adist.shard_videos(costs, world)
        assert len(shards) == world and sorted(i for s in shards for i in s) == list(range(len(costs)))
        assert all(s == sorted(s) for s in shards) and shards == adist.shard_videos(list(costs), world)
    assert adist.shard_videos([1, 1, 100, 1, 1], 2) == [[2], [0, 1, 3, 4]]    # costlier than all others together: alone
    assert adist.shard_videos([1, 100, 1, 1], 3)[0] == [1]
    assert adist.shard_videos([2.0, 1.0], 4) == [[0], [1], [], []]            # more ranks than videos: empty shards
    assert adist.shard_videos([], 2) == [[], []]
    assert adist.shard_videos([1, 1, 1, 1], 2) == [[0, 2], [1, 3]]            # ties: lowest index first, lowest rank first


def test_shard_videos_within_four_thirds_of_the_optimum():
    """Graham's bound for longest-processing-time-first: max load <= (4/3 - 1/(3 m)) x optimum; the optimum by exhaustion."""
    rng = np.random.default_rng(11)
    sets = [rng.integers(1, 30, 6).astype(float) for _ in range(40)] + [np.array([3, 3, 2, 2, 2, 0.5]), np.array([5, 5, 4, 4, 3, 3.0])]
    for costs in sets:
        for world in (2, 3):
            best = min(max(sum(c for c, r in zip(costs, assign) if r == k) for k in range(world))
                       for assign in itertools.product(range(world), repeat=len(costs)))
            got = max(sum(costs[i] for i in s) for s in adist.shard_videos(costs, world))
            assert got <= best * 4 / 3 + 1e-9, (costs, world, got, best)


def test_video_cost_terms():
    job = VideoJob("v", 75, 360, 640, 25, 48000)
    n_win = len(range(0, 48001, 8000))
    assert abs(adist.video_cost(job, 4, False) - (75 * 7.667 + 15 * 0.0577 + n_win * 91.299)) < 1e-9
    assert abs(adist.video_cost(job, 2, True) - (75 * (7.667 + 50.7) + 15 * 0.0577 + n_win * 44.891)) < 1e-9
    big = VideoJob("v", 75, 720, 1280, 30, 44100 * 3, wav_sr=44100)
    assert abs(adist.video_cost(big, 4, True) - (75 * (7.667 + 4 * 50.7) + 13 * 0.0577 + n_win * 91.299)) < 1e-9


def test_fuse_videos_is_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avcer_hip.h")).read(), flags=re.S)
    assert re.search(r"\bavcer_fuse_videos\s*\(", header)
    assert len(_lib.SIGNATURES["avcer_fuse_videos"][1]) == 22
    raw = open(os.path.join(ROOT, "include", "avcer_hip.h")).read()
    doc = raw[raw.index("avcer_audio_frame_mean + avcer_fuse for a CONCATENATION"):raw.index("int avcer_fuse_videos")]
    assert "run.py:85-165" in doc and "get_prob_audio_8_cl.py:94-101" in doc


# ------------------------------------------------------------------------------------------------ gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _records(n_videos):
    """Fabricated per-video tables: video i has 3 + 5 * (i % 4) frames and i % 3 windows (some have none)."""
    g = torch.Generator().manual_seed(1)
    n_f = [3 + 5 * (i % 4) for i in range(n_videos)]
    n_w = [i % 3 for i in range(n_videos)]
    rows = [torch.rand(n, 14, generator=g) for n in n_f]
    wins = [torch.rand(n, 8, generator=g) for n in n_w]
    return n_f, n_w, rows, wins


def _worker(rank, world, port, n_videos, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # (a) all_gather_ragged: rank r sends r % 3 * (r + 1) rows -- rank 0 (and every third) sends none
        mine = torch.full(((rank % 3) * (rank + 1), 5), float(rank)) + torch.arange(5)
        parts = adist.all_gather_ragged(mine)
        ok = len(parts) == world and all(
            torch.equal(p, torch.full(((r % 3) * (r + 1), 5), float(r)) + torch.arange(5)) for r, p in enumerate(parts))
        ints = adist.all_gather_ragged(torch.full((1 if rank % 2 else 0, 1), rank, dtype=torch.int32))
        ok = ok and all(p.dtype == torch.int32 and p.reshape(-1).tolist() == ([r] if r % 2 else []) for r, p in enumerate(ints))
        # (b) the payload exchange of run_dataset(distributed=True): unequal loads, a failed video (no rows), job order out
        n_f, n_w, rows, wins = _records(n_videos)
        failed = 2
        n_f[failed] = n_w[failed] = 0
        shards = adist.shard_videos([float(n) for n in _records(n_videos)[0]], world)
        sel = [i for i in shards[rank] if i != failed]
        loc_rows = torch.cat([rows[i] for i in sel]) if sel else torch.zeros(0, 14)
        loc_wins = torch.cat([wins[i] for i in sel]) if sel else torch.zeros(0, 8)
        full_rows, full_wins = exchange_tables(loc_rows, loc_wins, shards, n_f, n_w)
        keep = [i for i in range(n_videos) if i != failed]
        ok = ok and torch.equal(full_rows, torch.cat([rows[i] for i in keep])) and torch.equal(full_wins, torch.cat([wins[i] for i in keep]))
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def _run(world, n_videos):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_videos, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    return res


def test_all_gather_ragged_and_the_dataset_exchange_on_gloo():
    for world, n_videos in ((2, 7), (4, 7), (8, 5)):                          # 8 ranks, 5 videos: ranks without a video
        res = _run(world, n_videos)
        assert len(res) == world and all(ok for _, ok in res), (world, res)


def test_all_gather_ragged_is_the_identity_without_a_group():
    x = torch.rand(3, 4)
    assert adist.all_gather_ragged(x)[0] is x
    n_f, n_w, rows, wins = _records(4)
    full_rows, full_wins = exchange_tables(torch.cat(rows), torch.cat(wins), adist.shard_videos([1.0] * 4, 1), n_f, n_w)
    assert torch.equal(full_rows, torch.cat(rows)) and torch.equal(full_wins, torch.cat(wins))
