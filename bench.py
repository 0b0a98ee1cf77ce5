#!/usr/bin/env python3
"""Headline benchmark: clips/s of the full AV hot path (static CNN + LSTM + audio model + fusion) on synthetic
clips of 16 x 224x224 frames + 2 s @ 16 kHz (BASELINE.json metric), one process per GPU.

    python bench.py --gpus 1 --steps 5 --warmup 2 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path over one batch of `--clips` clips per GPU (weak scaling; 128 clips/GPU = BASELINE
config 5 at 8 GPUs; the static CNN runs in passes of up to 1024 frames).  Inputs are resident in HBM before
the timed region.  Rank 0 prints ONE JSON line.  The headline `value` is measured in a parity-green arithmetic mode
(--mode x3, default: f16 MFMA on fp16 hi/lo operand pairs with f32 accumulation, f32-grade: probabilities within 1e-4 of
the CPU oracle at every head sharpness tested; --mode fp32: exact f32 MFMA).

A plain run sets up, warms up, times exactly `--steps` steps and prints the line (`ms_per_step` = one timed step); with
`--dump-outputs DIR` it also writes what the last timed step returned (dump_outputs).  `--full` adds everything else, each
after the timed region: the serial evented pass behind `roofline`, the other arithmetic modes under "modes" (each with ITS
measured max |dprob|; plain bf16 does not meet the 1e-4 gate and is never the headline), the multi-rank check, BASELINE
configs 2 and 3, per-call latency, `configs.run_inference`, the measured ceilings of the GPU, the CPU baseline and the oracle
parity.  The --no-* switches below leave out single legs of a --full run.
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from avcer_amd import dist as adist  # noqa: E402
from avcer_amd import synth  # noqa: E402
from avcer_amd.engine import MODE_BF16, MODE_F16X3, MODE_FP32  # noqa: E402

T_FRAMES, T_AUDIO, FPS = 16, 32000, 25
# Algorithmic work (forward hooks on the imported reference; 1 MAC = 2 FLOP)
GFLOP_STATIC_FRAME_REF = 7.667      # ResNet-50 224x224 + fc as the reference's graph evaluates it
# The last bottleneck of stages 1-3 feeds only the next stage's stride-2 1x1 convolutions (video.py:12-19,140-149): its conv2 /
# conv3 outputs at the other positions are never read, and the library does not compute them (api.hip run_stage):
# 53 248 MAC x (3025 - 784) + 212 992 x (784 - 196) + 851 968 x (196 - 49) positions = 369.8 MMAC per frame.
GFLOP_STATIC_UNREAD = 2 * (53248 * 2241 + 212992 * 588 + 851968 * 147) * 1e-9
GFLOP_STATIC_FRAME = GFLOP_STATIC_FRAME_REF - GFLOP_STATIC_UNREAD   # products whose results are used: every rate below counts these
GFLOP_LSTM_EVAL = 0.0577
GFLOP_AUDIO_CHUNK = 44.891          # ExprModelV3 at 2 s
GFLOP_AUDIO_NOT_GEMM = 0.482 + 0.080 + 0.0655 + 0.0000164  # attention matmuls, conv layer 0, final Linear
LSTM_EVALS_PER_CLIP = 4             # frames 0,5,10,15 at 25 fps
GFLOP_CLIP = T_FRAMES * GFLOP_STATIC_FRAME + LSTM_EVALS_PER_CLIP * GFLOP_LSTM_EVAL + GFLOP_AUDIO_CHUNK
GFLOP_CLIP_GEMM = GFLOP_CLIP - GFLOP_AUDIO_NOT_GEMM - 2 * 512 * 7 * T_FRAMES * 1e-9  # through conv_gemm
GUIDE = "/opt/skills/guides/MI355X_MICROARCH.md"
PEAK_FALLBACK = {"fp32": 157.3, "bf16": 2500.0, "x3": 2500.0}  # used only where the guide file is absent
MFMA_PASSES = {"fp32": 1, "bf16": 1, "x3": 3}  # MFMA products issued per algorithmic product
DTYPE = {"fp32": "f32", "bf16": "bf16", "x3": "f16x3 (f16 MFMA on hi/lo-split f32 operands, f32 accumulate)"}
# what roofline.achieved aggregates: every MFMA kernel family of the step (roofline.per_family prices each one on its own)
KERNEL = {"fp32": "all MFMA launches of a step: conv_gemm_kernel<0,0,*>",
          "bf16": "all MFMA launches of a step: conv_gemm_kernel<1,*,*>",
          "x3": "all MFMA launches of a step, six families: conv_gemm_wd_kernel<*,*,*> (weights direct, about half of the time), "
                "bneck_kernel<*> (fused bottleneck chains, HBM-bound), bneck_tail2_kernel<256>, conv_gemm_kernel<3|2,*,*>, "
                "stem_pool_u8_kernel, conv_gemm_skinny_kernel<*> (launches of few positions: the LSTM steps) -- see roofline.per_family"}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.2-6.3 TB/s measured for a streaming copy)
FAMILY_BOUND = {"bneck_kernel": "hbm"}  # every other family is priced against the MFMA peak
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: at most this much in all


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def usable_cores() -> int:
    """CPU threads this process may actually use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, min(n, 64))


def peaks():
    """Dense MFMA peaks (TFLOP/s) read from the MI355X guide's chip-level table, plus the figure the device properties
    imply (CUs x 4 SIMDs x 1024 bf16 FLOP/clk x max clock) for comparison.  Returns (per-mode dict, source string)."""
    pk, src = dict(PEAK_FALLBACK), ("MI355X_MICROARCH.md chip-level table, constants copied into bench.py (the guide file is not on "
                                     "this box)")
    try:
        txt = open(GUIDE).read()
        bf = re.search(r"Peak BF16/FP16 MFMA\s*\|\s*\*\*~?([0-9.]+)\s*PF dense", txt)
        f32 = re.search(r"Peak FP32 \(matrix\)\s*\|\s*([0-9.]+)\s*TFLOPS", txt)
        if bf and f32:
            pk = {"fp32": float(f32.group(1)), "bf16": float(bf.group(1)) * 1e3, "x3": float(bf.group(1)) * 1e3}
            src = GUIDE + " (chip-level parameters)"
    except OSError:
        pass
    return pk, src


def kernel_source_hash():
    """Hash of the HIP sources and headers in the tree (avcer_amd/build.py source_hash): a committed PMC traffic figure is only
    valid for the kernels it was measured on, and the loaded binary must carry the same hash (binary_source_hash)."""
    from avcer_amd.build import source_hash
    return source_hash()


def pmc_traffic(mode, clips):
    """HBM bytes per MFMA-kernel launch from the committed rocprofv3 --pmc passes (tools/pmc_traffic.py): the counters
    cannot be read from inside this process, so the figure comes from profiles/ when it matches this configuration.
    Returns (bytes per launch, file, stamp dict); `stale` in the stamp says the kernels changed since the passes."""
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_traffic_{mode}.json")), reverse=True):
        try:
            d = json.load(open(path))
        except (OSError, ValueError):
            continue
        if d.get("clips_per_gpu") == clips:
            stamp = {"commit": d.get("commit"), "kernel_source_hash": d.get("kernel_source_hash"),
                     "stale": d.get("kernel_source_hash") != kernel_source_hash()}
            return d["hbm_bytes_per_launch"], os.path.relpath(path, ROOT), stamp
    return None, None, None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=128, help="clips per GPU per step")
    ap.add_argument("--mode", choices=["x3", "fp32", "bf16"], default="x3", help="arithmetic of the headline value")
    ap.add_argument("--no-secondary", action="store_true", help="skip the other arithmetic modes")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg")
    ap.add_argument("--cpu-clips", type=int, default=64, help="upper bound of the CPU baseline sample (sized to ~12 s)")
    ap.add_argument("--parity-clips", type=int, default=2)
    ap.add_argument("--no-configs", action="store_true", help="skip the per-model BASELINE configs 2 and 3")
    ap.add_argument("--no-overlap", action="store_true", help="timed steps on ONE stream (default: the audio branch runs on "
                                                             "its own HIP stream beside the visual branch)")
    ap.add_argument("--one-lane", action="store_true", help="A/B: avcer_set_static_lanes(1) -- every static-CNN call on one stream")
    ap.add_argument("--no-events", action="store_true", help="skip the separate evented pass (the roofline object is then empty)")
    ap.add_argument("--no-run-inference", action="store_true", help="skip configs.run_inference (one 30 s video through run.py)")
    ap.add_argument("--full", action="store_true", help="also run every measurement and check beyond the headline (roofline pass, "
                                                         "other modes, configs, CPU baseline, parity, ceilings, multi-rank check)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the arrays the last timed step returned to DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def make_inputs(n_clips, rank, device):
    frames = torch.from_numpy(synth.face_frames(1234 + rank, n_clips * T_FRAMES))
    frames = frames.reshape(n_clips, T_FRAMES, 224, 224, 3).to(device)
    wav = torch.from_numpy(synth.waveforms(5678 + rank, n_clips, T_AUDIO)).to(device)
    return frames, wav


def one_step(pipe, frames, wav, n_total):
    """shard-local records -> one all-gather -> replicated fusion (avcer_amd/dist.py)."""
    stat, dyn, aud = pipe.clip_records(frames, wav, FPS)
    if dist.is_initialized() and dist.get_world_size() > 1:
        rec = adist.pack_records(stat, dyn, aud)
        if dist.get_backend() == "gloo":  # rehearsal only: the CPU backend cannot take device tensors
            rec = adist.all_gather_records(rec.cpu(), n_total).to(stat.device)
        else:
            rec = adist.all_gather_records(rec, n_total)
        stat, dyn, aud = adist.unpack_records(rec, T_FRAMES, aud.shape[1])
    return pipe.fuse_records(stat.contiguous(), dyn.contiguous(), aud.contiguous())


def timed(pipe, frames, wav, n_total, steps, warmup, device, profile):
    """The timed region proper: `warmup` untimed steps, then exactly `steps` steps between barrier + synchronize pairs,
    WITHOUT any per-launch instrumentation.  When `profile` is set, a second pass of the same `steps` steps follows, outside
    the timed region, strictly serial (one stream) and with a HIP-event pair around every MFMA-kernel launch: the roofline
    figure comes from that pass, so the measurement does not sit inside the thing measured and co-running kernels of the
    overlapped audio branch cannot inflate per-launch durations.  Also returns what the last timed step returned (`last`)."""
    for _ in range(warmup):
        one_step(pipe, frames, wav, n_total)
    torch.cuda.synchronize(device)
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        last = one_step(pipe, frames, wav, n_total)
    torch.cuda.synchronize(device)
    own = time.perf_counter() - t0  # this rank's K steps, before it waits for the others
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    per_rank = [dt]
    if dist.is_initialized():
        # every rank's own clock over the timed region (the barriers bracket it, so these differ only by how long a rank waited
        # at the closing barrier's entry): the MAX is the job's time, the list shows the load balance behind it
        cdev = "cpu" if dist.get_backend() == "gloo" else device
        mine = torch.tensor([own], device=cdev, dtype=torch.float64)
        every = torch.zeros(dist.get_world_size(), device=cdev, dtype=torch.float64)
        dist.all_gather_into_tensor(every, mine)
        per_rank = [float(v) for v in every.cpu()]
        t = torch.tensor([dt], device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    kern_ms, launches, serial_dt, fams = 0.0, 0, None, None
    if profile:
        overlap = pipe.overlap_branches
        pipe.overlap_branches = False
        # one untimed step in the schedule of the evented pass: serial in every sense (one stream, and the library runs its
        # static-CNN calls on ONE lane while events are recorded), which sizes the one-lane workspace outside the clock
        pipe.engine.profile_enable(True)
        one_step(pipe, frames, wav, n_total)
        torch.cuda.synchronize(device)
        pipe.engine.profile_read_families()  # discarded; rewinds the event pool
        pipe.engine.gemm_stats(reset=True)
        t0 = time.perf_counter()
        for _ in range(steps):
            one_step(pipe, frames, wav, n_total)
        torch.cuda.synchronize(device)
        serial_dt = time.perf_counter() - t0
        fams = pipe.engine.profile_read_families()
        kern_ms, launches = sum(v[0] for v in fams.values()), sum(v[1] for v in fams.values())
        pipe.engine.profile_enable(False)
        pipe.overlap_branches = overlap
    return dt, kern_ms, launches, serial_dt, per_rank, fams, last


def dump_outputs(path, prob, am, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: the arrays one_step returns to its caller, from the last timed step -- the compound probabilities
    [4, clips, 16, 7] (float64, as the library computes them) and the compound argmax [4, clips, 16] (as float32) -- one
    DIR/<name>.npy each.  The inputs and weights are pure functions of their seeds, so two builds run with the same arguments
    can be compared array for array.  Above `limit` bytes in all, a fixed seeded sample of clips is written instead, with
    their indices as clip_index.npy.  Returns the names written."""
    arrays = {"compound_prob": prob.cpu().numpy().astype(np.float64), "compound_argmax": am.cpu().numpy().astype(np.float32)}
    n = arrays["compound_prob"].shape[1]
    per_clip = sum(a.nbytes for a in arrays.values()) // n + 8
    if per_clip * n > limit - 4096:  # 4 KiB: the .npy headers
        keep = np.sort(np.random.default_rng(0).choice(n, (limit - 4096) // per_clip, replace=False))
        arrays = {k: a[:, keep] for k, a in arrays.items()}
        arrays["clip_index"] = keep.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))
    return sorted(arrays)


def verify_ranks(pipe, frames, wav, n_total, clips, world, rank, device, check=8):
    """Multi-rank correctness of the sharded path, asserted (not just timed): after the all-gather every rank must hold
    the same compound predictions, and they must equal a single-rank run over the same clips.  Rank 0 regenerates the
    first `check` clips of EVERY rank's shard (the generators are pure functions of (seed, index)), runs them through
    the pipeline on its own and compares bit for bit -- the kernels' results do not depend on batch composition
    (tests/test_gpu_visual.py::test_static_batch_invariance_256), so equality is exact."""
    prob, am = one_step(pipe, frames, wav, n_total)
    torch.cuda.synchronize(device)
    am_host = am.cpu().numpy()
    digest = hashlib.sha256(am_host.tobytes() + prob.cpu().numpy().tobytes()).hexdigest()
    digests = [None] * world
    dist.all_gather_object(digests, digest)
    agree = len(set(digests)) == 1
    single = None
    if rank == 0:
        check = min(check, clips)
        single = True
        for r in range(world):
            f = torch.from_numpy(synth.face_frames(1234 + r, check * T_FRAMES)).reshape(check, T_FRAMES, 224, 224, 3)
            w = torch.from_numpy(synth.waveforms(5678 + r, check, T_AUDIO))
            alone = pipe.run_clips(f.to(device), w.to(device), FPS)
            lo = adist.shard_range(n_total, r, world)[0]
            single = single and bool(np.array_equal(alone["compound_argmax"].cpu().numpy(), am_host[:, lo:lo + check]))
            single = single and bool(torch.equal(alone["compound_prob"].cpu(), prob[:, lo:lo + check].cpu()))
    flag = [agree and (single is not False)]
    dist.broadcast_object_list(flag, src=0)
    if not agree or not flag[0]:
        raise SystemExit(f"bench.py: rank {rank}: multi-rank check FAILED (ranks agree: {agree}, digests {digests}, "
                         f"equals single-rank run: {single})")
    return {"ranks_hold_identical_predictions": agree, "equals_single_rank_run": single, "checked_clips_per_rank": check}


def gpu_outputs(pipe, frames, wav):
    """Product-path outputs for the parity clips of one arithmetic mode, as numpy (no oracle involved)."""
    out = pipe.run_clips(torch.from_numpy(frames), torch.from_numpy(wav), FPS)
    return {k: out[k].cpu().numpy() for k in ("static_probs", "dynamic_logits", "audio_logits", "compound_prob",
                                              "compound_argmax")}


def cpu_baseline(n_clips, gpu_by_mode, n_parity, timed=True):
    """The ONLY leg that touches oracle/: the CPU restatement of the reference (kind = "port") is timed on this box's
    host cores on a bounded sample of the same workload (batched static CNN over a clip's 16 frames, 4 LSTM
    evaluations, one audio window), and its outputs for the first `n_parity` clips check the GPU outputs of every
    measured arithmetic mode (gpu_by_mode: name -> gpu_outputs on those same clips)."""
    from oracle import audio as oa
    from oracle import fusion as of
    from oracle import video as ov

    cores = usable_cores()
    torch.set_num_threads(cores)
    log(f"cpu baseline on {cores} threads (os.cpu_count()={os.cpu_count()})")
    sds = [synth.to_torch(f(42)) for f in (synth.static_state_dict, synth.dynamic_state_dict, synth.audio_state_dict)]
    frames, wav = cpu_sample(n_clips)

    def clip(c):
        st, dy = ov.visual_forward(sds[0], sds[1], frames[c], np.ones(T_FRAMES, bool), FPS, batched=True)
        with torch.no_grad():
            lg = oa.expr_model_v3_forward(sds[2], torch.from_numpy(oa.normalize(wav[c:c + 1]))).numpy().reshape(1, -1)
        rows, fr = oa.replicate_per_frame(lg, [(0, T_AUDIO, 0, T_FRAMES)])
        prob, am = of.fuse(st.astype(np.float32), dy.astype(np.float32), rows, fr)
        return st, dy, lg, prob, am

    t0 = time.perf_counter()
    ref = [clip(0)]  # warm-up, also parity clip 0
    warm = time.perf_counter() - t0
    for c in range(1, n_parity):
        ref.append(clip(c))
    parity = {}
    for name, g in gpu_by_mode.items():
        worst, same = 0.0, True
        for c, (st, dy, lg, prob, am) in enumerate(ref):
            worst = max(worst, float(np.abs(g["static_probs"][c] - st).max()),
                        float(np.abs(of.softmax(g["dynamic_logits"][c]) - of.softmax(dy.astype(np.float32))).max()),
                        float(np.abs(of.softmax(g["audio_logits"][c:c + 1, :7]) - of.softmax(lg[:, :7])).max()),
                        float(np.abs(g["compound_prob"][:, c] - prob).max()))
            same = same and bool(np.array_equal(g["compound_argmax"][:, c], am))
        parity[name] = (worst, same)
    if not timed:  # N > 1: rank 0 keeps the parity check; the CPU baseline itself is an N = 1 figure
        return None, parity
    # bounded sample: after the warm-up clips above, best of 3 passes over the same clips, each pass about 5 s of CPU work
    t0 = time.perf_counter()
    clip(0)
    one = max(time.perf_counter() - t0, 1e-3)
    passes = 3 if one < 5.0 else 1  # slow host: one pass, so the default run stays within minutes
    n_clips = max(1, min(n_clips, int(5.0 / one)))
    dts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        for c in range(n_clips):
            clip(c)
        dts.append(time.perf_counter() - t0)
    dt = min(dts)
    # the reference's own call pattern (get_prob_video.py:91-166): one frame per forward pass
    t1 = time.perf_counter()
    ov.visual_forward(sds[0], sds[1], frames[0], np.ones(T_FRAMES, bool), FPS, batched=False)
    with torch.no_grad():
        oa.expr_model_v3_forward(sds[2], torch.from_numpy(oa.normalize(wav[0:1])))
    loop_dt = time.perf_counter() - t1
    base = {"value": n_clips / dt, "unit": "clips/s", "cores": cores, "kind": "port",
            "sample": f"{n_clips} clips (16 frames batched + 4 LSTM evals + one 2 s window each), torch-CPU fp32 oracle, "
                      f"warm-up {n_parity + 1} clips, best of {passes} passes ({', '.join('%.1f' % d for d in dts)} s)",
            "frame_by_frame_value": 1.0 / loop_dt,
            "frame_by_frame_sample": "1 clip, one frame per forward pass as the reference drives it"}
    return base, parity


def cpu_sample(n_clips):
    """Inputs of the CPU leg (and of the parity check): same generator and shapes as the GPU workload."""
    frames = synth.face_frames(1234, n_clips * T_FRAMES).reshape(n_clips, T_FRAMES, 224, 224, 3)
    return frames, synth.waveforms(5678, n_clips, T_AUDIO)


def free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N ranks with torch.distributed.run as a CHILD process and
    exit with its code.  Nothing in this parent has touched the GPU (torch.cuda.device_count() does not initialise it)."""
    have = torch.cuda.device_count()
    rehearse = os.environ.get("AVCER_BENCH_REHEARSE") == "1"
    if have < args.gpus and not rehearse:
        sys.exit(f"bench.py: --gpus {args.gpus} but this node exposes {have} GPU(s); set AVCER_BENCH_REHEARSE=1 to "
                 f"rehearse the {args.gpus}-rank path on one GPU (gloo collective, flagged in the output)")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    log("spawning " + " ".join(cmd))
    return subprocess.call(cmd, env=env)


def config_benches(pipe, modes, pk, device, iters=5):
    """BASELINE configs[1] (static CNN, batch 256) and configs[2] (audio model, 128 windows of 2 s) on their own:
    ~20 ms of GPU time each per mode.  Returns {name: {mode: {...}}} with the MFMA-kernel roofline of each."""
    eng = pipe.engine
    out = {}

    def run(label, fn, units, gflop_unit, gflop_mfma_unit, unit_name, mode_names):
        res = {}
        for name in mode_names:
            fn(modes[name])
            fn(modes[name])
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(iters):
                fn(modes[name])
            torch.cuda.synchronize(device)
            dt = (time.perf_counter() - t0) / iters  # wall time per pass without the profiling events
            eng.profile_enable(True)
            for _ in range(iters):
                fn(modes[name])
            torch.cuda.synchronize(device)
            kern_ms, launches = eng.profile_read()  # a second set of passes carries the per-launch HIP events
            eng.profile_enable(False)
            tf = gflop_unit * units / dt / 1e3
            ach = gflop_mfma_unit * units * iters / kern_ms if kern_ms else None  # GFLOP / ms = TFLOP/s inside the MFMA kernels
            res[name] = {"value": units / dt, "unit": unit_name + "/s", "ms": dt * 1e3, "dtype": DTYPE[name],
                         "algorithmic_tflops": tf, "frac_of_mfma_peak": tf / pk[name],
                         "frac_of_mfma_peak_executed": tf * MFMA_PASSES[name] / pk[name],
                         "roofline": {"bound": "mfma", "achieved": ach, "peak": pk[name], "unit": "TFLOP/s",
                                      "frac": ach / pk[name] if ach else None,
                                      "launches": launches // iters, "avg_launch_us": kern_ms * 1e3 / launches if launches else None}}
        out[label] = res

    frames = torch.from_numpy(synth.face_frames(1, 256)).to(device)
    run("static_b256", lambda m: eng.static_forward(frames, m), 256, GFLOP_STATIC_FRAME, GFLOP_STATIC_FRAME - 2 * 512 * 7e-9,
        "frames", ("x3", "bf16", "fp32"))
    # the same call on one stream alone (avcer_set_static_lanes(1)): what the two-lane split of 128-512-frame calls buys
    eng.set_static_lanes(1)
    try:
        for name in ("x3", "fp32"):
            for _ in range(2):
                eng.static_forward(frames, modes[name])
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(iters):
                eng.static_forward(frames, modes[name])
            torch.cuda.synchronize(device)
            out["static_b256"][name]["ms_one_lane"] = (time.perf_counter() - t0) / iters * 1e3
    finally:
        eng.set_static_lanes(2)
    out["static_b256"]["lanes_note"] = ("`ms` = the library default: the 256 frames as two half-batches on two HIP streams (bit-identical "
                                        "results); `ms_one_lane` = avcer_set_static_lanes(1); the roofline sub-object comes from a "
                                        "serial evented pass either way")
    del frames
    wav = torch.from_numpy(synth.waveforms(2, 128, T_AUDIO)).to(device)
    run("audio_b128", lambda m: eng.audio_forward(wav, True, m), 128, GFLOP_AUDIO_CHUNK,
        GFLOP_AUDIO_CHUNK - GFLOP_AUDIO_NOT_GEMM, "windows", ("x3", "bf16", "fp32"))
    out["static_b256"]["note"] = ("BASELINE configs[1]; bf16 is reported for reference only: it misses the 1e-4 parity "
                                  "gate (see modes.bf16.max_dprob_vs_cpu_oracle), x3 is the parity-green figure")
    return out


def scripted_detections(n, h, w):
    """One face per frame, drifting slowly (the rows RetinaFacePredictor returns: x0, y0, x1, y1, score, 5 landmarks)."""
    dets = []
    for t in range(n):
        cx, cy = w * (0.5 + 0.15 * np.sin(t / 40.0)), h * (0.5 + 0.1 * np.cos(t / 55.0))
        half = 0.28 * h
        row = np.zeros((1, 15), np.float32)
        row[0, :5] = (cx - 0.8 * half, cy - half, cx + 0.8 * half, cy + half, 0.99)
        dets.append(row)
    return dets


def run_inference_bench(pipe, modes, device, do_cpu, seconds=30, fps=25, h=360, w=640, prefix_s=6):
    """The reference's own run configuration (run.py:190-307): ONE video -- here 30 s at 25 fps, 640 x 360, one tracked face --
    through avcer_amd/run.py: crop -> tile on the GPU, static CNN on every frame, LSTM every 5th, the audio model over 4 s
    windows every 0.5 s (8 x window overlap, 199 tokens, mean padding, the empty tail window), fusion.  Face DETECTION is not
    in it (scripted boxes: synthetic detector weights find no faces; the detector is measured by tools/face_bench.py).
    Reports frames/s and the real-time factor the reference prints (elapsed / video duration, run.py:307) per arithmetic
    mode, the parity of a 6 s prefix against the oracle chain, and the oracle's time for that prefix."""
    from avcer_amd import run as arun
    from avcer_amd.audio_pipeline import chunk_spans

    n = seconds * fps
    frames = torch.from_numpy(synth.video_frames(77, n, h, w)).to(device)
    dets = scripted_detections(n, h, w)
    wav = torch.from_numpy(synth.waveforms(78, 1, seconds * 16000)[0]).to(device)
    eng = pipe.engine
    out = {"video": f"{seconds} s at {fps} fps, {w}x{h} BGR frames + 16 kHz mono, one scripted face track",
           "frames": n, "windows": None, "modes": {},
           "structure": "audio branch queued first on its own HIP stream, then tracker (host) -> crop -> visual branch on the main "
                        "stream, fusion behind both, one range-contract read, every device-to-host copy after the last launch"}

    class DetectorThenScript:
        """Stage 0 in the measured path (get_face_images.py:38-63): the RetinaFace-R50 network over every frame, box decoding
        and the device-side NMS run and their rows come back to the host -- and are then replaced by the scripted boxes,
        because the SYNTHETIC detector weights find no faces (real Resnet50_Final.pth is not in the image)."""

        def __init__(self, det):
            self.det, self.found = det, None

        def batch(self, fr, rgb=False):
            self.found = sum(len(d) for d in self.det.batch(fr, rgb=rgb))
            return dets

    detector = None
    for name in ("x3", "fp32"):
        res = arun.run_inference(eng, frames, wav, fps, detections=dets, mode=modes[name])  # warm-up (workspace growth)
        torch.cuda.synchronize(device)
        dts = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = arun.run_inference(eng, frames, wav, fps, detections=dets, mode=modes[name])
            torch.cuda.synchronize(device)
            dts.append(time.perf_counter() - t0)
        dt = sorted(dts)[1]
        out["windows"] = int(len(chunk_spans(seconds * 16000, 16000, fps, 4, 0.5)[0]))
        out["modes"][name] = {"s": dt, "frames_per_s": n / dt, "real_time_factor": dt / seconds, "dtype": DTYPE[name],
                              "x3_fallbacks_to_fp32": eng.x3_fallbacks}
        if name == "x3":  # the same video with the detector pass in front (stage 0: 51.5 GFLOP per 640 x 360 frame, 7 x the CNN)
            from avcer_amd.face_tiles import RetinaFacePredictor

            if detector is None:
                detector = DetectorThenScript(RetinaFacePredictor(eng, synth.to_torch(synth.retina_state_dict(42)), mode=modes[name]))
            arun.run_inference(eng, frames, wav, fps, detector=detector, mode=modes[name])  # warm-up
            torch.cuda.synchronize(device)
            dts = []
            for _ in range(3):
                t0 = time.perf_counter()
                arun.run_inference(eng, frames, wav, fps, detector=detector, mode=modes[name])
                torch.cuda.synchronize(device)
                dts.append(time.perf_counter() - t0)
            dtd = sorted(dts)[1]
            # stage 0 on its own, with per-family events (serial: nothing else is queued beside it)
            det = detector.det
            det.batch(frames, rgb=False)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            det.batch(frames, rgb=False)
            torch.cuda.synchronize(device)
            det_ms = (time.perf_counter() - t0) * 1e3
            eng.gemm_stats(reset=True)
            eng.profile_enable(True)
            det.batch(frames, rgb=False)
            torch.cuda.synchronize(device)
            fams = eng.profile_read_families()
            eng.profile_enable(False)
            _, det_flops = eng.gemm_stats(reset=True)
            fam_rows, mfma_ms = [], 0.0
            for fam, (ms, n_l, fl, by) in fams.items():
                if not n_l:
                    continue
                mfma_ms += ms
                bound = FAMILY_BOUND.get(fam, "mfma")
                tf, gbs = fl / ms / 1e9, by / ms / 1e6
                ent = {"kernel": fam, "ms": ms, "launches": n_l, "bound": bound, "algorithmic_tflops": tf, "compulsory_gb_per_s": gbs}
                if bound == "hbm":
                    ent.update(achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s", frac=gbs / HBM_PEAK_GBS)
                else:
                    ent.update(achieved=tf, peak=PEAK_FALLBACK["x3"], unit="TFLOP/s", frac=tf / PEAK_FALLBACK["x3"],
                               frac_executed=3 * tf / PEAK_FALLBACK["x3"])
                fam_rows.append(ent)
            out["with_detector"] = {"mode": name, "s": dtd, "frames_per_s": n / dtd, "real_time_factor": dtd / seconds,
                                    "detector": "RetinaFace-R50 network + decode + device NMS over all frames (synthetic weights: "
                                                f"{detector.found} boxes kept -- EVERY prior is a candidate, the worst case of the "
                                                "order + NMS kernels; the scripted track is used behind it)",
                                    "detector_gflop_per_frame": det_flops / n / 1e9,
                                    "detector_alone": {"ms": det_ms, "mfma_kernel_ms": mfma_ms,
                                                       "other_ms": det_ms - mfma_ms,
                                                       "other": "face_pre, max-pool, upsample-add, heads, decode, order, NMS, device-to-host rows",
                                                       "roofline": {"bound": "mfma", "achieved": det_flops / mfma_ms / 1e9, "peak": PEAK_FALLBACK["x3"],
                                                                    "unit": "TFLOP/s", "frac": det_flops / mfma_ms / 1e9 / PEAK_FALLBACK["x3"],
                                                                    "frac_of_peak_executed": 3 * det_flops / mfma_ms / 1e9 / PEAK_FALLBACK["x3"]},
                                                       "per_family": fam_rows}}
    if do_cpu:
        from oracle import audio as oa
        from oracle import face as oface
        from oracle import fusion as of
        from oracle import video as ov

        pn = prefix_s * fps
        pf, pd, pw = frames[:pn].cpu().numpy(), dets[:pn], wav[:prefix_s * 16000].cpu().numpy()
        sds = [synth.to_torch(f(42)) for f in (synth.static_state_dict, synth.dynamic_state_dict, synth.audio_state_dict)]
        t0 = time.perf_counter()
        recs, tiles = oface.process_video(pf, pd)
        rows0 = np.where(recs[:, 1] == 0)[0]
        present = np.zeros(pn, bool)
        present[recs[rows0, 0]] = True
        clip = np.zeros((pn, 224, 224, 3), np.uint8)
        clip[recs[rows0, 0]] = tiles[rows0]
        st, dy = ov.visual_forward(sds[0], sds[1], clip, present, fps, batched=True)
        a_rows, a_frames = oa.audio_forward(sds[2], torch.from_numpy(pw), 16000, fps, 4, 0.5, "mean")
        prob, am = of.fuse(st.astype(np.float32), dy.astype(np.float32), a_rows, a_frames, None, (1, 1, 1), True, False)
        cpu_dt = time.perf_counter() - t0
        worst, same = {}, {}
        for name in ("x3", "fp32"):
            g = arun.run_inference(eng, pf, pw, fps, detections=pd, mode=modes[name])
            worst[name] = max(float(np.abs(g["static_probs"] - st).max()),
                              float(np.abs(of.softmax(g["dynamic_logits"]) - of.softmax(dy.astype(np.float32))).max()),
                              float(np.abs(of.softmax(g["audio_rows"][:, :7]) - of.softmax(a_rows[:, :7])).max()),
                              float(np.abs(g["compound_prob"] - prob).max()))
            same[name] = bool(all(np.array_equal(g[k], am[i]) for i, k in enumerate(("av", "vs", "vd", "a"))) and
                              np.array_equal(g["audio_frames"], a_frames))
            if not (worst[name] < 1e-4 and same[name]):
                raise SystemExit(f"bench.py: run_inference parity FAILED in mode {name}: max|dprob| {worst[name]:.3e}, "
                                 f"argmax / frame table identical: {same[name]}")
        out["parity_prefix"] = {"seconds": prefix_s, "max_dprob_vs_cpu_oracle": worst, "argmax_identical": same, "gate": 1e-4}
        out["cpu_baseline"] = {"s": cpu_dt, "frames_per_s": pn / cpu_dt, "real_time_factor": cpu_dt / prefix_s,
                               "cores": usable_cores(), "kind": "port",
                               "sample": f"the first {prefix_s} s of the same video ({pn} frames batched through the CNN, "
                                         "its 4 s windows one by one), torch-CPU fp32 oracle chain, one pass"}
    return out


def per_call_latency(pipe, modes, device, iters=30):
    """The drop-in mirrors driven the way the reference's own loops drive its models (get_prob_video.py:91-178,
    get_prob_audio_8_cl.py:78-101): ONE frame / LSTM window / 4 s audio window per call.  Milliseconds per call; these
    launches are single-tile latency chains (a HIP graph of the call replays in the same time, tools/graph_probe.py)."""
    from avcer_amd.models import DynamicModel

    x = torch.randn(1, 3, 224, 224, device=device) * 50.0
    win = torch.randn(1, 10, 512, device=device)
    wav = torch.randn(1, 64000, device=device)
    dyn = pipe.dynamic
    out = {}

    def ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) / iters * 1e3

    saved = (pipe.static.mode, pipe.audio.mode, dyn.mode)
    for name in ("x3", "fp32"):
        pipe.static.mode = pipe.audio.mode = dyn.mode = modes[name]
        out[name] = {"static_frame_ms": ms(lambda: pipe.static(x)), "lstm_window_ms": ms(lambda: dyn(win)),
                     "audio_4s_window_ms": ms(lambda: pipe.audio(wav))}
    pipe.static.mode, pipe.audio.mode, dyn.mode = saved
    out["note"] = "one call per frame / window through StaticModel / DynamicModel / AudioModel, as INTEGRATION.md section 3 swaps them in"
    return out


def main():
    args = parse()
    if args.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))  # before any GPU call in this process
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch exactly one rank per GPU")
    # rehearsal on a 1-GPU box: AVCER_BENCH_REHEARSE=1 puts every rank on cuda:0 and uses gloo (CPU) for the collective
    rehearse = os.environ.get("AVCER_BENCH_REHEARSE") == "1" and world > 1
    if rehearse:
        local_rank = 0
    backend = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if not rehearse and torch.cuda.device_count() <= local_rank:
            sys.exit(f"bench.py: rank {rank} has no GPU {local_rank} ({torch.cuda.device_count()} visible)")
        torch.cuda.set_device(local_rank)
        # the collective libraries may greet on fd 1 ("[Gloo] Rank 0 is connected ..."): stdout carries ONE JSON line only
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            if rehearse:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            dist.barrier()
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        backend = dist.get_backend()
        if dist.get_world_size() != args.gpus:
            sys.exit(f"bench.py: process group has {dist.get_world_size()} ranks, expected {args.gpus}")
    device = torch.device("cuda", local_rank)

    from avcer_amd.pipeline import AVPipeline

    modes = {"fp32": MODE_FP32, "bf16": MODE_BF16, "x3": MODE_F16X3}
    pk, pk_src = peaks() if args.full else (None, None)
    torch.set_num_threads(min(usable_cores(), 16))
    log(f"rank {rank}/{world}: building pipeline (synthetic weights, seed 42)")
    pipe = AVPipeline(device=local_rank, seed=42, mode=modes[args.mode])
    if args.no_overlap:
        pipe.overlap_branches = False  # the library default (two streams) is what the headline times
    if args.one_lane:
        pipe.engine.set_static_lanes(1)
    log("generating inputs")
    frames, wav = make_inputs(args.clips, rank, device)
    n_total = args.clips * world

    def set_mode(name):
        pipe.mode = pipe.static.mode = pipe.audio.mode = modes[name]

    def measure(name, steps, warmup):
        set_mode(name)
        log(f"timing {name}: {warmup} warm-up + {steps} steps of {args.clips} clips/GPU")
        dt, kern_ms, launches, serial_dt, per_rank, fams, last = timed(pipe, frames, wav, n_total, steps, warmup, device,
                                                                         profile=args.full and not args.no_events)
        res = {"clips_per_s": n_total * steps / dt, "ms_per_step": dt / steps * 1e3, "per_rank_s": per_rank, "last": last,
               "roofline": None}
        log(f"{name}: {res['clips_per_s']:.1f} clips/s, {res['ms_per_step']:.1f} ms/step")
        if not args.full:
            return res
        per_family = None
        if fams:
            # each family against the roof that bounds it: the fused chains of ResNet stages 1-2 move 2.5-5 KB per position
            # for 100-160 executed FLOP per byte (below the ridge): HBM; everything else: the MFMA peak of the mode
            per_family = []
            for fam, (ms, n_l, fl, by) in fams.items():
                if not n_l:
                    continue
                bound = FAMILY_BOUND.get(fam, "mfma") if name == "x3" else "mfma"
                tf = fl / (ms * 1e-3) / 1e12 if ms else None
                gbs = by / (ms * 1e-3) / 1e9 if ms else None
                ent = {"kernel": fam, "ms_per_step": ms / steps, "launches_per_step": n_l / steps, "bound": bound,
                       "algorithmic_tflops": tf, "compulsory_gb_per_s": gbs}
                if bound == "hbm":
                    ent.update(achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s", frac=gbs / HBM_PEAK_GBS if gbs else None)
                else:
                    ent.update(achieved=tf, peak=pk[name], unit="TFLOP/s", frac=tf / pk[name] if tf else None,
                               frac_executed=tf * MFMA_PASSES[name] / pk[name] if tf else None)
                per_family.append(ent)
        flops_gemm = GFLOP_CLIP_GEMM * 1e9 * args.clips * steps  # algorithmic FLOPs this rank pushed through the MFMA kernels
        ach = flops_gemm / (kern_ms * 1e-3) / 1e12 if kern_ms else None
        traffic, traffic_src, stamp = pmc_traffic(name, args.clips)
        res["roofline"] = {
            "bound": "mfma", "kernel": KERNEL[name], "achieved": ach, "peak": pk[name], "unit": "TFLOP/s",
            "frac": ach / pk[name] if ach else None, "peak_source": pk_src,
            "traffic": traffic, "traffic_unit": "HBM bytes per launch",
            "traffic_source": traffic_src, "traffic_stamp": stamp,
            "mfma_products_per_algorithmic_product": MFMA_PASSES[name],
            "frac_of_peak_executed": ach * MFMA_PASSES[name] / pk[name] if ach else None,
            "launches_per_step": launches / steps if steps else 0,
            "avg_launch_us": kern_ms * 1e3 / launches if launches else None,
            "alg_gflop_per_launch": flops_gemm / launches / 1e9 if launches else None,
            "kernel_time_share": kern_ms * 1e-3 / serial_dt if serial_dt else None,
            "measured_in": f"a separate serial pass of the same {steps} steps (one stream, a HIP-event pair around every "
                           "MFMA-kernel launch) run right after the timed region; the timed region itself carries no "
                           "events" + ("" if args.no_overlap else " and runs the audio branch on a second HIP stream"),
            "serial_evented_ms_per_step": serial_dt / steps * 1e3 if serial_dt else None,
            "per_family": per_family,
            "per_family_note": "same evented pass; compulsory_gb_per_s = every operand read once + every output written once "
                               "(4 bytes per sp32 element) / event time; frac of a family = achieved / peak of ITS bound",
        }
        return res

    head = measure(args.mode, args.steps, args.warmup)
    last = head.pop("last")
    if args.dump_outputs and rank == 0:  # after the all-gather every rank holds the same outputs
        names = dump_outputs(args.dump_outputs, *last)
        log(f"wrote {', '.join(n + '.npy' for n in names)} to {args.dump_outputs}")
    del last
    full = args.full
    rank_check = verify_ranks(pipe, frames, wav, n_total, args.clips, world, rank, device) if full and world > 1 else None
    others = {} if args.no_secondary or not full else {m: measure(m, args.steps, args.warmup) for m in modes if m != args.mode}
    for res in others.values():
        del res["last"]

    if rank == 0:
        cfgs = None if args.no_configs or not full else config_benches(pipe, modes, pk, device)
        do_cpu = full and not args.no_cpu
        gpu_by_mode = {}
        if do_cpu:  # GPU outputs of every measured mode on the parity clips (the first clips of the CPU sample)
            pf, pw = cpu_sample(args.cpu_clips)
            pf, pw = pf[:args.parity_clips], pw[:args.parity_clips]
            for name in [args.mode] + list(others):
                set_mode(name)
                gpu_by_mode[name] = gpu_outputs(pipe, pf, pw)
        set_mode(args.mode)
        base, par = cpu_baseline(args.cpu_clips, gpu_by_mode, args.parity_clips, timed=world == 1) if do_cpu else (None, {})
        dprob, same = par.get(args.mode, (None, None))
        props = torch.cuda.get_device_properties(device)
        meas_mfma = meas_copy = None
        if full:
            try:
                meas_mfma, meas_copy = pipe.engine.measure_ceilings()
            except Exception as exc:  # a diagnostic: never lose the bench line over it
                log(f"measure_ceilings failed: {exc}")
        out = {
            "metric": "clips/sec (224x224x16f + 2s@16kHz), full AV path: static CNN + LSTM + wav2vec2 audio model + fusion",
            "value": head["clips_per_s"], "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE[args.mode], "data": "synthetic", "full": full,
            "config": {"workload": "full AV clips (BASELINE configs[3]/[4]): 16 u8 224x224 RGB face tiles + 32000 f32 "
                                   "samples per clip, synthetic weights (ResNet-50 + LSTM + wav2vec2-large-robust-12 "
                                   "ExprModelV3)", "clips_per_gpu": args.clips, "global_clips": n_total,
                       "frames_per_clip": T_FRAMES, "audio_samples_per_clip": T_AUDIO, "fps": FPS,
                       "static_sub_batch": 1024, "streams": 1 if args.no_overlap else 2, "parallelism": f"clip-sharded x{world} + 1 all-gather of per-clip records"},
            "collective": {"backend": ("rccl (torch nccl)" if backend == "nccl" else backend), "ranks": world,
                           "rehearsal_all_ranks_on_one_gpu": bool(rehearse), "check": rank_check,
                           "per_rank_s": head["per_rank_s"],
                           "per_rank_note": "each rank's own wall time over the K timed steps, before the closing barrier; "
                                            "value = clips / max over ranks of the barrier-to-barrier time"} if world > 1 else None,
            "device": {"name": props.name, "compute_units": props.multi_processor_count,
                       "measured_f16_mfma_tflops": meas_mfma, "measured_hbm_copy_tb_per_s": meas_copy,
                       "measured_note": "register-only v_mfma_f32_16x16x32_f16 loop / 1 GiB streaming copy on this GPU "
                                        "(avcer_measure_ceilings); roofline.peak stays the datasheet figure.  The MFMA kernels "
                                        "run at the socket power cap (tools/clock_probe.py): the loop's rate is what 1.4 kW buys"},
            "kernel_source_hash": kernel_source_hash(),
            "binary_source_hash": pipe.engine.lib.avcer_source_hash().decode(),
            "max_dprob_vs_cpu_oracle": dprob, "argmax_identical": same, "parity_gate": 1e-4,
            "gflop_per_clip": GFLOP_CLIP,
            "gflop_per_clip_reference_graph": GFLOP_CLIP + T_FRAMES * GFLOP_STATIC_UNREAD,
            "gflop_note": "gflop_per_clip (the figure every TFLOP/s here is computed from) leaves out the 0.74 GFLOP per frame of "
                          "conv2 / conv3 outputs of the last block of ResNet stages 1-3 that the reference computes and nothing "
                          "reads (the next stage's 1x1 convolutions have stride 2); the library evaluates those blocks at the "
                          "positions that are read",
            "roofline": head["roofline"],
        }
        if others:
            out["modes"] = {}
            for name, res in others.items():
                d2, s2 = par.get(name, (None, None))
                out["modes"][name] = {"value": res["clips_per_s"], "unit": "clips/s", "ms_per_step": res["ms_per_step"],
                                      "dtype": DTYPE[name], "max_dprob_vs_cpu_oracle": d2, "argmax_identical": s2,
                                      "meets_parity_gate": bool(d2 < 1e-4) if d2 is not None else None,
                                      "roofline": res["roofline"]}
        if cfgs is not None:
            cfgs["per_call_latency"] = per_call_latency(pipe, modes, device)
        if cfgs is not None and not args.no_run_inference:
            log("configs.run_inference: one 30 s video through avcer_amd/run.py")
            cfgs["run_inference"] = run_inference_bench(pipe, modes, device, do_cpu and world == 1)
        if cfgs is not None:
            out["configs"] = cfgs
        if base is not None:
            out["cpu_baseline"] = base
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
