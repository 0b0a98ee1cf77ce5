"""bench.py's command line and its --dump-outputs writer, without a GPU."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), capture_output=True, text=True,
                          timeout=300)


def test_bench_offers_full_and_dump_outputs():
    r = _bench("--help")
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_bench_refuses_zero_steps_before_any_gpu_call():
    """--steps sets the number of timed steps, and ms_per_step is one of them: zero steps would leave it undefined."""
    for argv in (("--steps", "0"), ("--warmup", "-1")):
        r = _bench("--gpus", "1", *argv)
        assert r.returncode != 0 and "--steps must be >= 1" in r.stderr, (argv, r.stderr[-500:])


def test_dump_outputs_writes_the_step_outputs_as_float_arrays(tmp_path):
    import bench

    g = torch.Generator().manual_seed(3)
    prob = torch.rand(4, 10, 16, 7, generator=g, dtype=torch.float64)
    am = prob.argmax(-1).to(torch.int32)
    names = bench.dump_outputs(str(tmp_path / "out"), prob, am)
    assert names == ["compound_argmax", "compound_prob"]
    p = np.load(tmp_path / "out" / "compound_prob.npy")
    a = np.load(tmp_path / "out" / "compound_argmax.npy")
    assert p.dtype == np.float64 and np.array_equal(p, prob.numpy())
    assert a.dtype == np.float32 and np.array_equal(a, am.numpy().astype(np.float32))


def test_dump_outputs_samples_a_fixed_set_of_clips_above_the_limit(tmp_path):
    import bench

    prob = torch.arange(4 * 1000 * 16 * 7, dtype=torch.float64).reshape(4, 1000, 16, 7)
    am = torch.zeros(4, 1000, 16, dtype=torch.int32)
    limit = 600_000  # bytes in all; a clip is 4 * 16 * 7 * 8 + 4 * 16 * 4 (+ 8 for its index) = 3848 bytes
    written = []
    for run in ("a", "b"):
        d = tmp_path / run
        names = bench.dump_outputs(str(d), prob, am, limit=limit)
        assert names == ["clip_index", "compound_argmax", "compound_prob"]
        assert sum(os.path.getsize(d / (n + ".npy")) for n in names) <= limit
        idx = np.load(d / "clip_index.npy")
        p = np.load(d / "compound_prob.npy")
        assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and len(idx) == p.shape[1] > 100
        assert np.array_equal(p, prob.numpy()[:, idx.astype(np.int64)])
        written.append(idx)
    assert np.array_equal(written[0], written[1])  # the same clips every time
