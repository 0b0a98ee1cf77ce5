"""A plain bench.py run end to end on the GPU: exactly --steps timed steps, the headline line, and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir, clips=8, steps=2, warmup=1):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--clips", str(clips), "--dump-outputs", str(out_dir)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    clips, steps = 8, 2
    line, err = _plain_run(tmp_path / "a", clips, steps)
    assert line["steps"] == steps and line["full"] is False and line["n_gpus"] == 1
    assert line["unit"] == "clips/s" and line["higher_is_better"] is True and line["dtype"].startswith("f16x3")
    assert line["ms_per_step"] > 0 and abs(line["value"] - clips * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    # nothing beyond the headline in a plain run
    assert line["roofline"] is None and line["max_dprob_vs_cpu_oracle"] is None and "modes" not in line
    assert "configs" not in line and "cpu_baseline" not in line
    assert f"1 warm-up + {steps} steps" in err

    prob = np.load(tmp_path / "a" / "compound_prob.npy")
    am = np.load(tmp_path / "a" / "compound_argmax.npy")
    assert sorted(os.listdir(tmp_path / "a")) == ["compound_argmax.npy", "compound_prob.npy"]
    assert prob.dtype == np.float64 and prob.shape == (4, clips, 16, 7)
    assert am.dtype == np.float32 and am.shape == (4, clips, 16)
    assert np.isfinite(prob).all() and (prob >= 0).all() and (prob <= 1 + 1e-9).all()
    assert np.isin(am, np.arange(7)).all()

    # same arguments, same inputs and weights: a second run returns the same outputs
    _plain_run(tmp_path / "b", clips, steps)
    assert np.array_equal(np.load(tmp_path / "b" / "compound_prob.npy"), prob)
    assert np.array_equal(np.load(tmp_path / "b" / "compound_argmax.npy"), am)
