"""The two-pass arena every workspace and weight-copy allocation is sized by (avcer_amd/csrc/arena.h), on the CPU: the header
includes nothing of HIP, so tests/arena_driver.cpp compiles with the host compiler alone."""
import os
import shutil
import subprocess

import pytest

from avcer_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def test_measured_and_bound_carvings_agree(tmp_path):
    """A carving of 0, 1, 255, 256, 257 bytes, a multi-GiB region and a few more: the measuring pass hands out nothing and ends
    where the bound pass ends; bound regions are 256-byte aligned, in order and disjoint, the last ends at the measured size;
    on one byte less of capacity the carving does not end at the capacity, which is how a bound pass fails, and the region that
    no longer fits is null."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "arena_driver")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", build.CSRC, os.path.join(HERE, "arena_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    vals, regions = {}, []
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] == "region":
            regions.append((int(f[1]), int(f[2])))
        else:
            vals[f[0]] = int(f[1])
    sizes = [s for _, s in regions]
    assert sizes[:5] == [0, 1, 255, 256, 257] and max(sizes) > 4 << 30
    assert vals["measuring_null"] == 1
    assert vals["bound_end"] == vals["measured"] == vals["end_exact"]
    base, end = vals["base"], vals["base"]
    for ptr, size in regions:
        assert ptr != 0 and ptr % 256 == 0
        assert end <= ptr < end + 256  # behind the previous region, by less than one alignment unit
        end = ptr + size
    assert end == base + vals["measured"]
    # the measured size is what the layout takes: every size rounded up to 256 except the last
    assert vals["measured"] == sum((s + 255) // 256 * 256 for s in sizes[:-1]) + sizes[-1]
    assert vals["end_short"] != vals["measured"] - 1 and vals["short_last"] == 0
