"""Builds and runs tools/jpeg_unpack_asan.hip: avcer_jpeg_scan_batch and avcer_jpeg_unpack_host (csrc/jpeg_unpack.hip: the device entropy
decoder's algorithm as host loops) under AddressSanitizer + UBSan, in a stand-alone program, on a CPU machine (never on the GPU,
never loaded into python).  `python tools/jpeg_unpack_asan.py`."""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from avcer_amd import build  # noqa: E402


def main() -> int:
    import jpeg_unpack_cases as cases

    golden = cases.golden()
    files = [b for _, b in golden + cases.stress()] + [b for _, b, _ in cases.defects(golden)] + [b for _, b in cases.mutants(golden, 60)]
    files.append(b"")  # no bytes at all
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "input.bin"), os.path.join(tmp, "jpeg_unpack_asan")
        with open(data, "wb") as f:
            f.write(np.int32(len(files)).tobytes() + np.array([len(b) for b in files], dtype=np.int64).tobytes() + b"".join(files))
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        cmd = [build._hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + san + [
            os.path.join(build.CSRC, "jpeg_decode.hip"), os.path.join(build.CSRC, "jpeg_unpack.hip"), os.path.join(ROOT, "tools", "jpeg_unpack_asan.hip"), "-fsanitize=address,undefined", "-o", exe]
        subprocess.run(cmd, check=True)
        return subprocess.run([exe, data]).returncode


if __name__ == "__main__":
    sys.exit(main())
