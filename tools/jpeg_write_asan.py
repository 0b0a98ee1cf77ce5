"""Builds and runs tools/jpeg_write_asan.hip: the host code of csrc/jpeg_encode.hip under AddressSanitizer + UBSan, in a stand-alone
program, on a CPU machine (never on the GPU, never loaded into python).  `python tools/jpeg_write_asan.py`."""
from __future__ import annotations

import io
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avcer_amd import build, jpeg  # noqa: E402


def main() -> int:
    from PIL import Image

    rng = np.random.default_rng(53)
    quality, subsampling = 95, 2
    images = []
    for t, (w, h) in enumerate([(1, 1), (17, 33), (40, 38), (52, 37), (8, 8), (69, 5), (200, 200), (33, 64)]):
        a = rng.integers(0, 256, (h, w, 3)) if t % 2 else rng.integers(0, 2, (h, w, 3)) * 255  # noise and bilevel: long codes, 0xFF bytes
        images.append(a.astype(np.uint8))
    coeffs, _ = jpeg.forward_numpy(images, quality, subsampling)
    files = []
    for a in images:
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=subsampling)
        files.append(b.getvalue())
    blob = b"".join(files)
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "input.bin"), os.path.join(tmp, "jpeg_write_asan")
        with open(data, "wb") as f:
            f.write(np.array([len(images), quality, subsampling], dtype=np.int32).tobytes())
            f.write(np.array([(a.shape[1], a.shape[0]) for a in images], dtype=np.int32).tobytes())
            f.write(np.int64(coeffs.size).tobytes() + coeffs.tobytes() + np.int64(len(blob)).tobytes() + blob)
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        cmd = [build._hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + san + [
            os.path.join(build.CSRC, "jpeg_encode.hip"), os.path.join(build.CSRC, "jpeg_decode.hip"), os.path.join(ROOT, "tools", "jpeg_write_asan.hip"), "-fsanitize=address,undefined", "-o", exe]
        subprocess.run(cmd, check=True)
        return subprocess.run([exe, data]).returncode


if __name__ == "__main__":
    sys.exit(main())
