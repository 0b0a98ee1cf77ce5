"""Writes tests/golden/jpeg_encode.npz: small RGB images and the bytes PIL wrote for them (libjpeg-turbo, standard Huffman tables),
the oracle of the JPEG encoder (csrc/jpeg_encode.hip avcer_jpeg_forward / avcer_jpeg_write_batch, avcer_amd/jpeg.py).  Run on a CPU
machine: `python tests/golden/make_jpeg_encode_golden.py`.

Keys: `names` [m], `quality` [m], `subsampling` [m] (PIL's numbering: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), `rgb_<i>` u8 [h, w, 3] and
`jpg_<i>` u8 = Image.fromarray(rgb_<i>).save(f, "JPEG", quality=quality[i], subsampling=subsampling[i]).  The GPU tests hold the
encoder to these bytes; a CPU test first checks that the PIL of the machine it runs on still writes them."""
import io
import os

import numpy as np
from PIL import Image

# (w, h, quality, subsampling, content)
CASES = [(1, 1, 95, 2, "smooth"), (7, 9, 75, 0, "noise"), (7, 9, 20, 2, "bilevel"), (8, 8, 95, 1, "smooth"), (8, 8, 1, 1, "noise"),
         (16, 16, 20, 2, "noise"), (16, 16, 100, 0, "noise"), (17, 33, 95, 2, "smooth"), (17, 33, 75, 1, "bilevel"),
         (52, 37, 95, 2, "smooth"), (52, 37, 1, 0, "bilevel"), (40, 38, 95, 2, "smooth"), (40, 38, 100, 2, "bilevel")]


def content(rng, kind, w, h):
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 3))
    elif kind == "bilevel":
        a = rng.integers(0, 2, (h, w, 3)) * 255
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([np.sin(xx / (5.0 + 3 * c) + c) * 70 + np.cos(yy / (7.0 - c)) * 50 + 128 for c in range(3)], axis=2)
        a = a + rng.normal(0, 3, a.shape)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def encode(rgb, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=int(quality), subsampling=int(subsampling))
    return b.getvalue()


def main():
    rng = np.random.default_rng(20261018)
    out = {"names": np.array([f"{w}x{h}_q{q}_s{s}_{k}" for w, h, q, s, k in CASES]), "quality": np.array([c[2] for c in CASES]),
           "subsampling": np.array([c[3] for c in CASES])}
    for i, (w, h, q, s, kind) in enumerate(CASES):
        out[f"rgb_{i}"] = content(rng, kind, w, h)
        out[f"jpg_{i}"] = np.frombuffer(encode(out[f"rgb_{i}"], q, s), dtype=np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_encode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
