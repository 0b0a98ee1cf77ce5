"""The JPEG round trip stated in numpy (avcer_amd/jpeg.py roundtrip_numpy = pixels_numpy(forward_numpy(...))) against PIL's own
round trip -- Image.save(buf, "JPEG", quality, subsampling), then Image.open(buf).convert("RGB") -- pixel for pixel, no tolerance.
It is the statement the device path (tests/test_gpu_jpeg_roundtrip.py) is held to where PIL itself is not called.

Sizes (w x h): a single pixel (1x1), a partial MCU in each direction (1x17, 9x7, 17x15, 33x47), whole blocks (8x8, 16x16), odd
chroma sizes (9x7, 17x15, 33x47: ceil(w / 2) and ceil(h / 2) odd) and an image wider and taller than one 224-sample stride
(250x301)."""
import io

import numpy as np
import pytest
from PIL import Image

from avcer_amd import jpeg

SIZES = [(1, 1), (1, 17), (8, 8), (9, 7), (16, 16), (17, 15), (33, 47), (250, 301)]
SUBSAMPLINGS = [0, 1, 2]
QUALITIES = [1, 50, 95, 100]


def images():
    """Per size a seeded uniform u8 noise image and a smooth gradient, [(name, rgb u8 [h, w, 3])]."""
    rng = np.random.default_rng(20261019)
    out = []
    for w, h in SIZES:
        out.append((f"noise {w}x{h}", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
        yy, xx = np.mgrid[0:h, 0:w]
        g = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(w + h - 2, 1)], axis=2)
        out.append((f"gradient {w}x{h}", np.rint(g).astype(np.uint8)))
    return out


def pil_roundtrip(rgb, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, "JPEG", quality=int(quality), subsampling=int(subsampling))
    buf.seek(0)
    with Image.open(buf) as img:
        return np.array(img.convert("RGB"))


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_roundtrip_numpy_is_pils_round_trip(subsampling, quality):
    named = images()
    got = jpeg.roundtrip_numpy([im for _, im in named], quality=quality, subsampling=subsampling)
    assert len(got) == len(named)
    for (name, im), g in zip(named, got):
        assert g is not None, f"{name} q{quality} s{subsampling}: the range guard fired on an encoder's own coefficients"
        np.testing.assert_array_equal(g, pil_roundtrip(im, quality, subsampling), err_msg=f"{name} q{quality} s{subsampling}")


def test_roundtrip_numpy_is_the_composition_of_the_two_statements():
    named = images()[:6]
    coeffs, desc = jpeg.forward_numpy([im for _, im in named], 95, 2)
    for a, b in zip(jpeg.roundtrip_numpy([im for _, im in named]), jpeg.pixels_numpy(coeffs, desc)):
        np.testing.assert_array_equal(a, b)
