"""Writes tests/golden/jpeg_crops.npz: JPEG byte strings PIL encoded and PIL's own decode of each (libjpeg-turbo), the oracle of
the JPEG crop decoder (csrc/jpeg_decode.hip, avcer_amd/jpeg.py).  Run on a CPU machine: `python tests/golden/make_jpeg_golden.py`.

The GPU tests read this file and never call PIL's JPEG decoder for a supported case -- the libjpeg build of the machine they run
on is not ours to assume.  Keys: `names` [m] (case labels), `handled` [m] bool (False: the four files that must fall back),
`jpg_<i>` u8 (the file), `rgbdx_<i>` u8 [h, w, 3] (absent where PIL raises: the truncated file): Image.open(file).convert("RGB")
with every pixel but the first of a row replaced by its difference from its left neighbour, modulo 256, which the archive's
deflate compresses to half of what the picture itself takes; `np.cumsum(rgbdx, axis=1, dtype=np.uint8)` is the picture again,
exactly (`undo_dx`).  Images are small and smooth (a wave's length grows with the image) so that the archive stays in the range
of the other goldens."""
import io
import os

import numpy as np
from PIL import Image

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (3, 40), (40, 3), (100, 75), (203, 187)]  # (w, h)


def dx(rgb):
    out = rgb.copy()
    out[:, 1:] = rgb[:, 1:] - rgb[:, :-1]  # uint8: modulo 256
    return out


def undo_dx(a):
    return np.cumsum(a, axis=1, dtype=np.uint8)


def content(rng, kind, w, h, mode):
    shape = (h, w, 3) if mode == "RGB" else (h, w)
    if kind == "noise":
        a = rng.integers(0, 256, shape)
    elif kind == "primaries":  # saturated colours in 5 x 5 patches: the colour conversion and the IDCT leave 0..255
        yy, xx = np.mgrid[0:h, 0:w]
        pick = rng.integers(0, 2, ((h + 4) // 5, (w + 4) // 5) + shape[2:]) * 255
        a = pick[yy // 5, xx // 5]
    else:  # smooth: low-frequency waves per channel, a little noise (on a large image only in its first 48 x 48 pixels, so
        # that the decoded picture still compresses in the archive)
        yy, xx = np.mgrid[0:h, 0:w]
        s = max(1.0, max(w, h) / 25.0)  # about one wave across the image, whatever its size
        ch = [np.sin(xx / ((5.0 + 3 * c) * s) + c) * 70 + np.cos(yy / ((7.0 - c) * s)) * 50 + 128 for c in range(3)]
        a = np.stack(ch, axis=2) if mode == "RGB" else ch[0]
        noise = rng.normal(0, 3, shape)
        noise[48:] = 0
        noise[:, 48:] = 0
        a = a + noise
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def encode(a, mode, **kw):
    b = io.BytesIO()
    Image.fromarray(a, mode).save(b, "JPEG", **kw)
    return b.getvalue()


def main():
    rng = np.random.default_rng(20261018)
    cases = []  # (name, bytes, handled)

    def add(name, w, h, mode="RGB", kind="smooth", handled=True, **kw):
        cases.append((name, encode(content(rng, kind, w, h, mode), mode, **kw), handled))

    for w, h in SIZES:
        for sub in (0, 1, 2):
            add(f"{w}x{h}_rgb_s{sub}_q95", w, h, quality=95, subsampling=sub)
        add(f"{w}x{h}_l_q95", w, h, mode="L", quality=95)
    for w, h in ((17, 33), (52, 37)):
        for sub in (0, 1, 2):
            add(f"{w}x{h}_rgb_s{sub}_q75", w, h, quality=75, subsampling=sub)
    for w, h in ((16, 16), (17, 33), (40, 3)):
        for sub in (0, 1, 2):
            for kind in ("noise", "primaries"):
                add(f"{w}x{h}_rgb_s{sub}_q20_{kind}", w, h, kind=kind, quality=20, subsampling=sub)
    add("52x37_l_q20_noise", 52, 37, mode="L", kind="noise", quality=20)
    for sub in (0, 1, 2):
        add(f"52x37_rgb_s{sub}_q95_optimize", 52, 37, quality=95, subsampling=sub, optimize=True)
        add(f"52x37_rgb_s{sub}_q95_rst3", 52, 37, quality=95, subsampling=sub, restart_marker_blocks=3)
        add(f"17x33_rgb_s{sub}_q75_rst3", 17, 33, quality=75, subsampling=sub, restart_marker_blocks=3)
        add(f"52x37_rgb_s{sub}_q95_rstrow", 52, 37, quality=95, subsampling=sub, restart_marker_rows=1)
    add("52x37_l_q95_optimize", 52, 37, mode="L", quality=95, optimize=True)
    add("52x37_l_q95_rst3", 52, 37, mode="L", quality=95, restart_marker_blocks=3)
    add("100x75_rgb_s2_q95_rstrow", 100, 75, quality=95, subsampling=2, restart_marker_rows=1)
    exif = Image.Exif()
    exif[0x010E] = "a face crop"  # ImageDescription
    add("40x40_rgb_s2_q95_exif_comment", 40, 40, quality=95, subsampling=2, exif=exif.tobytes(), comment=b"written by make_jpeg_golden")
    # the four that must fall back
    add("100x75_rgb_progressive", 100, 75, handled=False, quality=95, progressive=True)
    b = io.BytesIO()
    Image.fromarray(content(rng, "smooth", 40, 30, "RGB"), "RGB").save(b, "PNG")
    cases.append(("40x30_png_named_jpg", b.getvalue(), False))
    whole = encode(content(rng, "smooth", 100, 75, "RGB"), "RGB", quality=95)
    cases.append(("100x75_rgb_cut40", whole[:-40], False))
    b = io.BytesIO()
    Image.fromarray(content(rng, "smooth", 40, 30, "RGB"), "RGB").convert("CMYK").save(b, "JPEG", quality=95)
    cases.append(("40x30_cmyk", b.getvalue(), False))

    out = {"names": np.array([c[0] for c in cases]), "handled": np.array([c[2] for c in cases])}
    for i, (name, blob, handled) in enumerate(cases):
        out[f"jpg_{i}"] = np.frombuffer(blob, dtype=np.uint8)
        try:
            with Image.open(io.BytesIO(blob)) as img:
                if handled:
                    assert img.format == "JPEG" and not img.info.get("progressive"), name
                rgb = np.asarray(img.convert("RGB"))
                out[f"rgbdx_{i}"] = dx(rgb)
                assert (undo_dx(out[f"rgbdx_{i}"]) == rgb).all()
        except OSError:
            assert name.endswith("cut40"), name
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_crops.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
