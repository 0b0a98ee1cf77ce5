"""`PIL.Image.resize` of whole RGB frames on the device, bit for bit, for PIL's convolution filters.

What the detector path needs in front of it when it runs on a smaller copy of the frames (face_tiles.ScaledDetector): an
anti-aliased resize of a frame batch.  The claim is identity with PIL (Pillow's Resample.c, 8 bits per channel, the default `box`
and `reducing_gap=None`) at tolerance zero for "box", "bilinear", "bicubic" and "lanczos"; HAMMING (its C source mixes float
literals into the window) and NEAREST are not covered, and cv2's INTER_AREA / INTER_LINEAR give other pixels and are not claimed.

  * resize_plan    the coefficient table of one axis, built in double exactly as precompute_coeffs / normalize_coeffs_8bpc do
  * resize_numpy   the CPU statement of the arithmetic from those same tables (what the kernel is tested against)
  * resize_frames  the device call (Engine.resize_frames, csrc/resize.hip)

Per axis with `in` source and `out` output pixels: scale = in / out, fs = max(scale, 1), support = S * fs (S = 0.5 / 1 / 2 / 3),
ksize = ceil(support) * 2 + 1; for output xx: center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0),
xmax = min(int(center + support + 0.5), in), k[x] = F((x + xmin - center + 0.5) / fs) for x < xmax - xmin, divided by their running
sum in x order when that is not zero; kk = int(+-0.5 + k * 2^22) (truncating); the output is
clip(((1 << 21) + sum_j src[xmin + j] * kk[j]) >> 22, 0, 255) in int32.  Horizontal pass first, then vertical, a u8 image between
them; a pass whose axis keeps its size is skipped.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

PRECISION_BITS = 22       # Resample.c: 32 - 8 - 2
MAX_SIDE = 8192           # include/avcer_hip.h AVCER_RESIZE_MAX_SIDE
FORM_CHOOSE, FORM_FUSED, FORM_TWO_PASS = 0, 1, 2   # include/avcer_hip.h AVCER_RESIZE_*


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (window, support); math.sin is the C library's, as in Resample.c (numpy's vectorised sin may differ in the last bit)
FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def check_filter(name) -> str:
    if not isinstance(name, str) or name not in FILTERS:
        extra = f" ({name!r} is not covered: its result differs from PIL's)" if name in ("hamming", "nearest") else ""
        raise ValueError(f'resize filter must be one of "box", "bilinear", "bicubic", "lanczos", not {name!r}{extra}')
    return name


@dataclass(frozen=True)
class ResizePlan:
    """The table of one axis: first / count int32 [out], kk int32 [out, ksize] (zero behind count)."""
    in_size: int
    out_size: int
    filter: str
    ksize: int
    first: np.ndarray
    count: np.ndarray
    kk: np.ndarray

    def packed(self) -> np.ndarray:
        """int32 [out * (2 + ksize)]: first, count, kk back to back -- what avcer_resize_frames takes."""
        return np.ascontiguousarray(np.concatenate([self.first, self.count, self.kk.reshape(-1)]).astype(np.int32))


def _check_side(v, what) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_SIDE:
        raise ValueError(f"resize: {what} must be an integer in 1..{MAX_SIDE}, not {v!r}")
    return int(v)


def resize_plan(in_size: int, out_size: int, filter: str = "bilinear") -> ResizePlan:
    """The coefficient table of one axis (module docstring), cached per (in, out, filter).  in == out: PIL skips the pass, and the
    plan is the identity (one tap of 2^22 per output, which reproduces the input bit for bit), so that the kernel needs no special
    case.  ValueError for a filter other than the four, naming them, and for a side outside 1..8192."""
    return _plan(_check_side(in_size, "in_size"), _check_side(out_size, "out_size"), check_filter(filter))


@lru_cache(maxsize=64)
def _plan(in_size: int, out_size: int, name: str) -> ResizePlan:
    if in_size == out_size:
        first = np.arange(out_size, dtype=np.int32)
        plan = ResizePlan(in_size, out_size, name, 1, first, np.ones(out_size, np.int32), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32))
    else:
        f, sup = FILTERS[name]
        scale = in_size / out_size
        fs = max(scale, 1.0)
        support = sup * fs
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / fs
        first = np.zeros(out_size, np.int32)
        count = np.zeros(out_size, np.int32)
        kk = np.zeros((out_size, ksize), np.int32)
        one = float(1 << PRECISION_BITS)
        for xx in range(out_size):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), in_size)
            k = [f((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
            ww = 0.0
            for w in k:
                ww += w
            if ww != 0.0:
                k = [w / ww for w in k]
            kk[xx, :len(k)] = [int(-0.5 + w * one) if w < 0 else int(0.5 + w * one) for w in k]
            first[xx], count[xx] = xmin, len(k)
        plan = ResizePlan(in_size, out_size, name, ksize, first, count, kk)
    for a in (plan.first, plan.count, plan.kk):
        a.setflags(write=False)
    return plan


def _pass(img: np.ndarray, plan: ResizePlan, axis: int) -> np.ndarray:
    x = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((plan.out_size,) + x.shape[1:], np.uint8)
    for o in range(plan.out_size):
        a, n = int(plan.first[o]), int(plan.count[o])
        acc = np.tensordot(plan.kk[o, :n].astype(np.int64), x[a:a + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)   # >> on int64 is arithmetic; the sums fit int32 (Resample.c's type)
    return np.moveaxis(out, 0, axis)


def _check_size(size):
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError(f"resize: size must be (height, width), not {size!r}")
    return _check_side(size[0], "height"), _check_side(size[1], "width")


def resize_numpy(img, size, filter: str = "bilinear") -> np.ndarray:
    """u8 [H,W,3] or [n,H,W,3] -> [.., size[0], size[1], 3] = np.asarray(Image.fromarray(img).resize((size[1], size[0]), F)), computed
    from resize_plan's tables: the horizontal pass when the width changes, then the vertical pass when the height changes."""
    h2, w2 = _check_size(size)
    check_filter(filter)
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (3, 4) or img.shape[-1] != 3:
        raise ValueError("resize_numpy: uint8 [H,W,3] or [n,H,W,3]")
    ya, xa = img.ndim - 3, img.ndim - 2
    if img.shape[xa] != w2:
        img = _pass(img, resize_plan(img.shape[xa], w2, filter), xa)
    if img.shape[ya] != h2:
        img = _pass(img, resize_plan(img.shape[ya], h2, filter), ya)
    return np.ascontiguousarray(img)


def resize_frames(engine, frames, size, filter: str = "bilinear"):
    """frames u8 [n,H,W,3] -> u8 [n,size[0],size[1],3] on the device, PIL's Image.resize of every frame (Engine.resize_frames).  A batch
    that already has that size comes back as it is, with no launch."""
    return engine.resize_frames(frames, size, filter)


def target_size(height: int, width: int, size):
    """The `size` of ScaledDetector / detect_size for frames of height x width -> (h2, w2).  (height, width): as given.  An int n:
    the longest side becomes n, h2 = max(1, int(H * n / max(H, W) + 0.5)) and likewise w2.  Anything else raises ValueError."""
    if isinstance(size, (bool, np.bool_)):
        raise ValueError(f"detect size must be (height, width) or an int (the longest side), not {size!r}")
    if isinstance(size, (int, np.integer)):
        if size < 1:
            raise ValueError(f"detect size must be >= 1, not {size!r}")
        m = max(height, width)
        return max(1, int(height * int(size) / m + 0.5)), max(1, int(width * int(size) / m + 0.5))
    if isinstance(size, (tuple, list)) and len(size) == 2 and all(
            isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v >= 1 for v in size):
        return int(size[0]), int(size[1])
    raise ValueError(f"detect size must be (height, width) or an int (the longest side), not {size!r}")
