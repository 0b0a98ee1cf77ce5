"""Guard bands around kernel outputs: does a kernel write ONLY what it should, and ALL of it?

Every output of the call under test lives inside one larger allocation

    [ front guard | payload | rear guard ]

whose guards are multiples of 256 bytes (the payload keeps the alignment of a fresh tensor) and cover at least 256 rows of the
output each: a whole block tile of round-up past the last row, twice over.  The call runs twice, the whole allocation filled with
byte 0xA5 before the first run and 0x5A before the second -- two patterns that differ in every byte.  `check` asserts that
  1. in each run the guards and every gap element of the payload (an element the call must not write: the columns outside
     [y_coff, y_coff + n) of a strided output, the rows of other levels in a shared tensor) still hold that run's pattern;
  2. the elements the call must write are bit-identical in the two runs -- one it never wrote holds 0xA5.. in one run and 0x5A..
     in the other, so full coverage is proven without a reference;
  3. they are bit-identical, too, to a third run into a fresh tensor of exactly the output's size, which is the configuration the
     parity tests compare with float64;
  4. every input tensor holds the same bits after the runs as before.
A band may name a third kind of element besides "must" and "must not": `may`, the elements a contract leaves unspecified (the
coefficient blocks of a JPEG file that the reader ends up refusing).  They are left out of checks 1 to 3 and of nothing else.
All comparisons are on bytes, so NaN payloads compare like any other.  The module is device-agnostic: tests/test_guard_band_cpu.py
applies it to Python functions on CPU tensors, tests/test_gpu_write_bounds.py to the library's kernels."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

PATTERNS = (0xA5, 0x5A)
GUARD_ROWS = 256


@dataclass
class Band:
    """One output tensor of the call: `shape` elements of `dtype`; `written`: None (every element must be written) or a bool
    tensor that broadcasts to `shape`, True where the call must write, False where it must not (a gap).  `may`: None or a bool
    tensor that broadcasts to `shape`, True where the contract leaves the element unspecified (the call may write it or not, with
    any value); it must not overlap `written`.  `row_bytes`: the bytes of one output row of the case (default: the last dimension),
    which sizes the guards."""
    name: str
    shape: tuple
    dtype: torch.dtype
    written: torch.Tensor | None = None
    row_bytes: int | None = None
    may: torch.Tensor | None = None

    @property
    def itemsize(self) -> int:
        return torch.empty(0, dtype=self.dtype).element_size()

    @property
    def nbytes(self) -> int:
        return math.prod(self.shape) * self.itemsize

    @property
    def guard_bytes(self) -> int:
        row = self.row_bytes if self.row_bytes is not None else self.shape[-1] * self.itemsize
        return (GUARD_ROWS * row + 255) // 256 * 256

    def byte_mask(self) -> torch.Tensor:
        """bool [nbytes] on the CPU: True where the call must write."""
        if self.written is None:
            return torch.ones(self.nbytes, dtype=torch.bool)
        return self.written.cpu().expand(self.shape).reshape(-1).repeat_interleave(self.itemsize)

    def may_mask(self) -> torch.Tensor | None:
        """bool [nbytes] on the CPU: True where the call may write or not; None without `may`."""
        if self.may is None:
            return None
        if self.written is None:
            raise ValueError(f"output '{self.name}': a `may` region needs a `written` mask that leaves it out")
        may = self.may.cpu().expand(self.shape).reshape(-1).repeat_interleave(self.itemsize)
        both = may & self.byte_mask()
        if both.any():
            raise ValueError(f"output '{self.name}': `may` overlaps `written` in {int(both.sum())} bytes, the first at payload "
                             f"byte {_first(both)}")
        return may


def columns(ld: int, off: int, n: int) -> torch.Tensor:
    """The `written` mask of a strided 2-D output: rows of `ld` elements of which [off, off + n) are written."""
    m = torch.zeros(ld, dtype=torch.bool)
    m[off:off + n] = True
    return m


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _first(mask: torch.Tensor) -> int:
    return int(torch.nonzero(mask)[0])


def check(run, bands, inputs=(), device="cpu"):
    """`run(outs)` makes the call under test with `outs[i]` as its i-th output (a tensor of bands[i].shape / dtype).  Raises
    AssertionError with the band, the region and the first offending byte; returns the written payloads of the first run (CPU
    tensors of the bands' shapes; gap elements hold the first pattern)."""
    device = torch.device(device)

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    before = [_bytes(t).clone() for t in inputs]   # (on the CPU _bytes is a view)
    masks = [b.byte_mask() for b in bands]
    mays = [b.may_mask() for b in bands]
    payloads = []
    for run_no, pat in enumerate(PATTERNS):
        bufs, outs = [], []
        for b in bands:
            g = b.guard_bytes
            buf = torch.full((g + b.nbytes + g,), pat, dtype=torch.uint8, device=device)
            bufs.append(buf)
            outs.append(buf[g:g + b.nbytes].view(b.dtype).view(b.shape))
        run(outs)
        sync()
        got = []
        for b, buf, mask, may in zip(bands, bufs, masks, mays):
            g = b.guard_bytes
            raw = buf.cpu()
            row = b.row_bytes if b.row_bytes is not None else b.shape[-1] * b.itemsize
            where = f"output '{b.name}' (run {run_no + 1}, pattern 0x{pat:02X})"
            bad = raw[:g] != pat
            assert not bad.any(), (f"{where}: front guard overwritten: {int(bad.sum())} bytes, the last one "
                                   f"{g - int(torch.nonzero(bad)[-1])} bytes in front of the payload")
            bad = raw[g + b.nbytes:] != pat
            assert not bad.any(), (f"{where}: rear guard overwritten: {int(bad.sum())} bytes, the first one {_first(bad)} bytes "
                                   f"behind the payload (row {b.nbytes // row} + {_first(bad) // row}, byte {_first(bad) % row} of it)")
            pay = raw[g:g + b.nbytes]
            bad = (pay != pat) & ~mask
            if may is not None:
                bad &= ~may
            assert not bad.any(), (f"{where}: {int(bad.sum())} bytes of gap elements overwritten, the first at payload byte "
                                   f"{_first(bad)} (row {_first(bad) // row}, byte {_first(bad) % row} of it)")
            got.append(pay.clone())
        payloads.append(got)
    # a third run into fresh tensors of exactly the outputs' sizes
    exact = [torch.full((b.nbytes,), PATTERNS[0], dtype=torch.uint8, device=device).view(b.dtype).view(b.shape) for b in bands]
    run(exact)
    sync()
    # inputs first: a call that changes one also changes what its later runs compute
    for i, (t, was) in enumerate(zip(inputs, before)):
        bad = _bytes(t) != was
        assert not bad.any(), f"input {i}: {int(bad.sum())} bytes changed by the call, the first at byte {_first(bad)}"
    for i, (b, mask) in enumerate(zip(bands, masks)):
        row = b.row_bytes if b.row_bytes is not None else b.shape[-1] * b.itemsize
        p0, p1, p2 = payloads[0][i], payloads[1][i], _bytes(exact[i])
        bad = (p0 != p1) & mask
        assert not bad.any(), (f"output '{b.name}': {int(bad.sum())} bytes the call must write differ between the two runs (never "
                               f"written, or not deterministic), the first at payload byte {_first(bad)} (row {_first(bad) // row}, "
                               f"byte {_first(bad) % row} of it)")
        bad = (p0 != p2) & mask
        assert not bad.any(), (f"output '{b.name}': {int(bad.sum())} bytes differ between the guarded run and the run into an exactly "
                               f"sized tensor, the first at payload byte {_first(bad)} (row {_first(bad) // row})")
    return [payloads[0][i].view(b.dtype).view(b.shape) for i, b in enumerate(bands)]
