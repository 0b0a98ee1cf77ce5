"""tests/guard_band.py on plain CPU "kernels" (Python functions on tensors): it passes for a correct function and FAILS for each
kind of error it exists to catch -- a row past the end, an element in front of the start, a gap column, an unwritten payload
element, a modified input.  The GPU cases of tests/test_gpu_write_bounds.py rely on exactly these assertions."""
import pytest
import torch

from guard_band import Band, check, columns

M, N, LD, OFF = 5, 8, 16, 4


def _past(out, rows_before, rows_after):
    """The view a kernel with a wrong bound has: `out`'s rows extended into the storage around it."""
    ld = out.stride(0)
    return out.as_strided((rows_before + out.shape[0] + rows_after, out.shape[1]), (ld, 1), out.storage_offset() - rows_before * ld)


def _good(x):
    def run(outs):
        outs[0][:, OFF:OFF + N] = x * 2 + 1
    return run


def _bands():
    return [Band("y", (M, LD), torch.float32, written=columns(LD, OFF, N))]


def test_a_correct_function_passes():
    x = torch.arange(M * N, dtype=torch.float32).reshape(M, N)
    got, = check(_good(x), _bands(), inputs=[x])
    assert torch.equal(got[:, OFF:OFF + N], x * 2 + 1)
    # dense, two outputs of different types, NaN payload
    def run(outs):
        outs[0][:] = float("nan")
        outs[1][:] = 7
    check(run, [Band("a", (3, 5), torch.float32), Band("b", (11,), torch.int16, row_bytes=2)], inputs=[x])


def test_a_row_past_the_end_fails():
    x = torch.ones(M, N)

    def run(outs):
        _good(x)(outs)
        _past(outs[0], 0, 1)[M, OFF:OFF + N] = 3.0
    with pytest.raises(AssertionError, match="rear guard overwritten"):
        check(run, _bands(), inputs=[x])


def test_a_row_far_past_the_end_but_inside_the_guard_fails():
    """The guard holds 256 rows: a store 255 rows past the end is still seen."""
    x = torch.ones(M, N)

    def run(outs):
        _good(x)(outs)
        _past(outs[0], 0, 256)[M + 255, LD - 1] = 3.0
    with pytest.raises(AssertionError, match="rear guard overwritten"):
        check(run, _bands(), inputs=[x])


def test_an_element_before_the_start_fails():
    x = torch.ones(M, N)

    def run(outs):
        _good(x)(outs)
        _past(outs[0], 1, 0)[0, LD - 1] = 3.0
    with pytest.raises(AssertionError, match="front guard overwritten"):
        check(run, _bands(), inputs=[x])


def test_a_gap_column_fails():
    x = torch.ones(M, N)

    def run(outs):
        _good(x)(outs)
        outs[0][2, OFF + N] = 3.0
    with pytest.raises(AssertionError, match="gap elements overwritten"):
        check(run, _bands(), inputs=[x])


def test_an_unwritten_payload_element_fails():
    x = torch.ones(M, N)

    def run(outs):
        outs[0][:M - 1, OFF:OFF + N] = 3.0
        outs[0][M - 1, OFF:OFF + N - 1] = 3.0          # everything but the last element
    with pytest.raises(AssertionError, match="differ between the two runs"):
        check(run, _bands(), inputs=[x])


def test_a_result_that_depends_on_the_buffer_around_it_fails():
    """Bit identity with the run into an exactly sized tensor: a function whose values depend on where its output lives (here:
    on whether storage precedes it) is caught by the third run."""
    def run(outs):
        outs[0][:, OFF:OFF + N] = 1.0 if outs[0].storage_offset() else 2.0
    with pytest.raises(AssertionError, match="exactly sized"):
        check(run, _bands())


def test_a_modified_input_fails():
    x = torch.ones(M, N)

    def run(outs):
        _good(x)(outs)
        x[1, 1] = 5.0
    with pytest.raises(AssertionError, match="input 0"):
        check(run, _bands(), inputs=[x])


def _may_bands():
    """Row M - 1 of the written columns is unspecified: neither "must" nor "must not"."""
    written = columns(LD, OFF, N).expand(M, LD).clone()
    written[M - 1] = False
    may = torch.zeros(M, LD, dtype=torch.bool)
    may[M - 1, OFF:OFF + N] = True
    return [Band("y", (M, LD), torch.float32, written=written, may=may)]


def _sometimes(x, at):
    """Writes the "must" rows always and element `at` of the last row in every other call, with another value each time."""
    calls = []

    def run(outs):
        outs[0][:M - 1, OFF:OFF + N] = x[:M - 1] * 2 + 1
        calls.append(0)
        if len(calls) % 2:
            outs[0][M - 1, at] = float(len(calls))
    return run


def test_a_may_region_written_in_one_run_and_not_in_the_other_passes():
    x = torch.arange(M * N, dtype=torch.float32).reshape(M, N)
    got, = check(_sometimes(x, OFF + N - 1), _may_bands(), inputs=[x])
    assert torch.equal(got[:M - 1, OFF:OFF + N], x[:M - 1] * 2 + 1)
    # the same function without `may`: the last row is a gap, and the write into it is seen
    bands = _may_bands()
    bands[0].may = None
    with pytest.raises(AssertionError, match="gap elements overwritten"):
        check(_sometimes(x, OFF + N - 1), bands, inputs=[x])


def test_a_write_one_element_outside_the_may_region_fails():
    x = torch.ones(M, N)
    with pytest.raises(AssertionError, match="gap elements overwritten"):
        check(_sometimes(x, OFF + N), _may_bands(), inputs=[x])
    with pytest.raises(AssertionError, match="gap elements overwritten"):
        check(_sometimes(x, OFF - 1), _may_bands(), inputs=[x])


def test_a_may_region_does_not_excuse_an_unwritten_must_element():
    x = torch.ones(M, N)

    def run(outs):
        outs[0][:M - 1, OFF:OFF + N - 1] = 3.0
        outs[0][:M - 2, OFF + N - 1] = 3.0           # row M - 2 lacks its last element
    with pytest.raises(AssertionError, match="differ between the two runs"):
        check(run, _may_bands(), inputs=[x])


def test_a_may_region_that_overlaps_written_is_refused():
    bands = _may_bands()
    bands[0].may = bands[0].may.clone()
    bands[0].may[M - 2, OFF] = True
    with pytest.raises(ValueError, match="overlaps `written`"):
        check(_good(torch.ones(M, N)), bands)
    # written=None is "every element must be written": any `may` overlaps it
    with pytest.raises(ValueError, match="`may`"):
        check(_good(torch.ones(M, N)), [Band("y", (M, LD), torch.float32, may=torch.ones(1, dtype=torch.bool))])


def test_guards_are_aligned_and_cover_256_rows():
    for band in (Band("t", (300, 2048), torch.int16), Band("s", (17, 33), torch.float32), Band("w", (5,), torch.uint8, row_bytes=3)):
        row = band.row_bytes or band.shape[-1] * band.itemsize
        assert band.guard_bytes % 256 == 0 and band.guard_bytes >= 256 * row
    assert Band("t", (300, 2048), torch.int16).guard_bytes == 2 * 128 * 4096   # the stage-3 tail: 128 rows of 4096 bytes, twice
