"""The guard-frame harness of the stride tests (tests/frames.py) tested on its own, on the CPU: a stand-in "kernel" that writes exactly the
window passes, stand-ins that write anything more fail with the right location in the message, and the fixed layout list reaches every
store class the GEMMs' selector can return for each N the GPU tests use - the condition that keeps tests/test_gpu_strides.py from leaving a
store path out without saying so."""
import re

import pytest
import torch

from frames import GUARD_ROWS, LAYOUTS, Frame, classes_possible, layout_ptr, store_class
from mixq_amd import _capi

TEST_N = [1000, 1004, 256]        # the output widths of tests/test_gpu_strides.py (and 584 / 2 = 292 columns for the joint gate / up form)


def _frame(dtype=torch.float16, rows=5, cols=24, ld=40, col_off=8, elem_off=4, guard_rows=3):
    return Frame(rows, cols, ld, col_off, elem_off, dtype, "cpu", guard_rows)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.int32, torch.uint8])
def test_a_writer_of_exactly_the_window_passes(dtype):
    f = _frame(dtype)
    assert tuple(f.view.shape) == (5, 24) and f.view.stride() == (40, 1) and f.view.dtype == dtype
    es = f.view.element_size()
    assert (f.view.data_ptr() - (8 + 4) * es) % 256 == 0                     # column col_off of a grid elem_off elements behind a boundary
    f.assert_untouched("nothing ran")
    f.view.copy_(torch.ones(5, 24).to(dtype))                                   # the stand-in kernel
    f.assert_untouched("exact writer")
    # the guard: guard_rows full rows in front and behind, and the pad columns, all hold the position-dependent pattern
    assert f.start - 8 - 4 >= 3 * 40 and f.flat.numel() - (f.start - 8 + 5 * 40) >= 3 * 40
    if es == 2:
        g = f.flat.view(torch.int16)
        assert int((g[1:] == g[:-1]).sum()) <= 5 * 24                        # (no two neighbours equal outside what was written)


def _fails(f, what):
    with pytest.raises(AssertionError) as e:
        f.assert_untouched(what)
    msg = str(e.value)
    assert msg.startswith(what)
    m = re.search(r"(\d+) element\(s\).*first at \(row (-?\d+), column (\d+)\)", msg)
    assert m, msg
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def test_eight_elements_past_the_last_column_of_one_row_are_seen():
    f = _frame()
    f.view.fill_(1.0)
    f.flat[f.start + 2 * f.ld + f.cols: f.start + 2 * f.ld + f.cols + 8] = 1.0          # row 2, columns cols .. cols + 7
    assert _fails(f, "past N") == (8, 2, 24)


def test_a_write_to_row_rows_is_seen():
    f = _frame()
    f.view.fill_(1.0)
    f.flat[f.start + 5 * f.ld + 3] = 0.0
    assert _fails(f, "row M") == (1, 5, 3)


def test_a_write_to_the_row_before_the_window_is_seen():
    f = _frame()
    f.flat[f.start - f.ld: f.start - f.ld + 24] = 2.0
    assert _fails(f, "row -1") == (24, -1, 0)


def test_a_write_to_the_last_guard_element_of_the_buffer_is_seen():
    f = _frame()
    f.flat[-1] = 0.0
    count, row, col = _fails(f, "last element")
    rel = f.flat.numel() - 1 - f.start
    assert (count, row, col) == (1, rel // f.ld, rel % f.ld) and row >= f.rows + 3 - 1


@pytest.mark.parametrize("value", [0.0, 1.0, float("nan"), -2.5])
def test_the_same_value_everywhere_is_seen(value):
    """A kernel that clears or floods the buffer with ANY constant changes almost every guard element: the pattern is position-dependent."""
    f = _frame()
    f.flat.fill_(value)
    count, row, col = _fails(f, "flood")
    outside = f.flat.numel() - 5 * 24
    assert count >= outside - 2 and (row, col) == ((0 - f.start) // f.ld, (0 - f.start) % f.ld)


def test_a_stray_write_inside_a_four_byte_frame_is_seen():
    f = _frame(torch.int32, rows=1, cols=17, ld=32, col_off=0, elem_off=0)
    f.view.zero_()
    f.flat[f.start + 17] = 0                                                 # entry M of a row_amax buffer of M live entries
    assert _fails(f, "row_amax[M]") == (1, 0, 17)


def test_guard_rows_cover_the_tallest_tile():
    tallest = 0
    for name in _capi.gemm_config_names() + _capi.w8a16_config_names():
        m = re.search(r"(\d+)x(\d+)", name)
        if m:
            tallest = max(tallest, int(m.group(1)))
    assert 0 < tallest <= GUARD_ROWS


def test_store_class_restates_the_selector():
    assert store_class(1000, 1000, 0) == "staged" and store_class(1000, 1008, 256) == "staged"
    assert store_class(1004, 1008, 0) == "unstaged_by_N"
    assert store_class(1000, 1004, 0) == "unstaged_by_ld"
    assert store_class(1000, 1008, 8) == "unstaged_by_ptr"
    for N in (8, 64, 292, 1000, 1004):
        for ld in (N, N + 4, N + 8):
            for ptr in (0, 8, 16):
                staged = N % 8 == 0 and ld % 8 == 0 and ptr % 16 == 0
                assert (store_class(N, ld, ptr) == "staged") == staged


@pytest.mark.parametrize("N", TEST_N + [292])
def test_the_layout_list_reaches_every_store_class(N):
    layouts = LAYOUTS(N)
    assert layouts == [(N, 0, 0), (N + 8, 0, 0), (2 * N + 64, N + 8, 0), (N + 4, 0, 0), (N + 8, 0, 4), (N + 4, 4, 0)]
    got = set()
    for ld, col_off, elem_off in layouts:
        assert ld % 4 == 0 and ld >= col_off + N                              # what the entry points accept
        f = Frame(2, N, ld, col_off, elem_off, torch.float16, "cpu", 2)
        assert f.view.data_ptr() % 8 == 0                                     # ... and never a base below the documented 8 bytes
        assert f.view.data_ptr() % 256 == layout_ptr((ld, col_off, elem_off))
        got.add(store_class(N, ld, f.view.data_ptr()))
    assert got == classes_possible(N), (N, got)
    assert classes_possible(N) == {store_class(N, ld, p) for ld in range(N, N + 16, 4) for p in (0, 8)}
