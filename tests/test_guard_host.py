"""CPU self-tests of tests/guard.py: small Python "kernels" with the bugs the arena exists to catch -- each must be detected, with the right
region named -- and the layout rules (guard size, alignment) over a spread of shapes and dtypes."""
import pytest
import torch

import guard
from guard import Arena, GuardError

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.uint8, torch.int32, torch.int64]
SHAPES = [(1,), (5,), (1, 1), (1, 260), (7, 1), (392, 384), (3, 40000), (2, 3, 5, 7), (), (0, 8)]


def flat_with_guards(arena, t):
    """the allocation behind t as a 1-D tensor of t's dtype, and the index of t's first element in it: lets a Python "kernel" write out of bounds"""
    r = arena._rec_of(t)
    size = t.element_size()
    return r.base.view(t.dtype), r.guard // size


def good_kernel(out, x):
    out.copy_(2 * x)


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_layout_guard_size_alignment_and_poison(dtype, shape):
    a = Arena("cpu")
    t = a.empty(*shape, dtype=dtype)
    r = a._rec_of(t) if t.numel() else a.recs[-1]
    size = t.element_size()
    row = (shape[-1] if shape else 1) * size
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_contiguous()
    assert r.guard >= 64 * 1024 and r.guard >= 2 * row and r.guard % 256 == 0
    assert r.guard == guard.guard_bytes(shape, dtype)
    assert r.base.numel() == 2 * r.guard + t.numel() * size
    if t.numel():
        assert t.data_ptr() % 16 == 0 and t.data_ptr() - r.base.data_ptr() == r.guard
    # the payload and both guards carry the pattern, bit for bit
    view, pat = guard.poison_of(dtype)
    assert bool((r.base.view(view) == pat).all())
    if dtype.is_floating_point and t.numel():
        assert bool(torch.isnan(t).all())         # a value assertion on an unwritten element fails by itself
    a.check()
    if t.numel():
        with pytest.raises(GuardError, match="never written"):
            a.check_written(t)


def test_zeros_like_and_scratch():
    a = Arena("cpu")
    z = a.zeros(5, 12, dtype=torch.bfloat16)
    assert bool((z == 0).all())
    src = torch.arange(35.0).view(5, 7)
    c = a.like(src)
    assert torch.equal(c, src) and c.data_ptr() != src.data_ptr()
    cb = a.like(src, dtype=torch.bfloat16)
    assert cb.dtype == torch.bfloat16 and torch.equal(cb.float(), src)
    s = a.scratch((3, 8), "cpu", torch.float32)
    s1 = a.scratch(24, "cpu", torch.float32)
    assert tuple(s.shape) == (3, 8) and tuple(s1.shape) == (24,) and bool(torch.isnan(s).all())
    for t in (z, c, cb, s, s1):
        assert a._rec_of(t).guard >= 64 * 1024
    a.check()
    a.check_written(z)
    a.check_written(c)


# ------------------------------------------------------------------------------------------------ a correct kernel passes
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_correct_write_passes(dtype):
    a = Arena("cpu")
    x = a.frozen(torch.randn(9, 20).to(dtype))
    out = a.empty(9, 20, dtype=dtype)
    good_kernel(out, x)
    w = a.wide(9, 60, dtype=dtype)
    good_kernel(a.cols(w, 20, 40), x)
    a.check()
    a.check_written(out)
    a.check_written(w[:, 20:40])
    assert torch.equal(out, 2 * x)


# ------------------------------------------------------------------------------------------------ wrong kernels
def test_one_element_past_the_end():
    a = Arena("cpu")
    out = a.empty(6, 10)
    flat, i0 = flat_with_guards(a, out)
    flat[i0:i0 + 61] = 1.0                        # 60 elements + 1
    with pytest.raises(GuardError) as ei:
        a.check()
    msg = str(ei.value)
    assert "trailing guard" in msg and "leading guard" not in msg and "(6, 10)" in msg
    assert "0 bytes past the END" in msg and "1 elements / 4 bytes changed" in msg


def test_one_row_past_the_end():
    a = Arena("cpu")
    out = a.empty(6, 10, dtype=torch.bfloat16)
    flat, i0 = flat_with_guards(a, out)
    flat[i0 + 10:i0 + 70] = 1.0                   # every row stored one row down: row 0 never written, one row beyond the end
    with pytest.raises(GuardError) as ei:
        a.check()
    msg = str(ei.value)
    assert "trailing guard" in msg and "leading guard" not in msg and "10 elements / " in msg and "0 bytes past the END" in msg
    with pytest.raises(GuardError, match=r"10 of 60 elements were never written.*index \(0, 0\)"):
        a.check_written(out)


def test_row_lands_two_rows_past_the_end_is_still_inside_the_guard():
    a = Arena("cpu")
    out = a.empty(4, 40000)                        # rows of 160000 bytes: the guard grows with the row
    flat, i0 = flat_with_guards(a, out)
    flat[i0 + 5 * 40000:i0 + 6 * 40000] = 3.0
    with pytest.raises(GuardError) as ei:
        a.check()
    assert "trailing guard" in str(ei.value) and "(1 rows + 0 bytes past the last element)" in str(ei.value)


def test_write_before_the_start():
    a = Arena("cpu")
    out = a.empty(6, 10)
    flat, i0 = flat_with_guards(a, out)
    flat[i0 - 3:i0 + 60] = 1.0
    with pytest.raises(GuardError) as ei:
        a.check()
    msg = str(ei.value)
    assert "leading guard" in msg and "trailing guard" not in msg and "from 12 to 4 bytes BEFORE the start" in msg and "3 elements / 12 bytes" in msg


def test_skipped_element_and_skipped_row():
    a = Arena("cpu")
    x = torch.randn(8, 16)
    out = a.empty(8, 16)
    good_kernel(out, x)
    view, pat = guard.poison_of(torch.float32)
    out.view(view)[5, 7] = pat                     # "never stored"
    a.check()                                      # (no guard was touched)
    with pytest.raises(GuardError, match=r"1 of 128 elements were never written.*index \(5, 7\)"):
        a.check_written(out)
    assert not (out == 2 * x).all()                # ... and the test's own value comparison fails on the NaN
    out2 = a.empty(8, 16, dtype=torch.bfloat16)
    out2[:7] = 1.0                                 # the last (ragged-edge) row skipped
    with pytest.raises(GuardError, match=r"16 of 128 elements were never written.*index \(7, 0\)"):
        a.check_written(out2)


def test_stale_memory_cannot_hide_a_skipped_store():
    """the situation the arena is for: the same shape asked for twice; the second "launch" skips a row and would find the first one's bits"""
    a = Arena("cpu")
    x = torch.randn(8, 16)
    first = a.empty(8, 16)
    good_kernel(first, x)
    del first
    second = a.empty(8, 16)
    second[1:] = 2 * x[1:]
    assert not torch.equal(second, 2 * x)


def test_neighbouring_column_of_a_wide_buffer():
    a = Arena("cpu")
    w = a.wide(5, 30)
    a.cols(w, 10, 20)
    w[:, 10:20] = 1.0
    a.check()
    w[3, 20] = 1.0                                 # one column too far, in one row
    with pytest.raises(GuardError) as ei:
        a.check()
    msg = str(ei.value)
    assert "untouched columns [20, 30)" in msg and "row 3, column 20" in msg and "untouched columns [0, 10)" not in msg and "guard was" not in msg
    b = Arena("cpu")
    w = b.wide(5, 30, dtype=torch.bfloat16)
    b.cols(w, 0, 12)                               # the n= form: the first n columns
    w[:, :12] = 1.0
    w[0, 29] = 2.0
    with pytest.raises(GuardError, match=r"untouched columns \[12, 30\).*row 0, column 29"):
        b.check()


def test_modified_input():
    a = Arena("cpu")
    x, y = a.frozen(torch.randn(4, 4), torch.arange(6, dtype=torch.int64))
    out = a.empty(4, 4)
    good_kernel(out, x)
    a.check()
    was = x[2, 1].clone()
    x[2, 1] += 1.0
    with pytest.raises(GuardError) as ei:
        a.check()
    msg = str(ei.value)
    assert "input#1" in msg and "frozen input was modified" in msg and "(2, 1)" in msg and "input#2" not in msg and "guard" not in msg
    nan = a.frozen(torch.full((3,), float("nan")))
    x[2, 1] = was                                  # ((v + 1) - 1 is not v bit for bit for most draws of v)
    a.check()                                      # NaN inputs compare by bits, not by value


def test_scratch_overrun_is_reported_as_workspace():
    a = Arena("cpu")
    ws = a.scratch((4, 8), "cpu", torch.float32)
    flat, i0 = flat_with_guards(a, ws)
    flat[i0 + 32] = 0.0
    with pytest.raises(GuardError, match=r"workspace#1 \(4, 8\) float32: trailing guard"):
        a.check()
