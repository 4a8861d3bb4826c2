"""CPU: tests/poisoned_alloc.py does what a test on poisoned memory relies on -- it fills every storage byte of
every ``torch.empty``-family allocation, it restores torch, and the difference between the 0x00 and the 0xFF run catches an operator
that reads an element it never wrote (and only such an operator)."""
import pytest
import torch

from poisoned_alloc import poisoned, stale

# every dtype the package allocates through the torch.empty family (the outputs, operands, tables, handles, workspaces)
DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8, torch.uint32]


def _bytes(t):
    return torch.tensor([], dtype=torch.uint8).set_(t.untyped_storage())


def _reads_as(t, byte):
    if byte == 0:
        return bool((t == 0).all())
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    if t.dtype == torch.uint8:
        return bool((t == 255).all())
    if t.dtype == torch.uint32:
        return bool((t.view(torch.int32) == -1).all())
    return bool((t == -1).all())


@pytest.mark.parametrize("byte", [0x00, 0xFF])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_the_four_entry_points_are_filled(dtype, byte):
    like = torch.zeros(5, 3, dtype=dtype)
    with poisoned(byte) as p:
        made = [torch.empty(7, 3, dtype=dtype), torch.empty((2, 5), dtype=dtype, device="cpu"), torch.empty_like(like),
                torch.empty_strided((4, 3), (5, 1), dtype=dtype),               # rows of 3 in steps of 5: the gaps are filled too
                like.new_empty(6), like.new_empty((2, 2), dtype=torch.int32)]
        assert p.filled == len(made)
        torch.empty(0, dtype=dtype), torch.empty_like(like[:0]), like.new_empty(0)
        assert p.filled == len(made)                                            # zero elements: skipped, not counted
    for t in made:
        assert bool((_bytes(t) == byte).all()) and _reads_as(t, byte)
    assert made[0].shape == (7, 3) and made[2].shape == like.shape and made[2].dtype == dtype
    assert made[3].stride() == (5, 1) and _bytes(made[3]).numel() == (3 * 5 + 3) * like.element_size()
    assert made[4].dtype == dtype and made[5].dtype == torch.int32               # every other argument passed through


def test_only_the_two_bytes_are_allowed():
    for byte in (0x7F, 0x01, 0x80, -1, 256):
        with pytest.raises(ValueError):
            with poisoned(byte):
                pass


def test_the_originals_come_back_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    own = "new_empty" in torch.Tensor.__dict__
    with pytest.raises(RuntimeError, match="inside"):
        with poisoned(0xFF):
            assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.empty_strided is not before[2]
            raise RuntimeError("inside")
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    assert ("new_empty" in torch.Tensor.__dict__) == own
    with poisoned(0x00):                                                        # and a second use starts from the originals again
        pass
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before


def _broken_prefix_sum(x):
    """Never writes out[0], and reads it."""
    out = torch.empty(x.numel() + 1, dtype=x.dtype)
    for i in range(x.numel()):
        out[i + 1] = out[i] + x[i]
    return out[1:]


def _correct_prefix_sum(x):
    out = torch.empty(x.numel() + 1, dtype=x.dtype)
    out[0] = 0
    for i in range(x.numel()):
        out[i + 1] = out[i] + x[i]
    return out[1:]


def _three_runs(op, x):
    results = [op(x)]
    for byte in (0x00, 0xFF):
        with poisoned(byte) as p:
            results.append(op(x))
        assert p.filled > 0
    return results


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_a_read_of_an_unwritten_element_is_caught(dtype):
    plain, zero, ones = _three_runs(_broken_prefix_sum, torch.arange(1, 6, dtype=dtype))
    assert torch.equal(zero, torch.tensor([1, 3, 6, 10, 15], dtype=dtype))      # on "fresh" memory the bug is invisible
    assert not torch.equal(zero, ones)                                          # NaN / -1 in the element nobody wrote: caught


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_a_correct_operator_is_not_caught(dtype):
    plain, zero, ones = _three_runs(_correct_prefix_sum, torch.arange(1, 6, dtype=dtype))
    assert torch.equal(plain, zero) and torch.equal(zero, ones)


def test_stale_mode_catches_a_buffer_that_caches_the_first_input():
    def cached_max(x, buffer):                   # bug: the running maximum starts from what the buffer holds
        for v in x:
            buffer[0] = torch.maximum(buffer[0], v)
        return buffer[0].clone()

    def own_max(x, buffer):
        buffer[0] = x[0]
        return cached_max(x, buffer)

    new = lambda: torch.empty(1)                 # noqa: E731  (stale itself defines what the first buffer holds: NaN here)
    got, want = stale(cached_max, torch.tensor([9.0, 1.0]), torch.tensor([2.0, 3.0]), new)
    assert float(want) == 3.0 and torch.isnan(got)             # maximum(NaN, v) is NaN: the first call's state leaks into the second
    got, want = stale(cached_max, torch.tensor([9.0, 1.0]), torch.tensor([2.0, 3.0]), lambda: torch.empty(1, dtype=torch.int32))
    assert int(want) == 3 and int(got) == 9                    # integers start at -1: the second call returns the first call's 9
    got, want = stale(own_max, torch.tensor([9.0, 1.0]), torch.tensor([2.0, 3.0]), new)
    assert torch.equal(got, want)
