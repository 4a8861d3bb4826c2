"""Control over the contents of memory that no operand defines.

``poisoned(byte)`` is a context manager: inside it ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and
``Tensor.new_empty`` return memory whose every STORAGE byte is ``byte``, whatever the dtype, the strides or the device.  The package
reaches these functions as attributes of ``torch`` at call time, so replacing the attributes is enough; nothing else of torch changes,
and the originals come back on exit, after an exception too.  The object the ``with`` statement binds counts the allocations it filled
(``.filled``), so that a test can assert that the call under test really went through it.

Two fill values, and no others:

* ``0xFF``: every float type reads NaN, every integer type -1 (uint32: 2^32 - 1, as a count of a loop over int32 it is -1 as well);
* ``0x00``: what a fresh device allocation usually holds.

Patterns that read as large positive integers (``0x7F..``, ``0x01010101``) are refused on purpose: a latent bug would turn such a value
into a two-billion-trip loop or a wild address.  With -1 a stray count runs no trips and a stray index lands next to its own buffer.

``stale(run, first, second, new_buffer)`` is the third mode, for entry points whose workspace or partial-tile buffer is a caller-owned
argument: what a buffer last used for ANOTHER input of the same size class leaves behind.
"""
import contextlib

import torch

ALLOWED = (0x00, 0xFF)
_FUNCTIONS = ("empty", "empty_like", "empty_strided")


class Poison:
    def __init__(self, byte):
        self.byte = byte
        self.filled = 0          # allocations filled so far (zero-element tensors are not counted: there is nothing to fill)

    def fill(self, t):
        if isinstance(t, torch.Tensor) and t.numel() > 0:
            raw = torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
            raw.fill_(self.byte)
            self.filled += 1
        return t


@contextlib.contextmanager
def poisoned(byte):
    if byte not in ALLOWED:
        raise ValueError(f"fill byte {byte!r}: only 0x00 and 0xFF are allowed (see the module's docstring)")
    state = Poison(byte)

    def wrap(original):
        def filled(*args, **kwargs):
            return state.fill(original(*args, **kwargs))

        filled.__wrapped__ = original
        return filled

    originals = {name: getattr(torch, name) for name in _FUNCTIONS}
    own_new_empty = torch.Tensor.__dict__.get("new_empty")          # normally inherited from the C base class: nothing of its own
    inherited = torch.Tensor.new_empty
    try:
        for name, original in originals.items():
            setattr(torch, name, wrap(original))
        torch.Tensor.new_empty = lambda self, *args, **kwargs: state.fill(inherited(self, *args, **kwargs))
        yield state
    finally:
        for name, original in originals.items():
            setattr(torch, name, original)
        if own_new_empty is None:
            del torch.Tensor.new_empty
        else:
            torch.Tensor.new_empty = own_new_empty


def stale(run, first, second, new_buffer):
    """``run(x, buffer)`` on ``second`` with the buffer that the call on ``first`` left behind, untouched, and on a zeroed buffer:
    ``(got, want)``.  ``first`` and ``second`` belong to one size class (the same buffer fits both) and differ in exactly the quantities
    the buffer caches.  The first buffer starts with every byte 0xFF, whatever ``new_buffer`` returned: nothing here depends on what an
    allocation happens to hold."""
    buffer = Poison(0xFF).fill(new_buffer())
    run(first, buffer)
    got = run(second, buffer)
    want = run(second, new_buffer().zero_())
    return got, want
