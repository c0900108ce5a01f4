"""Guarded allocations for the GPU tests: every output is the middle of a larger buffer of 0xFF
bytes (a NaN in bf16 and fp32, no window byte), so a store past an output's end changes a byte
that ``check`` looks at, and an element nobody wrote still holds the fill."""
import torch

GUARD = 4096


class GuardedTorch:
    """Stands in for ``torch`` inside ops/encoder.py: every torch.empty there, and every output
    the tests allocate, is the middle of a larger buffer of 0xFF bytes."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None, interior=None):
        """interior (default: every dtype but fp32): check() also asserts that no fill is left
        inside; False for outputs with row gaps that must keep it."""
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        nbytes = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            nbytes *= int(s)
        raw = torch.full((2 * GUARD + (nbytes + 255) // 256 * 256,), 0xFF, dtype=torch.uint8,
                         device=device)
        t = raw[GUARD:GUARD + nbytes].view(dtype).view(*shape)
        # (fp32: the encoder's partial-row workspace, sized for the largest batch, is not an
        # output; the fp32 outputs dW / db are checked by the caller)
        self.bufs.append((raw, nbytes, t, dtype != torch.float32 if interior is None else interior))
        return t

    def empty_like(self, t):
        return self.empty(*t.shape, dtype=t.dtype, device=t.device)

    def check(self):
        torch.cuda.synchronize()
        for raw, nbytes, t, interior in self.bufs:
            assert bool((raw[:GUARD] == 0xFF).all()) and bool((raw[GUARD + nbytes:] == 0xFF).all()), \
                f"write outside an output of shape {tuple(t.shape)}"
            if interior:
                filled(t)
        self.bufs = []


def filled(t):
    """No 0xFF fill pattern is left inside output t."""
    if t.dtype == torch.uint8:
        assert bool((t <= 8).all()), "window byte not written"
    else:
        assert not bool(torch.isnan(t).any()), "output element not written"


def untouched(t):
    """Every byte of t still holds the fill."""
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())
