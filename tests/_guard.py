"""Guarded operands for the op-level entry points: one raw uint8 allocation [front border | payload | back border], every byte
0xFF before anything else happens.  0xFF.. reads as NaN in fp32, bf16 and fp64, so

  * a kernel that LOADS from a border gets a NaN that survives arithmetic (the canary 0xA5A5A5A5 of tests/_abi.py is -2.9e-16 as
    fp32 and would vanish in a sum);
  * a kernel that STORES into a border changes a byte that .check() finds;
  * an output element that is never written reads back as NaN (all_written).

The payload starts 256-byte aligned and is exactly prod(shape) * itemsize bytes; the back border starts at the very next byte.
Each border is at least max(64 KiB, 2 slabs), one slab being everything behind the leading index of the tensor: an overrun by a
row, a plane or a tile still lands inside the allocation (a coverage condition, not a measured number).

Plain helper module (not a conftest); usable with device="cpu" (tests/test_guard_host.py)."""
import numpy as np
import torch

FILL = 0xFF
MIN_BORDER = 64 * 1024


def _prod(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Guarded(object):
    def __init__(self, shape, dtype, values=None, device="cuda", min_border=0):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.shape, self.dtype = shape, dtype
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = _prod(shape) * item
        slab = _prod(shape[1:]) * item
        self.border = max(MIN_BORDER, 2 * slab, int(min_border))
        self.raw = torch.full((self.border + 255 + self.nbytes + self.border,), FILL, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        self.off = ((base + self.border + 255) & ~255) - base
        self.ptr = base + self.off
        self.bytes = self.raw[self.off:self.off + self.nbytes]          # the payload as bytes
        self.tensor = self.bytes.view(dtype).view(shape)                # ... and as the typed tensor
        if values is not None:
            self.set(values)

    def set(self, values):
        if isinstance(values, np.ndarray):
            a = np.ascontiguousarray(values)
            if a.dtype == np.float64 and self.dtype in (torch.float32, torch.bfloat16):
                a = a.astype(np.float32)        # the rounding the rest of the suite applies (fp64 -> fp32 [-> bf16])
            elif not a.flags.writeable:
                a = a.copy()                    # torch.from_numpy wants a writable array; the caller's stays read-only
            values = torch.from_numpy(a)
        self.tensor.copy_(values.reshape(self.shape).to(self.dtype))
        return self

    def fill(self, byte):
        """Every payload byte = `byte` (scratch buffers: 0x00 and 0xFF must give the same results)."""
        self.bytes.fill_(byte)
        return self

    def borders(self):
        return self.raw[:self.off], self.raw[self.off + self.nbytes:]

    def check(self, name):
        """Synchronises; both borders must still be all 0xFF."""
        if self.raw.is_cuda:
            torch.cuda.synchronize()
        for side, b in zip(("front", "back"), self.borders()):
            bad = b != FILL
            if bool(bad.any().item()):
                idx = torch.nonzero(bad).reshape(-1)
                first, last, cnt = int(idx[0].item()), int(idx[-1].item()), int(idx.numel())
                where = first - int(b.numel()) if side == "front" else first
                raise AssertionError("%s: %s border changed: %d bytes, first at payload %s %d, span %d bytes" % (
                    name, side, cnt, "start" if side == "front" else "end +", where, last - first + 1))

    def numpy(self):
        t = self.tensor
        return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def all_written(t, name="output"):
    """No element of an output payload still holds the NaN it was created with."""
    t = t.tensor if isinstance(t, Guarded) else t
    nan = torch.isnan(t.float() if t.dtype == torch.bfloat16 else t)
    n = int(nan.sum().item())
    assert n == 0, "%s: %d of %d elements never written (or NaN), first at flat index %d" % (
        name, n, nan.numel(), int(torch.nonzero(nan.reshape(-1))[0].item()))
