"""Guard bands around a kernel's buffers: a write outside an output, a write to a row the call must
leave alone, and a read outside an input all become failed assertions.

Every buffer is one uint8 allocation of band + payload + band; the payload is handed out as a
contiguous typed view at exactly the size asked for.  BAND is 64 KiB on each side, by condition and
not by measurement: four times the 16 KiB that one 1024-lane workgroup stores with a single
16-byte-per-lane instruction, and a multiple of 512 B, so the payload keeps the allocator's own
alignment (misalign = 4 moves it by exactly 4 bytes, for the entry points that document no alignment
and carry a scalar path).

Outputs (`guarded`): the bands hold BAND_BYTE, the payload is prefilled bytewise with a second
pattern (0x5C: 2.5e17 as fp32, 343 as fp16, 1.5e9 as int32 — no result here equals it).
`assert_bands_intact` compares both bands bytewise, `assert_untouched(rows)` the payload rows the
call must not write (rows at or past a device count, rows outside every segment).

Inputs (`guarded_copy`): the bands, and the rows the call must not read, hold `fill` as values of the
array's own type.  A case runs under two fills A and B, both harmless (floats: NaN and 1e30, FLOAT_FILLS;
indices and counts: two values valid for that array) and `assert_same_bits` compares the two runs'
outputs bytewise: a result that depends on the fill has read what it must not.

Works on CPU tensors as on the device (tests/test_guard_bands_host.py shows on the CPU, with wrong
"kernels" written in torch, that each of these checks fails when it should).  A plain module: no
fixture, marker or pytest setting.
"""
import numpy as np
import torch

BAND = 64 * 1024
BAND_BYTE = 0xA5
PAYLOAD_BYTE = 0x5C
FLOAT_FILLS = (float("nan"), 1e30)


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _row_index(rows, n_rows, device):
    """rows: a bool mask over dim 0, a slice, an int index list / array / tensor -> int64 index tensor."""
    if isinstance(rows, slice):
        return torch.arange(n_rows, device=device)[rows]
    rows = (rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.array(rows))).to(device)
    if rows.dtype == torch.bool:
        assert rows.numel() == n_rows, (rows.numel(), n_rows)
        return torch.nonzero(rows).flatten()
    return rows.long()


class Guarded:
    """Handle of one guarded buffer: `raw` (the uint8 allocation), `data` (the typed payload)."""

    def __init__(self, shape, dtype, device, misalign=0):
        assert misalign in (0, 4), misalign
        if isinstance(shape, int):
            shape = (shape,)
        self.shape = tuple(int(s) for s in shape)
        self.nbytes = _numel(self.shape) * torch.empty((), dtype=dtype).element_size()
        self.misalign = misalign
        self.raw = torch.empty(2 * BAND + misalign + self.nbytes, dtype=torch.uint8, device=device)
        self.lo = BAND + misalign  # payload's first byte
        self.hi = self.lo + self.nbytes  # one past its last
        self.data = self.raw[self.lo:self.hi].view(dtype).view(self.shape)
        self._band = None  # the bands' expected bytes, front then back

    def _bands(self):
        return torch.cat((self.raw[:self.lo], self.raw[self.hi:]))

    def _seal(self):
        self._band = self._bands().clone()

    def _payload_bytes(self):
        rows = self.shape[0] if self.shape else 1
        return self.raw[self.lo:self.hi].view(rows, -1) if self.nbytes else self.raw[self.lo:self.hi].view(rows, 0)

    def assert_bands_intact(self, what="buffer"):
        got = self._bands()
        bad = torch.nonzero(got != self._band).flatten()
        if bad.numel():
            b = int(bad[0])
            where = f"{self.lo - b} B before the start" if b < self.lo else f"{b - self.lo} B past the end"
            raise AssertionError(f"{what}: {bad.numel()} band bytes modified, the first {where}")

    def assert_untouched(self, rows, what="buffer"):
        """The payload rows `rows` (dim 0) still hold the prefill, bytewise."""
        assert self._row_ref is not None, "assert_untouched is for guarded() outputs"
        idx = _row_index(rows, self.shape[0], self.raw.device)
        now, ref = self._payload_bytes()[idx], self._row_ref[idx]
        bad = torch.nonzero((now != ref).any(dim=1)).flatten()
        if bad.numel():
            raise AssertionError(f"{what}: {bad.numel()} rows written that the call must leave alone, "
                                 f"the first row {int(idx[bad[0]])}")

    _row_ref = None


def guarded(shape, dtype, device, fill=PAYLOAD_BYTE, misalign=0):
    """An output buffer: -> (payload, handle).  `fill` is the byte the payload is prefilled with."""
    h = Guarded(shape, dtype, device, misalign)
    h.raw.fill_(BAND_BYTE)
    h.raw[h.lo:h.hi].fill_(int(fill))
    h._seal()
    h._row_ref = h._payload_bytes().clone()
    return h.data, h


def guarded_copy(array, fill, device=None, rows=None, misalign=0):
    """An input buffer holding `array` (numpy array or tensor): -> (payload, handle).  The bands, and
    the payload rows `rows` (those the call must not read; None = none), hold `fill` as values of the
    array's type."""
    src = array.contiguous() if isinstance(array, torch.Tensor) else torch.from_numpy(np.array(array, order="C"))
    device = src.device if device is None else device
    h = Guarded(tuple(src.shape), src.dtype, device, misalign)
    item = src.element_size()
    assert BAND % item == 0
    # (typed fill of the whole allocation from the payload's phase: band elements line up with the payload's)
    whole = h.raw[misalign % item:]
    whole = whole[:whole.numel() // item * item].view(src.dtype)
    whole.fill_(fill)
    if misalign % item:
        h.raw[:misalign % item].fill_(BAND_BYTE)
    tail = (h.raw.numel() - misalign % item) % item
    if tail:
        h.raw[h.raw.numel() - tail:].fill_(BAND_BYTE)
    h.data.copy_(src.to(device))
    if rows is not None:
        idx = _row_index(rows, h.shape[0], h.raw.device)
        if idx.numel():
            h.data[idx] = fill
    h._seal()
    return h.data, h


def same_bits(a, b):
    """Bytewise equality of two tensors (NaN payloads and signed zeros count)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)))


def assert_same_bits(a, b, what="output", why="depends on the fill of memory the call must not read"):
    """The A/B comparison: outputs of the same call under input fill A and under fill B (or, with another
    `why`, any two tensors that must agree bit for bit)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ab = a.contiguous().view(-1).view(torch.uint8)
    bb = b.contiguous().view(-1).view(torch.uint8)
    bad = torch.nonzero(ab != bb).flatten()
    if bad.numel():
        e = torch.unique(bad // a.element_size())
        raise AssertionError(f"{what}: {why} ({bad.numel()} bytes differ, in {e.numel()} of {a.numel()} elements: "
                             f"{e[:8].tolist()}{' ...' if e.numel() > 8 else ''})")
