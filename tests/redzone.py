"""Test helper: guarded buffers, so that a kernel's WRITE outside an output -- or READ past an operand -- shows in a test.

conftest.py poisons free memory, which turns a read of memory nobody wrote into a NaN.  A write past an output, past the advertised
workspace or into a neighbour's padding lands in some other tensor, and no assertion looks there.  Here every output / workspace of a
test is a view into the middle of a larger allocation the test owns:

    [ margin: sentinel words | body (the tensor the kernel gets) | slack | margin: sentinel words ]

`guarded()` returns the body; `Guard.check()` (or `check()` for all live guards of a `Zone`) synchronizes and asserts that both margins
still hold the sentinel, bit for bit, naming the first damaged byte offset relative to the body.  The body of an output is pre-filled
with NaN, so an element the kernel should have written and did not is a NaN in the comparison that follows.

`at_end_of_poison()` places an input so that its last byte is followed by a NaN margin (what test_dgrad_x3_with_fused_batchnorm_sums
does by hand): a read past the operand's end becomes a NaN in the result.

The margins are ordinary memory of the test; nothing here provokes a fault.  No GPU kernels of its own: torch fills and compares.
"""
import torch

MARGIN = 64 << 10                 # bytes on either side (the widest row stride of the guarded outputs, 6890 * 3 * 4 B, fits 0.79 times)
ALIGN = 256                       # the body starts on a 256-byte boundary, as a tensor of the caching allocator would
SENTINEL = 0x7FC0BEEF             # a quiet-NaN bit pattern with a payload, as int32: a stray READ of a margin is a NaN as well


class Guard:
    """one guarded allocation; `.view` is the tensor handed to the kernel."""

    def __init__(self, shape, dtype=torch.float32, device='cpu', fill=float('nan'), margin=MARGIN, name=''):
        assert margin % ALIGN == 0 and margin > 0
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        esz = torch.empty((), dtype=dtype).element_size()
        self.nbytes = n * esz
        body = (self.nbytes + 3) // 4 * 4                             # margins are compared as int32 words
        total = ALIGN + margin + body + margin
        self.base = torch.full((total // 4,), SENTINEL, dtype=torch.int32, device=device)
        skew = (-(self.base.data_ptr() + margin)) % ALIGN             # bytes to the next boundary at which the body may start
        assert skew % 4 == 0
        self.lo = (skew + margin) // 4                                # body's first word
        self.hi = self.lo + body // 4                                 # first word behind the body
        self.name, self.margin = name, margin
        self.view = self.base[self.lo:self.hi].view(torch.uint8)[:self.nbytes].view(dtype).view(shape)
        assert self.view.data_ptr() % ALIGN == 0
        if fill is not None and n:
            self.view.fill_(fill)

    def damage(self):
        """-> None, or (byte offset relative to the body's first byte, word found) of the first damaged margin word."""
        if self.base.is_cuda:
            torch.cuda.synchronize(self.base.device)
        for start, stop in ((0, self.lo), (self.hi, self.base.numel())):
            bad = (self.base[start:stop] != SENTINEL).nonzero()
            if bad.numel():
                w = start + int(bad[0])
                return (w - self.lo) * 4, int(self.base[w]) & 0xFFFFFFFF
        return None

    def check(self):
        d = self.damage()
        assert d is None, ('redzone %r (%d bytes): a margin word was overwritten at byte offset %d from the start of the buffer '
                           '(%s), found 0x%08x' % (self.name, self.nbytes, d[0],
                                                   '%d bytes before it' % -d[0] if d[0] < 0 else '%d bytes past its end' % (d[0] - self.nbytes), d[1]))


class Zone:
    """the guards of one test: z.guarded(...) like the module function, z.check() checks them all."""

    def __init__(self, device):
        self.device, self.guards = device, []

    def guarded(self, shape, dtype=torch.float32, fill=float('nan'), margin=MARGIN, name=''):
        g = Guard(shape, dtype, self.device, fill, margin, name or 'buffer %d' % len(self.guards))
        self.guards.append(g)
        return g.view

    def at_end(self, t):
        return at_end_of_poison(t, self.device)

    def check(self):
        for g in self.guards:
            g.check()


_LIVE = []


def guarded(shape, dtype=torch.float32, device='cpu', fill=float('nan'), margin=MARGIN, name=''):
    """-> a `shape` view (256-byte aligned) into the middle of a larger allocation whose margins hold SENTINEL; registered for check()."""
    g = Guard(shape, dtype, device, fill, margin, name or 'buffer %d' % len(_LIVE))
    _LIVE.append(g)
    return g.view


def check():
    """assert (after a synchronize) that the margins of every buffer made by guarded() since the last check() are intact; forgets them."""
    live, _LIVE[:] = list(_LIVE), []
    for g in live:
        g.check()


def at_end_of_poison(t, device=None, margin=MARGIN):
    """-> a contiguous copy of `t` on `device` whose last byte is directly followed by `margin` bytes of NaN (and preceded by NaN)."""
    if t is None:
        return None
    device = t.device if device is None else device
    t = t.contiguous()
    assert t.element_size() == 4, 'at_end_of_poison: 4-byte element types only'
    n = t.numel()
    front = ALIGN // 4
    base = torch.full((front + n + margin // 4,), float('nan'), dtype=torch.float32, device=device)
    body = base[front:front + n]
    out = body.view(t.dtype).view(t.shape) if t.dtype != torch.float32 else body.view(t.shape)
    out.copy_(t)
    return out
