"""Test helper: guarded buffers, so that a kernel's WRITE outside an output -- or READ past an operand -- shows in a test.

conftest.py poisons free memory, which turns a read of memory nobody wrote into a NaN.  A write past an output, past the advertised
workspace or into a neighbour's padding lands in some other tensor, and no assertion looks there.  Here every output / workspace of a
test is a view into the middle of a larger allocation the test owns:

    [ margin: sentinel words | body (the tensor the kernel gets) | slack | margin: sentinel words ]

`guarded()` returns the body; `Guard.check()` (or `check()` for all live guards of a `Zone`) synchronizes and asserts that both margins
still hold the sentinel, bit for bit, naming the first damaged byte offset relative to the body.  The body of an output is pre-filled
with NaN, so an element the kernel should have written and did not is a NaN in the comparison that follows.

`at_end_of_poison()` places an input so that its last byte is followed by a NaN margin (what test_dgrad_x3_with_fused_batchnorm_sums
does by hand): a read past the operand's end becomes a NaN in the result.  2-byte element types (bf16 bit patterns as int16) get the bf16
quiet-NaN pattern 0x7FC0 as margin; `at_end_of_poison_wide()` (what `Zone.at_end` calls) also takes 1- and 8-byte element types.

`planes_with_gaps()` re-homes a [3][ps] int16 plane operand (straps_split3_bf16[_cm], the weight packs) as [3][ps'] with ps' > n: split3 always
gives ps == n rounded up to 8, so a read past plane 0 lands in plane 1 -- finite, plausible data.  Here every plane is followed by a gap of
0x7FC0 words: an over-read whose value is USED is a NaN in the result.  `PlaneGuard` is the output counterpart (straps_conv_fwd_x3p's y_planes
with y_plane_stride larger than the extent): margins as a Guard, and the gap words behind every plane must be unchanged after the call.

The margins are ordinary memory of the test; nothing here provokes a fault.  No GPU kernels of its own: torch fills and compares.
"""
import torch

MARGIN = 64 << 10                 # bytes on either side (the widest row stride of the guarded outputs, 6890 * 3 * 4 B, fits 0.79 times)
ALIGN = 256                       # the body starts on a 256-byte boundary, as a tensor of the caching allocator would
SENTINEL = 0x7FC0BEEF             # a quiet-NaN bit pattern with a payload, as int32: a stray READ of a margin is a NaN as well
BF16_NAN = 0x7FC0                 # bf16 quiet NaN (as int16: 32704): the margin / gap word of 2-byte plane tensors
BYTE_POISON = 4                   # margin byte of 1-byte operands (arg-max taps, tile maps): a VALID tap on purpose, see at_end_of_poison_wide
PLANE_GAP = MARGIN // 2           # default gap behind a plane, in 2-byte elements (a 256-row tile of one 32-channel chunk is 8 192 elements)


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
        self.device, self.guards, self.operands = device, [], []

    def guarded(self, shape, dtype=torch.float32, fill=float('nan'), margin=MARGIN, name=''):
        g = Guard(shape, dtype, self.device, fill, margin, name or 'buffer %d' % len(self.guards))
        self.guards.append(g)
        return g.view

    def at_end(self, t):
        # (the zone keeps the operand alive: a call that passes hipabi.ptr(z.at_end(t)) would otherwise hand over memory the allocator has taken back)
        out = at_end_of_poison_wide(t, self.device)
        self.operands.append(out)
        return out

    def planes(self, planes, n, gap=PLANE_GAP):
        return planes_with_gaps(planes, n, self.device, gap)

    def guarded_planes(self, n, gap=PLANE_GAP, name=''):
        """-> (int16 [3][ps'] output planes with guarded gaps, ps'); checked by check()"""
        g = PlaneGuard(n, self.device, gap, name or 'planes %d' % len(self.guards))
        self.guards.append(g)
        return g.view, g.ps

    def check(self):
        for g in self.guards:
            g.check()


class PlaneGuard(Guard):
    """a guarded OUTPUT plane tensor: `.view` is int16 [3][ps], ps = n rounded up to 8 + gap; elements [n, ps) of every plane (the gap) and the
    margins around the whole tensor must be unchanged after the call; the extents [0, n) are pre-filled with 0x7FC0 as well (an element the kernel
    should have written and did not reads as NaN)."""

    def __init__(self, n, device='cpu', gap=PLANE_GAP, name=''):
        assert gap > 0 and gap % 8 == 0
        self.n, self.ps = int(n), (int(n) + 7) // 8 * 8 + gap
        Guard.__init__(self, (3, self.ps), torch.int16, device, fill=BF16_NAN, name=name)
        assert self.view.data_ptr() % 16 == 0

    def gap_damage(self):
        """-> None, or (plane, element offset inside the plane, word found) of the first changed gap word."""
        if self.base.is_cuda:
            torch.cuda.synchronize(self.base.device)
        bad = (self.view[:, self.n:] != BF16_NAN).nonzero()
        if bad.numel():
            pl, off = int(bad[0, 0]), int(bad[0, 1]) + self.n
            return pl, off, int(self.view[pl, off]) & 0xFFFF
        return None

    def check(self):
        Guard.check(self)
        d = self.gap_damage()
        assert d is None, ('plane gap %r (3 planes of %d elements at stride %d): the gap behind plane %d was overwritten at element %d of the plane '
                           '(%d elements past its extent), found 0x%04x' % (self.name, self.n, self.ps, d[0], d[1], d[1] - self.n, d[2]))


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
    assert t.element_size() in (2, 4), 'at_end_of_poison: 2- and 4-byte element types only'
    n = t.numel()
    if t.element_size() == 2:
        front = ALIGN // 2
        base = torch.full((front + n + margin // 2,), BF16_NAN, dtype=torch.int16, device=device)
        out = base[front:front + n].view(t.dtype).view(t.shape)
        out.copy_(t)
        return out
    front = ALIGN // 4
    base = torch.full((front + n + margin // 4,), float('nan'), dtype=torch.float32, device=device)
    body = base[front:front + n]
    out = body.view(t.dtype).view(t.shape) if t.dtype != torch.float32 else body.view(t.shape)
    out.copy_(t)
    return out


def at_end_of_poison_wide(t, device=None, margin=MARGIN):
    """at_end_of_poison for the operands of the BatchNorm / pooling kernels as well: 1-byte element types (arg-max taps, tile maps) get a margin of
    BYTE_POISON -- bytes have no NaN.  The trade-off: a byte outside 0..8 (0xEE, say) could never be a right tap and would be easier to attribute, but
    bn_bwd_reduce_pooled_kernel gathers raw at the position its tap names -- tap 0xEE is 79 rows below the window, far outside the tensor, and a test
    helper must not turn an over-read of one byte into a wild read.  The centre tap stays inside the window; it shows because the gradient operand read
    at the same offset is NaN there, and as a tile-map byte it marks an inactive tile active, whose NaN prefill is then overwritten -- and 8-byte ones (double partial sums) a
    margin of fp64 NaNs (two fp32 NaN words side by side are a FINITE double)"""
    if t is None or t.element_size() in (2, 4):
        return at_end_of_poison(t, device, margin)
    device = t.device if device is None else device
    t = t.contiguous()
    assert t.element_size() in (1, 8), 'at_end_of_poison_wide: 1-, 2-, 4- and 8-byte element types only'
    n = t.numel()
    if t.element_size() == 8:
        front = ALIGN // 8
        base = torch.full((front + n + margin // 8,), float('nan'), dtype=torch.float64, device=device)
        out = base[front:front + n].view(t.dtype).view(t.shape)
    else:
        base = torch.full((ALIGN + n + margin,), BYTE_POISON, dtype=torch.uint8, device=device)
        out = base[ALIGN:ALIGN + n].view(t.dtype).view(t.shape)
    out.copy_(t)
    return out


def planes_with_gaps(planes, n, device=None, gap=PLANE_GAP):
    """[3][ps] int16 planes whose first n elements each are the operand -> (copy [3][ps'], ps') with ps' = n rounded up to 8 + gap > n,
    ps' % 8 == 0, a 16-byte-aligned base, and 0x7FC0 in every element outside the three extents: directly behind element n - 1 of every plane
    (the gap; behind the last plane it is the margin) and in front of plane 0."""
    assert planes.dim() == 2 and planes.shape[0] == 3 and planes.element_size() == 2 and planes.shape[1] >= n
    assert gap > 0 and gap % 8 == 0
    device = planes.device if device is None else device
    ps = (n + 7) // 8 * 8 + gap
    front = ALIGN // 2
    base = torch.full((front + 3 * ps,), BF16_NAN, dtype=torch.int16, device=device)
    out = base[front:].view(3, ps)
    out[:, :n].copy_(planes[:, :n])
    assert out.data_ptr() % 16 == 0
    return out, ps
