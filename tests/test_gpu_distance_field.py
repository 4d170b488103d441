"""GPU: straps_distance_field (csrc/silfit.hip) against the integer transforms of tests/silfit_cases.py, exactly (torch.equal).

Sizes 1, 2, 3, 16, 17, 64, 65, 256, 257 (one lane per column in waves of 64, rows of 256 lanes per trip: both ragged and whole, and a second
trip of one lane), batches of 1 and 3, every mask case: empty, full, one pixel in each corner, random at density 0.4 (foreground bytes 2 and
255) and 0.01, and an empty frame between two non-empty ones; the reference is brute force.
Sizes 320 (two trips, the second ragged, a whole number of waves), 1000 (four trips, the last ragged, a padded column grid) and 1024 (the limit:
four whole trips, the full LDS row): the dense, the full and the empty mask alone and the batch (density 0.01, empty, one corner pixel), against
the row-blocked two-pass transform -- brute force on a dense 1024 x 1024 mask is out of reach, and tests/test_silfit_cases_cpu.py holds the two
transforms equal at every size up to 257 on all masks and at 1000 and 1024 on sparse ones.
The output sits behind redzone guards, the mask ends against a margin of foreground bytes."""
import numpy as np
import pytest
import torch

import silfit_cases as SC
from redzone import Zone
from smpl_cases import cpu_threads
from straps_amd import fit, hipabi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    torch.set_num_threads(cpu_threads())
    return torch.device('cuda:0')


def at_end_bytes(t, dev):
    """a uint8 tensor whose last byte is followed by a margin of 0xFF bytes (foreground, were it read)"""
    n = t.numel()
    base = torch.full((256 + n + 65536,), 255, dtype=torch.uint8, device=dev)
    out = base[256:256 + n].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize('wh', [1, 2, 3, 16, 17, 64, 65, 256, 257, 320, 1000, 1024])
def test_distance_field_is_exact(dev, wh):
    for names, masks, want in SC.distance_field_batches(wh):
        want = torch.from_numpy(want)
        z = Zone(dev)
        d2 = z.guarded(masks.shape, dtype=torch.int32, fill=-7, name='d2')
        m = at_end_bytes(torch.from_numpy(masks), dev)
        hipabi.check(hipabi.lib().straps_distance_field(hipabi.ptr(m), hipabi.ptr(d2), masks.shape[0], wh, hipabi.stream_ptr()), 'straps_distance_field')
        z.check()
        assert torch.equal(d2.cpu(), want), (wh, names)
        if 'empty' in names:
            assert bool((d2[names.index('empty')] == 2 * wh * wh).all())


def test_python_entry_takes_bool_and_float_masks_and_is_reproducible(dev):
    wh = 17
    m = torch.from_numpy(np.stack([SC.mask_cases(wh)[n] for n in ('rand04', 'empty', 'rand001')])).to(dev)
    want = torch.from_numpy(np.stack([SC.reference_d2(wh, n) for n in ('rand04', 'empty', 'rand001')]))
    a = fit.distance_field(m)
    assert a.dtype == torch.int32 and torch.equal(a.cpu(), want)
    assert torch.equal(fit.distance_field(m != 0), a) and torch.equal(fit.distance_field(m.float() * -0.5), a) and torch.equal(fit.distance_field(m), a)
    assert torch.equal(fit.distance_field(m[2:3]), a[2:3])      # a frame alone equals the frame inside a batch
    with pytest.raises(RuntimeError):
        fit.distance_field(m[:, :5])
    # a frame wider than one trip of 256 lanes
    names = ('rand001', 'empty', 'rand04')
    wide = torch.from_numpy(np.stack([SC.mask_cases(257)[n] for n in names])).to(dev)
    assert torch.equal(fit.distance_field(wide).cpu(), torch.from_numpy(np.stack([SC.reference_d2(257, n) for n in names])))
