"""CPU: the redzone helper itself -- a plain torch indexed write into either margin is reported with its offset, a clean buffer passes,
an unwritten body is NaN, and at_end_of_poison() puts NaN directly behind an operand."""
import pytest
import torch

import redzone
from redzone import Guard, Zone


def test_clean_buffer_passes_and_body_is_nan_and_aligned():
    for shape, dtype in (((3, 10), torch.float32), ((7,), torch.float32), ((5, 3), torch.int32), ((2, 3), torch.float64)):
        g = Guard(shape, dtype, 'cpu', fill=float('nan') if dtype.is_floating_point else 0, name='clean')
        assert tuple(g.view.shape) == shape and g.view.dtype == dtype
        assert g.view.data_ptr() % 256 == 0
        if dtype.is_floating_point:
            assert bool(torch.isnan(g.view).all())
        g.view.fill_(1)                                        # writing the whole body is what a kernel does
        g.check()
        assert g.lo * 4 >= redzone.MARGIN and (g.base.numel() - g.hi) * 4 >= redzone.MARGIN


@pytest.mark.parametrize('where', ['just_before', 'far_before', 'just_behind', 'far_behind'])
def test_a_write_into_a_margin_is_reported_with_its_offset(where):
    g = Guard((4, 10), torch.float32, 'cpu', name='victim')
    n = g.view.numel()
    word = {'just_before': g.lo - 1, 'far_before': 0, 'just_behind': g.hi, 'far_behind': g.base.numel() - 1}[where]
    g.base[word] = 12345                                       # a plain indexed write, as a stray store would be
    off = (word - g.lo) * 4
    assert g.damage() == (off, 12345)
    with pytest.raises(AssertionError, match=r"redzone 'victim'.*byte offset %d " % off):
        g.check()
    if where == 'just_behind':
        assert off == n * 4


def test_first_damaged_offset_is_named():
    g = Guard((8,), torch.float32, 'cpu')
    g.base[g.hi + 5] = 1
    g.base[g.hi + 2] = 1
    assert g.damage()[0] == 32 + 8


def test_module_level_registry_and_zone():
    a = redzone.guarded((3,), torch.float32, 'cpu')
    b = redzone.guarded((3,), torch.float32, 'cpu', fill=0.0)
    assert bool(torch.isnan(a).all()) and not b.any()
    redzone.check()
    z = Zone('cpu')
    v = z.guarded((5,), name='v')
    z.check()
    z.guards[0].base[z.guards[0].hi] = 0
    with pytest.raises(AssertionError, match='0 bytes past its end'):
        z.check()
    assert v.numel() == 5


def test_at_end_of_poison():
    t = torch.arange(30, dtype=torch.float32).view(3, 10)
    p = redzone.at_end_of_poison(t)
    assert torch.equal(p, t) and p.is_contiguous() and p.data_ptr() % 4 == 0
    base = p.untyped_storage()
    whole = torch.empty(0, dtype=torch.float32).set_(base)
    first = (p.data_ptr() - whole.data_ptr()) // 4
    assert bool(torch.isnan(whole[first + 30:]).all()) and whole.numel() - first - 30 == redzone.MARGIN // 4
    assert bool(torch.isnan(whole[:first]).all())
    i = redzone.at_end_of_poison(torch.arange(6, dtype=torch.int32))
    assert i.dtype == torch.int32 and i.tolist() == list(range(6))
    assert redzone.at_end_of_poison(None) is None
