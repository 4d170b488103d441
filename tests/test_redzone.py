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


def _whole(t, dtype):
    whole = torch.empty(0, dtype=dtype).set_(t.untyped_storage())
    return whole, (t.data_ptr() - whole.data_ptr()) // whole.element_size()


def test_at_end_of_poison_two_byte_elements():
    t = (torch.arange(27, dtype=torch.int16) - 5).view(3, 9)
    p = redzone.at_end_of_poison(t)
    assert torch.equal(p, t) and p.dtype == torch.int16 and p.is_contiguous() and p.data_ptr() % 16 == 0
    whole, first = _whole(p, torch.int16)
    assert bool((whole[first + 27:] == redzone.BF16_NAN).all()) and whole.numel() - first - 27 == redzone.MARGIN // 2
    assert bool((whole[:first] == redzone.BF16_NAN).all())
    # the margin word IS a NaN when a bf16 consumer reads it
    assert bool(torch.isnan(whole[first + 27:first + 29].view(torch.bfloat16).float()).all())
    b = redzone.at_end_of_poison(torch.ones(5, dtype=torch.bfloat16))
    assert b.dtype == torch.bfloat16 and b.tolist() == [1.0] * 5
    with pytest.raises(AssertionError, match='2- and 4-byte'):
        redzone.at_end_of_poison(torch.zeros(3, dtype=torch.float64))


@pytest.mark.parametrize('n', [8, 13, 96, 1001])
def test_planes_with_gaps(n):
    ps = (n + 7) // 8 * 8
    src = (torch.arange(3 * ps, dtype=torch.int32) % 251 + 1).to(torch.int16).view(3, ps)
    out, ps2 = redzone.planes_with_gaps(src, n, gap=64)
    assert ps2 > n and ps2 % 8 == 0 and ps2 == ps + 64 and out.data_ptr() % 16 == 0 and tuple(out.shape) == (3, ps2)
    assert out.stride() == (ps2, 1)
    assert torch.equal(out[:, :n], src[:, :n])
    assert bool((out[:, n:] == redzone.BF16_NAN).all())              # the gap starts at element n, not at the rounded stride
    whole, first = _whole(out, torch.int16)
    assert bool((whole[:first] == redzone.BF16_NAN).all()) and whole.numel() == first + 3 * ps2
    # a read one element past a plane is a NaN once used
    assert bool(torch.isnan(out[:, n].view(torch.bfloat16).float()).all())
    z = Zone('cpu')
    o2, ps3 = z.planes(src, n)
    assert ps3 == ps + redzone.PLANE_GAP and torch.equal(o2[:, :n], src[:, :n])


def test_guarded_output_planes_intact_passes_and_body_is_nan():
    z = Zone('cpu')
    v, ps = z.guarded_planes(21, gap=16, name='yp')
    assert tuple(v.shape) == (3, ps) and ps == 24 + 16 and v.dtype == torch.int16 and v.data_ptr() % 16 == 0
    assert bool((v == redzone.BF16_NAN).all())
    v[:, :21] = 7                                                     # what the kernel does: the three extents, nothing else
    z.check()


@pytest.mark.parametrize('plane,off', [(0, 21), (1, 23), (2, 39), (0, 24)])
def test_a_write_into_a_plane_gap_is_reported_with_plane_and_offset(plane, off):
    g = redzone.PlaneGuard(21, 'cpu', gap=16, name='yp')
    g.view[:, :21] = 3
    g.view[2, 30] = 9                                                 # a later one: the FIRST is named
    g.view[plane, off] = 5                                            # a plain indexed write, as a stray store would be
    first = min((plane, off), (2, 30))
    assert g.gap_damage() == (first[0], first[1], 5 if first == (plane, off) else 9)
    with pytest.raises(AssertionError, match=r"plane gap 'yp'.*behind plane %d was overwritten at element %d " % first):
        g.check()


def test_a_write_behind_the_last_plane_is_a_margin_hit():
    g = redzone.PlaneGuard(8, 'cpu', gap=8)
    g.base[g.hi] = 1
    with pytest.raises(AssertionError, match='0 bytes past its end'):
        g.check()


def test_at_end_of_poison_wide_takes_bytes_and_doubles():
    t = torch.arange(11, dtype=torch.uint8).view(1, 11)
    p = redzone.at_end_of_poison_wide(t)
    assert torch.equal(p, t) and p.dtype == torch.uint8
    whole, first = _whole(p, torch.uint8)
    assert bool((whole[first + 11:] == redzone.BYTE_POISON).all()) and whole.numel() - first - 11 == redzone.MARGIN and bool((whole[:first] == redzone.BYTE_POISON).all())
    d = redzone.at_end_of_poison_wide(torch.arange(5, dtype=torch.float64))
    assert d.dtype == torch.float64 and d.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and d.data_ptr() % 16 == 0
    whole, first = _whole(d, torch.float64)
    assert bool(torch.isnan(whole[first + 5:]).all()) and whole.numel() - first - 5 == redzone.MARGIN // 8 and bool(torch.isnan(whole[:first]).all())
    f = redzone.at_end_of_poison_wide(torch.ones(3))
    assert f.dtype == torch.float32 and f.tolist() == [1.0] * 3 and redzone.at_end_of_poison_wide(None) is None
    z = redzone.Zone('cpu')
    a = z.at_end(t)
    assert z.operands[-1] is a                      # the zone keeps its operands alive
