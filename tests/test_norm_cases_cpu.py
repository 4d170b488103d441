"""CPU: tests/norm_cases.py -- the Python restatement of the launch rules of the BatchNorm, pooling and pooling-gradient kernels -- held to what the
built library reveals without a launch (straps_bn_bwd_blocks, straps_bn_bwd_workspace_bytes; no compute calls -- there is no GPU here), and the
coverage statement: the tables of tests/test_gpu_norm_pool_edges.py together reach every loop form, trip count and tail that can be reached.

The tiling and grid rules themselves (straps_grid256, straps_grid256_rows, straps_bn_tiled, straps_bn_tiled_grid, capped_grid, POOL_CHUNK) are not
exported: the library cannot confirm their restatement without a launch, and no entry point exists for that.  They are checked here against the
properties the kernels rely on (a stride that is a multiple of the row, a tiled grid that is a multiple of the column blocks)."""
import itertools

import pytest

import norm_cases as N
from straps_amd import hipabi


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _bwd_geometries():
    g = [(b.rows, b.c) for b in N.BWD] + [(B * H * H, c) for B, H, c in N.AUTOGRAD] + [(B * H * W, c) for B, H, W, c in N.POOL_SMALL + N.POOL_BWD_BIG + [N.POOL_SPARSE]]
    return g


def test_reduction_blocks_and_workspace_agree_for_every_case(lib):
    for rows, c in _bwd_geometries():
        assert N.bn_bwd_channels_ok(c), c
        assert lib.straps_bn_bwd_blocks(rows, c) == N.straps_bn_bwd_blocks(rows, c), (rows, c)
        assert lib.straps_bn_bwd_workspace_bytes(rows, c) == N.straps_bn_bwd_workspace_bytes(rows, c), (rows, c)
        nblk, rpb = N.straps_bn_bwd_blocks(rows, c), N.rows_per_block(rows, c)
        assert nblk * rpb >= rows and rpb < 2 ** 31                      # the blocks cover every row


def test_reduction_blocks_and_workspace_agree_on_a_grid(lib):
    rows = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8191, 65536, 65537, 131071, 131072, 131073, 131075, 140001, 260160, 262144, 1 << 22, (1 << 31) + 5]
    for r, c in itertools.product(rows, (4, 8, 32, 60, 64, 68, 128, 256, 512, 1024, 2048, 3072, 4096)):
        assert lib.straps_bn_bwd_blocks(r, c) == N.straps_bn_bwd_blocks(r, c), (r, c)
        assert lib.straps_bn_bwd_workspace_bytes(r, c) == N.straps_bn_bwd_workspace_bytes(r, c), (r, c)


def test_the_tables_reach_every_reachable_form():
    got = N.reached()
    missing = sorted(i for i in N.REQUIRED if i not in got)
    assert not missing, 'no case reaches %s' % missing
    assert not [i for i in N.UNREACHABLE if i in got], 'listed as unreachable, but a case reaches it'
    assert not [i for i in got if i not in N.EVERY], 'a form the coverage statement does not know'
    assert all(isinstance(v, str) and len(v) > 20 for v in N.UNREACHABLE.values())
    assert N.REQUIRED | set(N.UNREACHABLE) == N.EVERY and not (N.REQUIRED & set(N.UNREACHABLE))


def test_every_tensor_stays_under_twenty_million_floats():
    assert max(N.largest_tensor_floats()) < N.MAX_FLOATS == 20 * 1000 * 1000


def test_cases_named_for_a_form_reach_it():
    r = N.bn_apply_reach
    assert r('plain', 7, 96) == ('bn_apply', 'per_element', '1', True)
    assert r('plain', 43700, 96) == ('bn_apply', 'per_element', '>1', True)
    assert r('plain', 131072, 96) == ('bn_apply', 'per_element', '>1', False)
    assert r('x3', 5, 64) == ('bn_apply_x3', 'fixed', '1', True) and r('x3', 147, 128)[1] == 'fixed' and r('x3', 6, 768) == ('bn_apply_x3', 'fixed', '1', True)
    assert r('x3', 66537, 64) == ('bn_apply_x3', 'fixed', '>1', True)
    assert r('x3', 8, 256) == ('bn_apply_x3', 'tiled', '1', False)
    assert r('x3', 5472, 768) == ('bn_apply_x3', 'tiled', '>1', True) and N.straps_bn_tiled_grid(5472, 192, 4) == 4095
    assert r('x3', 2068, 2048) == ('bn_apply_x3', 'tiled', '>1', True) and N.straps_bn_tiled_grid(2068, 512, 4) == 4096
    b = N.bn_bwd_apply_reach
    assert b(8, 1024) == ('bn_bwd_apply', 'tiled', '1', False)
    assert b(1372, 3072) == ('bn_bwd_apply', 'tiled', '>1', True) and N.straps_bn_tiled_grid(1372, 768, 4) == 4092
    assert b(1373, 2048) == ('bn_bwd_apply', 'fixed', '1', False) and b(9, 64) == ('bn_bwd_apply', 'fixed', '1', True) and b(140001, 64) == ('bn_bwd_apply', 'fixed', '>1', True)
    d = N.bn_bwd_reduce_reach
    assert d(9, 64) == ('bn_bwd_reduce', False, True, False) and d(65, 4) == ('bn_bwd_reduce', False, True, False)
    assert d(130, 32) == ('bn_bwd_reduce', False, True, False) and N.rows_per_block(130, 32) == 44
    assert d(64, 8) == ('bn_bwd_reduce', True, False, False)
    assert d(131075, 4) == ('bn_bwd_reduce', True, True, True) and (N.straps_bn_bwd_blocks(131075, 4), N.rows_per_block(131075, 4)) == (2048, 65)
    assert d(260160, 4) == ('bn_bwd_reduce', True, False, True)
    assert d(140001, 64) == ('bn_bwd_reduce', True, True, True) and d(1373, 2048) == ('bn_bwd_reduce', True, True, False) and N.rows_per_block(140001, 64) == 69
    assert N.bn_partials_sum4_reach(960) == ('bn_partials_sum4', False, True) and N.bn_partials_sum4_reach(961) == ('bn_partials_sum4', True, True)
    assert N.bn_partials_sum4_reach(1024) == ('bn_partials_sum4', True, False)
    assert N.pool_reach('maxpool_idx', *N.POOL_FWD_BIG)[2:] == ('>1', True)
    assert N.pool_reach('maxpool_bwd', *N.POOL_BWD_BIG[0])[2:] == ('>1', True) and N.pool_reach('maxpool_bwd', *N.POOL_BWD_BIG[1])[2:] == ('>1', False)
    B, H, W, c = N.POOL_BWD_BIG[0]
    assert (B * H * W * c // 4) % N.POOL_CHUNK != 0
    assert N.bn_bwd_apply_pool_reach(1, 3, 5, 2048)[1] == 'per_element'
    assert N.gap_bwd_reach(5, 64, 3300)[2:] == ('>1', True)
    B, H, W, c = N.POOL_SPARSE
    assert W % 32 != 0 and H % 2 == 1


def test_every_option_of_the_entries_is_covered():
    a = N.APPLY
    assert {x.entry for x in a} == {'plain', 'x3', 'bits'} and {x.res for x in a} == {x.relu for x in a} == {False, True}
    assert any(not x.y and x.planes for x in a) and any(x.planes == 2 for x in a)
    assert all(x.y or x.planes for x in a) and all(x.c % 32 == 0 and x.relu for x in a if x.entry == 'bits') and all(x.planes == 0 for x in a if x.entry == 'plain')
    assert {N.bn_apply_reach('x3', x.rows, x.c)[1] for x in a if x.entry == 'bits'} == {'fixed', 'tiled'}
    b = N.BWD
    assert {x.entry for x in b} == {'plain', 'x3', 'bits', 'finish', 'finish_bits'}
    assert {x.mask for x in b} == {'none', 'yact', 'bits', 'rederived'} and {x.flags for x in b} == {0, 1, 2, 3} and {x.dz for x in b} == {False, True}
    assert any(not x.draw and x.planes for x in b) and all(x.draw or x.planes for x in b)
    assert all((x.mask == 'bits') == (x.entry in ('bits', 'finish_bits')) and (x.mask != 'bits' or (not x.dz and x.c % 32 == 0)) for x in b)
    assert all(x.planes == 0 for x in b if x.entry == 'plain') and all(x.planes == 0 or x.c % 32 == 0 for x in b)
    assert {x.nblk for x in b if x.entry.startswith('finish')} == set(N.FINISH_NBLK) and all(x.nblk == 0 for x in b if not x.entry.startswith('finish'))
    assert {N.bn_bwd_apply_reach(B * H * H, c)[1] for B, H, c in N.AUTOGRAD} == {'fixed', 'tiled'}


def test_unreachable_forms_stay_unreachable_over_a_sweep():
    """the reasons of UNREACHABLE, swept: a fixed stride behind straps_grid256_rows for every supported channel count; a tiled grid that is a multiple
    of the column blocks; no empty reduction block without the unrolled loop"""
    for c in range(4, 16388, 4):
        C4 = c >> 2
        for n4 in (C4, 255 * C4, 4099 * C4, (1 << 20) + C4 * 3, 5 * (1 << 20) * C4):
            g = N.straps_grid256_rows(n4, C4)
            assert 1 <= g <= N.CAP and (g * 256) % C4 == 0, (c, n4)
    for c, rows in itertools.product(range(64, 4097, 64), (4, 8, 16, 20, 4096, 5472, 16380, 16384, 65536, 100000)):
        wcg = N.straps_bn_tiled(rows, c >> 2)
        if wcg:
            ncb, g = (c >> 6) // wcg, N.straps_bn_tiled_grid(rows, c >> 2, wcg)
            assert c >= 256 and g % ncb == 0 and ncb <= g <= N.CAP and rows % (16 // wcg) == 0, (c, rows)
            assert N._tiled(rows, c >> 2, wcg)[1:] != ('1', True)
    for c in (4, 64, 128, 256, 1024, 2048, 4096):
        hi = 64 * (2048 // ((c + 63) // 64))
        for rows in itertools.chain(range(1, 700), range(hi - 70, hi + 200), (2 * hi, 2 * hi + 1, 3 * hi - 1)):
            r = N.bn_bwd_reduce_reach(rows, c)
            assert r[1] or r[2]
            assert not (r[3] and not r[1]), (rows, c)
