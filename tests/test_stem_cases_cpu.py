"""CPU: tests/stem_cases.py held together -- the reach table of the stem edge cases is complete, the restated sizes equal the library's size functions,
the mask / activity references agree with a per-pixel scan of x, the tracer cases are exact in fp32, the float64 references agree with a second
evaluation, and the argument checks of the stem entry points return before a launch.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import stem_cases as S
from straps_amd import hipabi

EINVAL = 1


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _err(lib):
    return lib.straps_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------------------ reach

def test_every_required_combination_is_reached():
    got = S.reached()
    missing = [k for k in S.REQUIRED if not got.get(k)]
    assert not missing, 'no case reaches %s' % missing                      # (the cap on left-out combinations is zero)
    assert not set(S.REQUIRED) & set(S.UNREACHABLE)
    assert len(set(S.REQUIRED)) == len(S.REQUIRED)
    for k in S.REQUIRED:
        print('REACH %-22s %-34s %4d  %s' % (k[0], k[1], len(got[k]), got[k][0]))
    # what the issue names explicitly
    for want in ('n_active 0', 'n_active 1', 'n_active 4', 'n_active 5', 'n_active 7', 'n_active 8', 'n_active C', 'list length 0', 'list length 1',
                 'list length 2', 'straddle across ranks 3|4', 'straddle across ranks 6|7', 'vector fill', 'scalar fill'):
        assert ('stem_kernel', want) in S.REQUIRED
    for nt in range(1, 5):
        assert ('stem_dgrad_kernel', '<%d>' % nt) in S.REQUIRED and ('stem_dgrad_kernel', '<%d> after full' % nt) in S.REQUIRED
    # the proxy_like family: tiles with 0, 1, 3, 4, 5, 7, 8 and all channels active
    seen = set()
    for case in S.cases('fwd'):
        if case.family == 'proxy_like' and case.shape[1] == 18:
            seen |= {t.n_active for t in S.fwd_reach(S.case_mask(case), case.shape)}
    assert {0, 1, 3, 4, 5, 7, 8, 18} <= seen, sorted(seen)


def test_unreachable_stays_unreachable():
    """sweeps: a K group / a unit never touches three channels; an active tile has an active channel; every needed group of every tile of every case is
    contracted in EXACTLY one pass (the rule the channel passes of stem_kernel rest on)"""
    for Cn in range(1, 70):
        K, Kp = 49 * Cn, S.fwd_kp(Cn)
        k = np.arange(Kp).reshape(-1, 8)
        assert int((np.minimum(k[:, 7], K - 1) // 49 - k[:, 0] // 49).max()) <= 1
    for nc in range(1, 5):
        assert all(sp is None or sp[1] - sp[0] <= 1 for sp in S.wgrad_units(nc))
    rng = np.random.RandomState(5)
    flags = [np.ones((Cn, 13), bool) for Cn in (1, 4, 5, 7, 8, 18, 64)]
    flags += [rng.rand(Cn, 13) < p for Cn in (2, 5, 6, 7, 8, 9, 18) for p in (0.05, 0.3, 0.8) for _ in range(6)]
    for case in S.cases('fwd'):
        B, Cn, H, W = case.shape
        cells = S.mask_cells(S.case_mask(case), B, Cn, H, W)
        tx_, ty_, _ = S.tiles(B, H, W, S.FWD_TY)
        flags += [S.fwd_rowflags(cells, b, ty, tx, Cn, H, W) for b in range(B) for ty in range(ty_) for tx in range(tx_)]
    for rf in flags:
        t, (counts, needed) = S.fwd_tile_reach(rf)
        assert (t.n_active == 0) == (not rf.any()) and (t.passes == 0) == (t.n_active == 0)
        assert bool((counts == needed).all()), 'a needed K group is contracted %s times' % sorted(set(counts[counts != needed].tolist()))
    assert S.proxy_reach(257) == (False, True) and S.proxy_reach(256) == (True, False) and S.proxy_reach(255) == (False, False)


# ------------------------------------------------------------------------------------------------------------------------------------ mask references

def _brute_words(x):
    x = x.numpy()
    B, Cn, H, W = x.shape
    HC, WW = S.mask_dims(H, W)
    words = np.zeros((B, Cn, HC, WW), np.uint32)
    b, c, h, w = np.nonzero(x != 0)
    np.bitwise_or.at(words, (b, c, h >> 2, w >> 8), (np.uint32(1) << ((w >> 3) & 31).astype(np.uint32)))
    return words


def _brute_tile_channels(x, ty, ph):
    """per tile and channel: a non-zero PIXEL inside the cells that the tile's patch touches"""
    nz = x.numpy() != 0
    B, Cn, H, W = nz.shape
    tx_, ty_, _ = S.tiles(B, H, W, ty)
    out = np.zeros((B, ty_, tx_, Cn), bool)
    for tyi in range(ty_):
        r0, r1 = S.patch_rows(tyi, ty, ph, H)
        for txi in range(tx_):
            wa, wb = S.patch_cols(txi, W)
            out[:, tyi, txi] = nz[:, :, (r0 >> 2) * 4:(r1 >> 2) * 4 + 4, (wa >> 3) * 8:(wb >> 3) * 8 + 8].any(axis=(2, 3))
    return out.reshape(-1, Cn)


def test_mask_references_against_a_pixel_scan():
    seen = set()
    for case in S.cases('wgrad'):
        x = S.case_x(case)
        B, Cn, H, W = case.shape
        m = S.nzmask_ref(x)
        assert m.shape == (B, Cn) + S.mask_dims(H, W) and m.size == S.nzmask_words(B, Cn, H, W)
        assert np.array_equal(m, _brute_words(x)), case.id
        act = _brute_tile_channels(x, S.WG_TY, S.WG_PH)
        assert np.array_equal(S.tile_any_ref(m, B, Cn, H, W), act.any(1).astype(np.uint8)), case.id
        tact = S.tile_act_ref(m, B, Cn, H, W)
        for c in range(Cn):
            assert np.array_equal((tact[c // 4] >> (c % 4)) & 1, act[:, c].astype(np.uint8)), case.id
        assert int(tact.max()) < (1 << min(4, Cn))
        seen.add(case.family)
        if case.arg == 'negzero':
            cells = S.mask_cells(m, B, Cn, H, W)
            assert not cells[:, :, 1].any() and not cells[:, :, :, 1::2].any() and cells[:, :, 0, 0].all()
        if case.arg == 'nan':
            b, c, h, w = S.nan_pixel(case.shape)
            assert (m[b, c, h >> 2, w >> 8] >> ((w >> 3) & 31)) & 1
    assert seen == {'dense', 'tracer', 'single_pixel', 'proxy_like', 'specials'}
    # a single pixel lights exactly one bit
    for shape in S.SINGLE_SHAPES:
        for pos in S.single_pixel_positions(shape):
            m = S.nzmask_ref(S.single_pixel_x(shape, pos))
            assert sum(bin(int(v)).count('1') for v in m.reshape(-1)) == 1


def test_single_pixel_positions_come_from_the_geometry():
    pos = {(h, w) for (c, h, w) in S.single_pixel_positions((1, 6, 8, 516))}
    cols = {w for (h, w) in pos}
    assert {0, 515, 60, 61, 65, 66, 67, 7, 8, 255, 256} <= cols
    assert {(0, 0), (0, 515), (7, 0), (7, 515)} <= pos and {3, 4} <= {h for (h, w) in pos}
    rows = {h for (c, h, w) in S.single_pixel_positions((1, 18, 33, 50))}
    assert {0, 32, 3, 4, 5, 17, 1, 9} <= rows              # forward tile row 1 reads rows 5 .. 17, the weight gradient's rows 1 .. 9
    assert S.patch_cols(1, 516) == (60, 131) and S.patch_cols(0, 516) == (0, 67) and S.patch_rows(1, S.FWD_TY, S.FWD_PH, 33) == (5, 17)


# ------------------------------------------------------------------------------------------------------------------------------------ sizes

def test_restated_sizes_equal_the_library(lib):
    shapes = {c.shape for c in S.cases('wgrad')}
    shapes |= {(B, Cn, H, W) for B in (1, 2) for Cn in (1, 19, 20, 21) for H in range(1, 19) for W in (7, 63, 64, 65, 255, 256, 257, 511, 512, 513)}
    shapes |= {(B, Cn, 3, 9) for B in (254, 255, 256, 257, 258) for Cn in (1, 4, 5)}             # one tile per image: ntiles = 255 .. 257
    shapes |= {(B, 3, 7, 70) for B in (63, 64, 65)}                                              # four tiles per image: ntiles = 252, 256, 260
    for (B, Cn, H, W) in sorted(shapes):
        what = (B, Cn, H, W)
        assert lib.straps_stem_stat_blocks(B, H, W) == S.stat_blocks(B, H, W), what
        assert lib.straps_stem_nzmask_words(B, Cn, H, W) == S.nzmask_words(B, Cn, H, W), what
        assert lib.straps_stem_tiles(B, H, W) == S.stem_tiles(B, H, W), what
        assert lib.straps_stem_wgrad_workspace_bytes(B, Cn, H, W) == S.wgrad_workspace_bytes(B, Cn, H, W), what
    for cin in range(0, 70):
        assert lib.straps_stem_dgrad_weight_floats(cin) == S.dgrad_weight_floats(cin), cin
        if cin:
            assert lib.straps_stem_weight_floats(cin) == S.stem_weight_floats(cin), cin
            assert S.pack_stem_weight_ref(np.zeros((64, cin, 7, 7), np.float32)).size == S.stem_weight_floats(cin)
    assert [S.dgrad_chunks(c) for c in (18, 19, 20, 21, 25, 64)] == [(0, 18, 5), (0, 19, 5), (1, 0, 0), (1, 1, 1), (1, 5, 2), (3, 4, 1)]
    assert lib.straps_stem_nzmask_words(0, 3, 8, 8) == 0 and S.nzmask_words(0, 3, 8, 8) == 0
    assert [S.wgrad_reach(S.nzmask_ref(np.ones(s, np.float32)), s).rows for s in ((255, 1, 3, 9), (256, 1, 3, 9), (257, 1, 3, 9))] == [1, 1, 2]
    assert S.fwd_lds_bytes(18) <= S.LDS_LIMIT < S.fwd_lds_bytes(300)


def test_packed_weight_restatements():
    """the two packed layouts, entry by entry from their definition (a slow loop on a small weight)"""
    w = S.det((64, 3, 7, 7), 77).numpy()
    f = S.pack_stem_weight_ref(w).reshape(-1, 2, 64, 4)
    for g, nt, lane, e in itertools.product((0, 5, 18), (0, 1), (0, 31, 32, 63), range(4)):
        k = 8 * g + 4 * (lane >> 5) + e
        assert f[g, nt, lane, e] == (w.reshape(64, -1)[nt * 32 + (lane & 31), k] if k < 147 else 0)
    w = S.det((64, 23, 7, 7), 78).numpy()
    p = S.pack_stem_dgrad_weight_ref(w).reshape(64, 2, 5, 64, 4)
    real = 0
    for kg, ch, nt, lane, s in itertools.product((0, 1, 22, 43, 63), (0, 1), range(5), (0, 3, 17, 46, 63), (0, 3)):
        d, e = kg >> 4, (kg >> 2) & 3
        o = 16 * (kg & 3) + 4 * (lane >> 4) + s
        n = nt * 16 + (lane & 15)
        c, r, q = ch * 20 + (n >> 2), ((n >> 1) & 1) + 5 - 2 * d, (n & 1) + 5 - 2 * e
        ok = c < 23 and 0 <= r < 7 and 0 <= q < 7
        real += ok
        assert p[kg, ch, nt, lane, s] == (w[o, c, r, q] if ok else 0)
    assert real > 50
    # 49 of the 64 (d, e, py, px) combinations are real taps
    p1 = S.pack_stem_dgrad_weight_ref(np.ones((64, 1, 7, 7), np.float32)).reshape(64, 1, 5, 64, 4)
    assert int(p1[0::4, 0, 0, 0:4, 0].sum()) == 49


# ------------------------------------------------------------------------------------------------------------------------------------ exactness of the tracer cases

EXACT = float(2 ** 24)


def stats_exact(case):
    """the float64 sum of y^2 over a (tile, channel) stays below 2^24: the fp32 statistics partials of the case are exact integers"""
    y, _ = S.fwd_reference(S.case_x(case), S.case_w(case))
    B, Cn, H, W = case.shape
    _, q, a, _ = S.stats_reference(y.permute(0, 2, 3, 1).float(), B, H, W)
    return float(q.max()) < EXACT and float(a.max()) < EXACT


def test_tracer_cases_stay_below_2_to_24():
    marked = {}
    for case in S.cases('wgrad'):
        if not S.case_integer(case):
            continue
        x, w, dy = S.case_x(case), S.case_w(case), S.case_dy(case)
        assert bool((x == x.round()).all()) and float(x.abs().max()) <= 2 and float(w.abs().max()) <= 2 and float(dy.abs().max()) <= 2
        assert len({float(v) for v in w[:2, :1, :2, :2].flatten()}) > 2
        B, Cn, H, W = case.shape
        if case.shape in S.FWD_SHAPES or case.shape[0] == 1:
            assert float(S.fwd_reference(x, w)[1].max()) < EXACT, case.id
            marked[case.id] = stats_exact(case)
            assert marked[case.id] or case.family == 'tracer', '%s: the statistics of this case are not exact in fp32' % case.id
        assert 4.0 * B * S.out_hw(H, W)[0] * S.out_hw(H, W)[1] < EXACT, case.id                 # sum|x dy| <= 2 * 2 * (B Ho Wo)
    for (cin, B, H, W) in S.dgrad_cases():
        assert 4.0 * 1024 < EXACT
    case = [c for c in S.cases('wgrad') if c.id == 'tracer-7x5x64x136'][0]
    assert float(S.wgrad_reference(S.case_x(case), S.case_dy(case))[1].max()) < EXACT
    # (the tracer weights change sign along every index, so y stays small even at 64 channels: EVERY integer case has exact statistics, and the GPU
    # tests compare the partials of all of them with ==)
    assert marked and all(marked.values()), sorted(k for k, v in marked.items() if not v)


# ------------------------------------------------------------------------------------------------------------------------------------ references

def test_references_against_a_second_evaluation():
    for shape in ((1, 1, 7, 7), (2, 2, 9, 13)):
        x, w = S.det(shape, 81, 0.0, 1.0), S.dense_w(shape[1], 82)
        y, ya = S.fwd_reference(x, w)
        want = S.fwd_loop(x, w)
        assert float((y - want).abs().max()) <= 1e-13 * float(ya.max())
        assert float((ya - S.fwd_loop(x.abs(), w.abs())).abs().max()) <= 1e-13 * float(ya.max()) and bool((ya >= y.abs() - 1e-15).all())
        B, Cn, H, W = shape
        Ho, Wo = S.out_hw(H, W)
        assert tuple(y.shape) == (B, 64, Ho, Wo)
        dy = S.det((B, 64, Ho, Wo), 83)
        dw, dwa = S.wgrad_reference(x, dy)
        assert float((dw - S.wgrad_unfold(x, dy)).abs().max()) <= 1e-13 * float(dwa.max())
        dx, dxa = S.dgrad_reference(dy, w, H, W)
        assert float((dx - S.dgrad_fold(dy, w, H, W)).abs().max()) <= 1e-13 * float(dxa.max())
        # and by the adjoint identity <y, dy> = <w, dw> = <x, dx>
        ip = float((y * dy.double()).sum())
        assert abs(ip - float((w.double() * dw).sum())) <= 1e-12 * float((ya * dy.abs()).sum())
        assert abs(ip - float((x.double() * dx).sum())) <= 1e-12 * float((ya * dy.abs()).sum())
    # the tracer references are integers
    x, w = S.tracer_x((2, 2, 9, 13)), S.tracer_w(2)
    y = S.fwd_reference(x, w)[0]
    assert bool((y == y.round()).all()) and bool((y == S.fwd_loop(x, w)).all())
    # window_contains against the forward of a single one
    for pix in ((0, 0, 0), (1, 8, 12), (1, 4, 7)):
        x = torch.zeros(2, 1, 9, 13)
        x[pix[0], 0, pix[1], pix[2]] = 1
        hit = S.fwd_reference(x, torch.ones(64, 1, 7, 7))[0][:, 0] != 0
        assert np.array_equal(hit.numpy(), S.window_contains(2, 9, 13, pix))
    # stats_reference counts the in-range pixels of ragged tiles
    y = torch.ones(3, 5, 33, 64)
    s1, s2, sa, n = S.stats_reference(y, 3, 9, 66)
    assert n.tolist() == [128.0, 4.0, 32.0, 1.0] * 3 and bool((s1 == n[:, None]).all()) and bool((s2 == s1).all()) and bool((sa == s1).all())


# ------------------------------------------------------------------------------------------------------------------------------------ argument checks

def _buf(n=64):
    a = np.full(n, 0x5A, np.uint8)
    return a, C.c_void_p(a.ctypes.data)


def _intact(*arrays):
    return all(bool((a == 0x5A).all()) for a in arrays)


def test_stem_argument_checks_return_before_a_launch(lib):
    """every check returns the error code with the entry point's name in straps_last_error and never touches its outputs (host memory here: the
    pointers are not dereferenced, nothing is launched)"""
    xa, x = _buf()
    ya, y = _buf()
    za, z = _buf()
    for (h, w) in ((6, 8), (8, 6)):
        assert lib.straps_stem_fwd(x, x, None, None, 0, y, z, None, 1, 3, h, w, None) == EINVAL and 'straps_stem_fwd' in _err(lib)
    assert lib.straps_stem_fwd(x, x, x, None, 1, y, None, None, 1, 3, 8, 8, None) == EINVAL and 'scale and shift' in _err(lib)
    assert lib.straps_stem_fwd(x, x, None, x, 1, y, None, None, 1, 3, 8, 8, None) == EINVAL and 'scale and shift' in _err(lib)
    assert lib.straps_stem_fwd(x, x, None, None, 0, y, z, None, 1, 300, 8, 8, None) == EINVAL and 'LDS' in _err(lib)
    assert lib.straps_stem_nzmask(x, y, 0, 3, 8, 8, None) == EINVAL and 'straps_stem_nzmask' in _err(lib)
    assert lib.straps_stem_wgrad(x, x, y, None, None, 1, 3, 8, 8, 0, None) == EINVAL and 'straps_stem_wgrad' in _err(lib)
    assert lib.straps_stem_tile_activity(x, y, 1, 3, 6, 8, None) == EINVAL and 'straps_stem_tile_activity' in _err(lib)
    assert lib.straps_stem_dgrad(x, x, y, 1, 65, 8, 8, 0, None) == EINVAL and 'straps_stem_dgrad' in _err(lib)
    assert lib.straps_stem_dgrad(x, x, y, 1, 3, 8, 8, 2, None) == EINVAL and 'accumulate' in _err(lib)
    for (wh, std) in ((16, 2), (24, 0), (24, 7)):
        assert lib.straps_build_proxy_input_std(x, x, y, 1, 3, wh, std, None) == EINVAL and 'straps_build_proxy_input' in _err(lib)
        assert lib.straps_build_proxy_input_nz(x, x, y, z, 1, 3, wh, std, None) == EINVAL and 'straps_build_proxy_input_nz' in _err(lib)
    assert lib.straps_build_proxy_input_nz(x, x, y, z, 1, 3, 28, 2, None) == EINVAL and 'multiple of 8' in _err(lib)
    assert _intact(xa, ya, za)
