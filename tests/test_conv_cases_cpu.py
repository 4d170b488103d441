"""CPU: tests/conv_cases.py -- the Python restatement of the convolution family's dispatch -- held to everything the built library reveals without a
launch (block counts, workspace bytes, route queries; no compute calls -- there is no GPU here), the conditions the case tables of
tests/test_gpu_conv_edges.py are named for, and the coverage statement: the tables together reach every instantiation the product library can
dispatch to.  A later change of a size rule that moves a case off its kernel fails here instead of thinning the coverage quietly.  The same for the
single-product bf16 inference route (csrc/conv_bf16.hip) and the tables of tests/test_gpu_conv_bf16_edges.py: the automatic rule against
straps_conv_bf16_tile_choice, every stated refusal against the entry point (refused before any launch), the ten configurations and the edge classes."""
import ctypes as C
import itertools

import pytest

import conv_cases as K
from straps_amd import hipabi


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _conv_cases():
    return K.FWD_EXPLICIT + K.FWD_AUTO + K.FWD_PLANES + K.DGRAD_EXPLICIT + K.DGRAD_S2_SMALL + K.DGRAD_AUTO


def test_plane_route_block_counts_agree_for_every_case(lib):
    """straps_conv_x3_stat_blocks / straps_conv_dgrad_x3_bn_blocks == the restatement, for every case under its own tile_cfg, under the twin's
    (the named tile / the shared-epilogue bit) and under the A/B bits"""
    n = 0
    for (B, H, W, ci, co, k, s, cfg) in _conv_cases():
        pad = K.pad_of(k)
        twins = {cfg, cfg | 256, cfg | 512, cfg | 512 | 1024, cfg | K.SHARED_EPILOGUE_BIT}
        p = K.fwd_problem(B, H, W, ci, co, k, s, pad)
        twins.add(K.x3_route(p, cfg, {'y', 'stats'})[0][1] if K.x3_route(p, cfg, {'y', 'stats'})[0][0] == 'x3' else cfg)
        for t in twins:
            assert lib.straps_conv_x3_stat_blocks(B, H, W, ci, co, k, k, s, pad, t) == K.x3_stat_blocks(B, H, W, ci, co, k, s, pad, t), (B, H, W, ci, co, k, s, t)
            if ci % 64 == 0 and co % 32 == 0:
                assert lib.straps_conv_dgrad_x3_bn_blocks(B, H, W, ci, co, k, k, s, pad, t) == K.dgrad_x3_bn_blocks(B, H, W, ci, co, k, s, pad, t), \
                    (B, H, W, ci, co, k, s, t)
            n += 1
    assert n > 1000


def test_plane_route_block_counts_agree_on_a_grid(lib):
    """the same over a grid of geometries around every threshold of the rules (128 / 256 / 512 tile equivalents, M % 128, halo slot limits)"""
    maps = [(1, 1, 1), (1, 3, 43), (2, 8, 8), (4, 4, 8), (1, 4, 64), (8, 16, 16), (4, 32, 32), (2, 64, 64), (1, 128, 127), (1, 128, 128), (1, 129, 128), (2, 128, 128),
            (2, 129, 128), (4, 128, 128), (4, 128, 129), (8, 128, 128), (1, 255, 257), (3, 91, 241), (16, 64, 64), (64, 16, 16), (128, 8, 8), (512, 8, 8), (32, 32, 32)]
    for (B, H, W), (ci, co), (k, s), cfg in itertools.product(maps, ((64, 64), (64, 128), (128, 64), (256, 256), (128, 512)), ((3, 1), (3, 2), (1, 1), (1, 2)),
                                                            (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 256, 512, 1536, 64)):
        pad = K.pad_of(k)
        assert lib.straps_conv_x3_stat_blocks(B, H, W, ci, co, k, k, s, pad, cfg) == K.x3_stat_blocks(B, H, W, ci, co, k, s, pad, cfg), (B, H, W, ci, co, k, s, cfg)
        assert lib.straps_conv_dgrad_x3_bn_blocks(B, H, W, ci, co, k, k, s, pad, cfg) == K.dgrad_x3_bn_blocks(B, H, W, ci, co, k, s, pad, cfg), (B, H, W, ci, co, k, s, cfg)
        if k == 1:
            for c5 in (0, 1, 2, 5):
                assert lib.straps_conv_x3f_stat_blocks(B, H, W, ci, co, 1, 1, s, 0, c5) == K.x3f_stat_blocks(B, H, W, ci, co, 1, s, 0, c5), (B, H, W, ci, co, s, c5)
                assert lib.straps_conv_dgrad_x3f_bn_blocks(B, H, W, ci, co, 1, 1, s, 0, c5) == K.dgrad_x3f_bn_blocks(B, H, W, ci, co, 1, s, 0, c5), (B, H, W, ci, co, s, c5)
    assert lib.straps_conv_x3f_stat_blocks(1, 8, 8, 64, 64, 3, 3, 1, 1, 0) == K.x3f_stat_blocks(1, 8, 8, 64, 64, 3, 1, 1, 0) == -1


def test_fp32_operand_route_queries_agree_for_every_case(lib):
    for (B, H, W, ci, co, s, cfg) in K.X3F_FWD:
        assert lib.straps_conv_x3f_supported(ci, co, 1, 1, s, 0) == K.x3f_supported(ci, co, 1, s, 0) == 1
        for t in (cfg, 0, 1, 2, 5):
            assert lib.straps_conv_x3f_stat_blocks(B, H, W, ci, co, 1, 1, s, 0, t) == K.x3f_stat_blocks(B, H, W, ci, co, 1, s, 0, t), (B, H, W, ci, co, s, t)
    for (B, H, W, ci, co, s, cfg) in K.X3F_DGRAD:
        assert lib.straps_conv_x3f_supported(ci, co, 1, 1, s, 0) == 1
        for t in (cfg, 0, 1, 2, 5):
            assert lib.straps_conv_dgrad_x3f_bn_blocks(B, H, W, ci, co, 1, 1, s, 0, t) == K.dgrad_x3f_bn_blocks(B, H, W, ci, co, 1, s, 0, t), (B, H, W, ci, co, s, t)
    for ci, co, k, s, pad in itertools.product((32, 64, 96, 128), (32, 64, 192), (1, 3), (1, 2, 3), (0, 1)):
        assert lib.straps_conv_x3f_supported(ci, co, k, k, s, pad) == K.x3f_supported(ci, co, k, s, pad)


def _wgrad_geometries():
    grid = [(B, H, W, ci, co, k, s) for (B, H, W) in ((1, 1, 1), (1, 4, 8), (3, 2, 16), (5, 6, 32), (7, 2, 64), (2, 10, 24), (1, 91, 91), (2, 128, 128), (3, 20, 20), (64, 16, 16))
            for (ci, co) in ((64, 64), (64, 128), (128, 64), (128, 256), (256, 128), (192, 128), (512, 512)) for (k, s) in ((3, 1), (3, 2), (1, 1), (1, 2))]
    return K.WGRAD_HALO + K.WGRAD_TAP + K.WGRAD_F32 + grid


def test_weight_gradient_queries_agree_and_every_plan_stays_inside_the_advertised_workspace(lib):
    """straps_conv_wgrad_workspace_bytes is the fp32 plan's size.  The kernels on the planes choose their own blocks, splits and chunk size: their
    partials -- splits x Cout x taps x Cin floats, every split written, the reduction reads exactly `splits` of them -- must fit."""
    for c in _wgrad_geometries():
        B, H, W, ci, co, k, s = c
        pad = K.pad_of(k)
        adv = lib.straps_conv_wgrad_workspace_bytes(B, H, W, ci, co, k, k, s, pad)
        assert adv == K.wgrad_workspace_bytes(B, H, W, ci, co, k, s, pad), c
        assert lib.straps_conv_wgrad_x3_on_planes(B, H, W, ci, co, k, k, s, pad) == int(K.wgrad_x3_route(B, H, W, ci, co, k, s, pad) != 0), c
        for planes in (True, False):
            pl = K.wgrad_plan(B, H, W, ci, co, k, s, pad, planes)
            assert 1 <= pl.splits and pl.splits * co * pl.taps * ci * 4 <= adv, (c, pl)
            assert pl.splits * pl.unit >= pl.units, (c, pl)          # the splits cover every pixel / chunk
    for (B, H, W, ci, co, s, bn) in K.WGRAD_X3F + [(b, h, w, ci, co, s, 0) for (b, h, w, ci, co, k, s) in _wgrad_geometries() if k == 1]:
        pl = K.wgrad_x3f_plan(B, H, W, ci, co, s, bn)
        assert lib.straps_conv_wgrad_x3f_workspace_bytes(B, H, W, ci, co, 1, 1, s, 0) == K.wgrad_x3f_workspace_bytes(B, H, W, ci, co, 1, s, 0) \
            == pl.splits * co * ci * 4, (B, H, W, ci, co, s)
        assert pl.splits * pl.unit >= pl.units
    assert lib.straps_conv_wgrad_x3f_workspace_bytes(1, 8, 8, 64, 64, 3, 3, 1, 1) == K.wgrad_x3f_workspace_bytes(1, 8, 8, 64, 64, 3, 1, 1) == 0


def _library_plan(lib, route, B, H, W, ci, co, k, s, pad):
    """straps_conv_wgrad_plan -> (the plan in conv_cases.py's terms, the raw struct)"""
    out = hipabi.WgradPlanStruct()
    assert lib.straps_conv_wgrad_plan(route, B, H, W, ci, co, k, k, s, pad, C.byref(out)) == 0, lib.straps_last_error()
    fam = hipabi.WG_FAMILIES[out.family]
    inst = {'wgrad_f32': (fam, out.bco), 'wgrad3_f32': (fam,), 'wgrad3_x3': (fam, out.chunk_px)}.get(fam, (fam, out.bco, out.bci))
    if fam in ('wgrad3_f32', 'wgrad3_x3'):
        assert (out.bco, out.bci) == (64, 64) and out.chunk_px == (32 if fam == 'wgrad3_f32' else inst[1])
    else:
        assert out.chunk_px == 0 and (fam != 'wgrad_f32' or out.bco == out.bci)
    return K.WPlan(inst, out.splits, out.unit, out.units, out.tiles, out.taps), out


W3PX = 32 + 112          # csrc/conv_wgrad_plan.h


def _lds_bytes(inst):
    """dynamic LDS of an instantiation: the per-tap formula of conv_cases.wgrad_clamp (the fp32-operand kernel stages the same image); elsewhere the
    constants of csrc/conv_wgrad.hip"""
    if inst[0] == 'wgrad3_x3':
        return {32: 2 * 3 * (32 + 128) * 64 * 2, 64: 2 * 3 * (64 + 136) * 64 * 2}[inst[1]]
    if inst[0] == 'wgrad3_f32':
        return 2 * 2 * W3PX * 64 * 4
    if inst[0] == 'wgrad_f32':
        return {64: 32 * 1024, 128: 64 * 1024}[inst[1]]
    return 2 * 3 * 32 * (inst[1] + inst[2]) * 2


def test_the_library_plan_is_the_restated_plan_field_by_field(lib):
    """straps_conv_wgrad_plan shows the ONE plan that sizing, routing and launch read (csrc/conv_wgrad_plan.h): for every geometry and both operand
    forms it equals conv_cases.wgrad_plan -- instantiation, splits, per-split extent, total extent, tiles, taps -- its partials are splits x Cout x
    taps x Cin floats and fit the advertised workspace, its LDS is the instantiation's; the same for the fp32-operand 1x1 route."""
    n = 0
    for c in _wgrad_geometries():
        B, H, W, ci, co, k, s = c
        pad = K.pad_of(k)
        adv = lib.straps_conv_wgrad_workspace_bytes(B, H, W, ci, co, k, k, s, pad)
        for planes in (True, False):
            want = K.wgrad_plan(B, H, W, ci, co, k, s, pad, planes)
            got, raw = _library_plan(lib, hipabi.WG_ROUTE_PLANES if planes else hipabi.WG_ROUTE_F32, B, H, W, ci, co, k, s, pad)
            assert got == want, (c, planes, got, want)
            assert raw.part_bytes == want.splits * co * want.taps * ci * 4 <= adv, (c, planes, raw.part_bytes, adv)
            assert raw.lds_bytes == _lds_bytes(want.inst), (c, planes, raw.lds_bytes)
            if not planes:
                assert raw.part_bytes == adv, c
            n += 1
        assert lib.straps_conv_wgrad_x3_on_planes(B, H, W, ci, co, k, k, s, pad) == int(K.wgrad_plan(B, H, W, ci, co, k, s, pad).inst[0] in ('wgrad_x3', 'wgrad3_x3')), c
    assert n > 600
    for (B, H, W, ci, co, s, bn) in K.WGRAD_X3F + [(b, h, w, ci, co, s, 0) for (b, h, w, ci, co, k, s) in _wgrad_geometries() if k == 1]:
        want = K.wgrad_x3f_plan(B, H, W, ci, co, s, bn)
        got, raw = _library_plan(lib, hipabi.WG_ROUTE_F32_1X1, B, H, W, ci, co, 1, s, 0)
        assert got == want._replace(inst=want.inst[:3]), (B, H, W, ci, co, s, got, want)          # (the operand-path BatchNorm is the call's, not the plan's)
        assert raw.part_bytes == want.splits * co * ci * 4 == lib.straps_conv_wgrad_x3f_workspace_bytes(B, H, W, ci, co, 1, 1, s, 0)
        assert raw.lds_bytes == _lds_bytes(want.inst)
    # geometries a route refuses: an error, no plan
    out = hipabi.WgradPlanStruct()
    assert lib.straps_conv_wgrad_plan(hipabi.WG_ROUTE_F32_1X1, 1, 8, 8, 64, 64, 3, 3, 1, 1, C.byref(out)) == 1 and b'1x1' in lib.straps_last_error()
    assert lib.straps_conv_wgrad_plan(hipabi.WG_ROUTE_PLANES, 1, 8, 8, 32, 64, 3, 3, 1, 1, C.byref(out)) == 1 and b'cin%64' in lib.straps_last_error()
    assert lib.straps_conv_wgrad_plan(7, 1, 8, 8, 64, 64, 3, 3, 1, 1, C.byref(out)) == 1
    assert lib.straps_conv_wgrad_plan(hipabi.WG_ROUTE_F32, 1, 8, 8, 64, 64, 3, 3, 1, 1, None) == 1


def test_the_tables_reach_every_instantiation_the_product_library_dispatches_to(lib):
    """the reached set is the LIBRARY's: every forward / data-gradient launch of the tables is named by straps_conv_plan (the weight gradients are held to
    straps_conv_wgrad_plan above), and the restatement names the same ones"""
    got = K.reached(lambda route, kind, g, cfg, ops: _plan_inst(_conv_plan(lib, route, kind, g, cfg, ops)))
    assert got == K.reached()
    missing = [i for i in K.REQUIRED if i not in got and i not in K.UNREACHABLE]
    assert not missing, 'no case reaches %s' % missing
    assert all(i in K.REQUIRED or i[0] == 'wgrad_x3' for i in K.UNREACHABLE)
    assert not [i for i in K.UNREACHABLE if i in got], 'listed as unreachable, but a case reaches it'
    assert not [i for i in got if i not in K.REQUIRED], 'an instantiation the coverage statement does not know'
    # what the issue names, spelled out: dispatch_x3_abl<0> cases 1-5 and 7-12, the three launch_x3h forms, every dispatch_lean form with EPI 1 and 2
    # (tile 9 excepted: unreachable), every x3f tile configuration, every weight-gradient block
    for cfg in (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12):
        assert ('x3', cfg, 0) in got
    for cfg, epi in itertools.product((3, 5, 7, 11, 12), (1, 2)):
        assert ('x3', cfg, epi) in got
    for epi in (0, 1, 2):
        assert ('x3h', 1, epi) in got and ('x3h', 3, epi) in got
    assert ('x3h', 2, 0) in got


def test_unreachable_instantiations_stay_unreachable_over_a_sweep():
    """lean tile 9: the rule picks tile 9 only for several one-tap classes, i.e. a 1x1 / stride-2 gradient, whose dead classes take the shared epilogue"""
    for (B, H, W), (ci, co), (k, s) in itertools.product(((1, 1, 1), (1, 1, 2), (2, 9, 14), (1, 255, 257), (2, 255, 257), (1, 512, 512), (4, 256, 256)),
                                                        ((128, 32), (256, 32), (512, 64), (1024, 64)), ((3, 1), (3, 2), (1, 1), (1, 2))):
        for kind, ops in [('fwd', K.fwd_ops('raw_stats'))] + [('dgrad', o) for o in K.DGRAD_FORMS.values()]:
            p = (K.fwd_problem(B, H, W, co, ci, k, s, K.pad_of(k)) if kind == 'fwd' else K.dgrad_problem(B, H, W, ci, co, k, s, K.pad_of(k)))
            inst = K.x3_route(p, 0, ops)[0]
            assert not (inst[:2] == ('x3', 9) and inst[2] != 0), (kind, B, H, W, ci, co, k, s, ops)
    for c in _wgrad_geometries():
        assert K.wgrad_plan(*c, K.pad_of(c[5])).inst not in K.UNREACHABLE


def test_explicit_tile_tables_hold_the_rows_they_are_named_for():
    for table, kind in ((K.FWD_EXPLICIT, 'fwd'), (K.DGRAD_EXPLICIT, 'dgrad')):
        seen = {}
        for (B, H, W, ci, co, k, s, cfg) in table:
            p = (K.fwd_problem if kind == 'fwd' else K.dgrad_problem)(B, H, W, ci, co, k, s, K.pad_of(k))
            inst, bm, _ = K.x3_route(p, cfg, {'y', 'stats'} if kind == 'fwd' else K.DGRAD_FORMS['addend'])
            assert inst == ('x3', cfg, 0) and bm == K.X3_BM[cfg]
            red = ci if kind == 'fwd' else co
            seen.setdefault((cfg, k, s, red), set()).add(max(x.M for x in p.cls))
        assert set(seen) == {(cfg, k, s, r) for cfg in K.X3_TILES for (k, s, r) in K.VARIANTS}
        for (cfg, k, s, r), ms in seen.items():
            bm = K.X3_BM[cfg]
            assert bm + 1 in ms and 2 * bm - 1 in ms and any(m < bm // 2 for m in ms), (cfg, ms)
    # H = 1 and W = 1 maps under a 3x3 / pad 1 filter at every row tile
    for bm, maps in K.EDGE_MAPS.items():
        assert any(h == 1 for _, h, w in maps) and any(w == 1 for _, h, w in maps), bm


def test_automatic_rule_tables_hold_the_classes_they_are_named_for():
    def fwd(c, form='raw_stats'):
        B, H, W, ci, co, k, s, cfg = c
        return K.x3_route(K.fwd_problem(B, H, W, ci, co, k, s, K.pad_of(k)), cfg, K.fwd_ops(form))
    want = [('x3', 7, 1)] * 2 + [('x3', 5, 1)] * 2 + [('x3', 12, 1)] * 2 + [('x3', 3, 1), ('x3', 7, 1)] + [('x3h', 1, 1)] * 2 + [('x3', 11, 1)] * 4 + [('x3h', 3, 1)] * 4 + \
           [('x3h', 2, 0)] * 2 + [('x3h', 1, 1)]
    assert [fwd(c)[0] for c in K.FWD_AUTO] == want
    assert [fwd(c, 'fused')[0] for c in K.FWD_AUTO] == [(a, b, 0) for (a, b, _) in want]
    # one row short of and one row past a multiple of the tile, in every size class of the 128-channel rule
    for short, past in ((0, 1), (2, 3), (4, 5)):
        bm = fwd(K.FWD_AUTO[short])[1]
        ms, mp = (K.FWD_AUTO[i][0] * K.FWD_AUTO[i][1] * K.FWD_AUTO[i][2] for i in (short, past))
        assert ms % bm == bm - 1 and mp % bm == 1
    # gradients: the lean form with an addend, bits and fused sums; the fp32-mask sums on the shared epilogue of the SAME tile
    for c in K.DGRAD_AUTO:
        B, H, W, ci, co, k, s, cfg = c
        p = K.dgrad_problem(B, H, W, ci, co, k, s, K.pad_of(k))
        r = {n: K.x3_route(p, cfg, o)[0] for n, o in K.DGRAD_FORMS.items()}
        if (k, s) == (1, 2):
            assert set(r.values()) == {('x3', 9, 0)}
            continue
        assert r['addend'][2] == r['bits'][2] == r['bn_mask'][2] == r['bn_bits'][2] == 2 and r['bn_out'] == r['addend'][:2] + (0,)
        assert K.x3_route(p, K.twin_cfg(p, cfg, K.DGRAD_FORMS['addend']), K.DGRAD_FORMS['addend'])[0] == r['addend'][:2] + (0,)
    got = [K.x3_route(K.dgrad_problem(*c[:7], K.pad_of(c[5])), 0, K.DGRAD_FORMS['addend'])[0][:2] for c in K.DGRAD_AUTO]
    assert got == [('x3', 7), ('x3', 5), ('x3', 12), ('x3h', 1), ('x3h', 3), ('x3h', 3), ('x3', 11), ('x3', 3), ('x3', 3), ('x3', 11), ('x3', 12), ('x3', 9), ('x3', 12)]
    # every stride-2 case has a ragged class
    for c in K.DGRAD_AUTO:
        if c[6] == 2:
            p = K.dgrad_problem(*c[:7], K.pad_of(c[5]))
            bm = K.x3_route(p, 0, K.DGRAD_FORMS['addend'])[1]
            assert len(p.cls) == 4 and any(x.M % bm for x in p.cls)


def test_stride_two_small_maps_have_one_two_and_four_classes_and_dead_ones():
    n = {}
    for c in K.DGRAD_S2_SMALL:
        B, H, W, ci, co, k, s, cfg = c
        p = K.dgrad_problem(B, H, W, ci, co, k, s, K.pad_of(k))
        n.setdefault(k, set()).add(len(p.cls))
        if k == 1:
            assert [x.ntaps for x in p.cls] == [1] + [0] * (len(p.cls) - 1)
        else:
            assert all(x.ntaps > 0 for x in p.cls)
    assert n == {1: {1, 2, 4}, 3: {1, 2, 4}}


def test_fp32_operand_tables_hold_the_streaming_conditions():
    fewer, one_more, by_rule = set(), set(), set()
    for table, prob, ops in ((K.X3F_FWD, K.fwd_problem, {'y', 'stats'}), (K.X3F_DGRAD, K.dgrad_problem, {'y', 'res', 'res_bits', 'bnr_raw'})):
        for (B, H, W, ci, co, s, cfg) in table:
            p = prob(B, H, W, ci, co, 1, s, 0)
            inst = K.x3f_route(p, cfg, ops)[0]
            if inst[0] != 'x3f_stream':
                continue
            wgs, mt = K.stream_workgroups(p, inst[1])
            full = max(1, min(2, (160 * 1024) // K.stream_lds_bytes(64 if inst[1] == 256 else 128, inst[1], 2, inst[1] == 256, p.Cin)) * 256 // (p.Cout // inst[1]))
            if mt < full:
                fewer.add((table is K.X3F_FWD, inst[1]))
            if mt > full and mt % full == 1:
                one_more.add((table is K.X3F_FWD, inst[1]))
            if cfg == 0:
                by_rule.add(table is K.X3F_FWD)
    assert fewer == {(f, bn) for f in (True, False) for bn in (256, 128, 64)}
    assert one_more == {(f, bn) for f in (True, False) for bn in (256, 128, 64)}
    assert by_rule == {True, False}


def test_weight_gradient_tables_hold_the_plans_they_are_named_for():
    plans = {c: K.wgrad_plan(*c, 1) for c in K.WGRAD_HALO}
    assert plans[(1, 4, 8, 64, 64, 3, 1)] == K.WPlan(('wgrad3_x3', 32), 1, 1, 1, 1, 9)                     # one chunk, one split
    assert {c[2] for c in K.WGRAD_HALO} == {8, 16, 32, 64}
    for w in (8, 16, 32, 64):
        assert {plans[c].inst[1] for c in K.WGRAD_HALO if c[2] == w} >= ({32, 64} if w < 64 else {32, 64})
    assert any(p.units % p.unit for p in plans.values() if p.inst[1] == 32) and any(p.units % p.unit for p in plans.values() if p.inst[1] == 64)
    # the 64-pixel plan is refused by the row count only: it has half the chunks of the 32-pixel plan, and half the chunks never need more splits
    for B, H, W, (ci, co) in itertools.product(range(1, 30), range(1, 13), (8, 16, 32, 64), ((64, 64), (128, 256), (384, 1024), (512, 1024))):
        p32, p64 = K.wgrad3_plan(B, H, W, ci, co, 3, 1, 1), K.wgrad3_plan(B, H, W, ci, co, 3, 1, 1, 64)
        if p32 and p64:
            assert p64[0] * 2 == p32[0] and p64[2] <= p32[2], (B, H, W, ci, co)
    # per-tap kernel: every block at M in {1, 31, 33, 129} where its rule admits them, a short / an empty last split, each bound of the split count
    by_block = {}
    for c in K.WGRAD_TAP:
        pl = K.wgrad_plan(*c, K.pad_of(c[5]))
        assert pl.inst[0] == 'wgrad_x3', c
        d = by_block.setdefault(pl.inst[1:], dict(M=set(), last=set(), clamp=set()))
        d['M'].add(pl.units); d['last'].add(K.last_split_state(pl)); d['clamp'].add(K.wgrad_clamp(*c, K.pad_of(c[5])))
    assert set(by_block) == {(256, 128), (128, 64), (64, 128), (128, 128), (64, 64)}
    for blk, d in by_block.items():
        if blk != (128, 128):                                   # (128 x 128: 1x1 layers from 8 192 pixels on only)
            assert {1, 31, 33, 129} <= d['M'], (blk, d['M'])
        assert {'short', 'empty'} <= d['last'], (blk, d['last'])
        assert {'max_s', 'target'} <= d['clamp'], (blk, d['clamp'])
    assert 'cap' in by_block[(256, 128)]['clamp']                # (the only block whose target exceeds the fp32 plan's count)
    # fp32-operand weight gradient: every block with and without the operand-path BatchNorm, at the four small pixel counts
    fb = {}
    for c in K.WGRAD_X3F:
        pl = K.wgrad_x3f_plan(*c)
        fb.setdefault(pl.inst[1:3], set()).add(pl.units)
    assert set(fb) == {(256, 64), (64, 256), (256, 128), (128, 256), (128, 128), (64, 64)} and all({1, 31, 33, 129} <= m for m in fb.values())
    assert 'empty' in {K.last_split_state(K.wgrad_x3f_plan(*c)) for c in K.WGRAD_X3F}
    assert {K.wgrad_plan(*c, K.pad_of(c[5]), planes=False).inst for c in K.WGRAD_F32} == {('wgrad3_f32',), ('wgrad_f32', 64), ('wgrad_f32', 128)}


# ----------------------------------------------------------------------------------------------------------------------------------------
# the launch plan of the forward / data-gradient convolutions (csrc/conv_plan.h) against the restatement

ROUTES = {'x3': hipabi.CONV_ROUTE_PLANES, 'x3f': hipabi.CONV_ROUTE_F32_1X1, 'bf16': hipabi.CONV_ROUTE_BF16}
KINDS = {'fwd': hipabi.CONV_KIND_FWD, 'dgrad': hipabi.CONV_KIND_DGRAD}


def _conv_plan(lib, route, kind, g, cfg, ops):
    """straps_conv_plan for g = (B, H, W, Cin, Cout, k, stride, pad) -> the raw struct"""
    B, H, W, ci, co, k, s, pad = g
    out = hipabi.ConvPlanStruct()
    rc = lib.straps_conv_plan(ROUTES[route], KINDS[kind], sum(hipabi.CONV_OPS[o] for o in ops), B, H, W, ci, co, k, k, s, pad, cfg, C.byref(out))
    assert rc == 0, (route, kind, g, cfg, ops, lib.straps_last_error())
    return out


def _plan_inst(out):
    """the instantiation a plan names, in conv_cases.py's terms"""
    fam = hipabi.CONV_FAMILIES[out.family]
    if fam in ('x3', 'x3h'):
        return (fam, out.tile, out.epilogue)
    if fam == 'x3f':
        return (fam, out.tile, out.epilogue, bool(out.abn))
    if fam == 'x3f_stream':
        return (fam, out.bn, out.epilogue, bool(out.abn))
    assert fam in ('bf16', 'bf16_halo') and out.epilogue == 3 and (fam == 'bf16_halo') == (out.tile in K.BF16_HALO)
    return ('bf16', out.tile)


def _restated_launch(route, kind, g, cfg, ops):
    """-> (instantiation, bm, blocks, (grid x, grid y), LDS bytes, threads) by conv_cases.py"""
    p = K._problem(kind, g)
    if route == 'bf16':
        inst = K.bf16_route(p, cfg)
        bm, bn = K.BF16_BM[inst[1]], K.BF16_BN[inst[1]]
        return (inst, bm, -(-p.cls[0].M // bm), K.launch_grid(p, bm, bn)) + K.bf16_lds_bytes(inst[1])
    inst, bm, blocks = (K.x3_route if route == 'x3' else K.x3f_route)(p, cfg, ops)
    if route == 'x3f':
        lds, threads, grid = K.x3f_lds_bytes(p, inst)
        return inst, bm, blocks, grid, lds, threads
    bn = K.X3_HALO_FORMS[inst[1]][0] if inst[0] == 'x3h' else K.X3_BN[inst[1]]
    return (inst, bm, blocks, K.launch_grid(p, bm, bn)) + K.x3_lds_bytes(inst)


def _hold_plan_to_restatement(lib, route, kind, g, cfg, ops):
    want = _restated_launch(route, kind, g, cfg, ops)
    out = _conv_plan(lib, route, kind, g, cfg, ops)
    got = (_plan_inst(out), out.bm, out.blocks, (out.grid_x, out.grid_y), out.lds_bytes, out.threads)
    assert got == want, (route, kind, g, cfg, sorted(ops), got, want)
    # the partial blocks are the M tiles of the classes, one class after the other
    p = K._problem(kind, g)
    assert out.ncls == len(p.cls) and list(out.mt)[:out.ncls] == [-(-c.M // out.bm) for c in p.cls] and sum(out.mt) == out.blocks
    assert list(out.part_base)[:out.ncls] == [sum(list(out.mt)[:i]) for i in range(out.ncls)] and out.nt * out.bn == p.Cout
    return out


def test_the_library_plan_names_the_restated_launch_for_every_case(lib):
    """straps_conv_plan == x3_route / x3f_route / bf16_route for every launch of the forward / data-gradient tables -- instantiation, row tile, partial
    blocks, grid, LDS bytes, threads; the streaming kernel's grid is stream_workgroups' -- under the case's own tile_cfg with every operand set the GPU
    files run it with, under its twin's, and (the fp32-operand route has no twin) under every tile_cfg of that route"""
    n = 0
    for cid, route, kind, g, cfg, ops, with_twin in K.launches():
        out = _hold_plan_to_restatement(lib, route, kind, g, cfg, ops)
        n += 1
        if route == 'x3' and out.epilogue:
            twin = K.twin_cfg(K._problem(kind, g), cfg, ops)
            t = _hold_plan_to_restatement(lib, route, kind, g, twin, ops)
            assert (t.family, t.tile, t.bm, t.bn, t.epilogue) == (out.family, out.tile, out.bm, out.bn, 0), (cid, twin)
        if route == 'x3f':
            for c5 in (0, 1, 2, 5):
                _hold_plan_to_restatement(lib, route, kind, g, c5, ops)
    assert n > 1800


def _m_map(M):
    return (1, 1, M)


T_EDGES = (127, 128, 255, 256, 511, 512)


def test_the_library_plan_is_the_restated_one_around_every_threshold_of_the_rules(lib):
    """the same comparison at the rules' thresholds (arithmetic only: the sizes are free), and every legacy block-count / tile-choice query is the plan's
    field for the operand set include/straps_hip.h states for it"""
    n = 0
    # plane routes: 128x128-tile equivalents per class = 127 / 128 / 255 / 256 / 511 / 512, one class (a forward) and four (a stride-2 gradient whose dx
    # has 4 t x 128 pixels), one-tap and nine-tap filters, 128- and 256-wide against the cout % 128 != 0 branch (64, 192); with and without the halo kernel
    for t, k, wide, cfg in itertools.product(T_EDGES, (1, 3), (128, 256, 64, 192), (0, 256, 512, 512 | 1024, 64)):
        rows = -(-t // (wide // 128)) if wide % 128 == 0 else t          # (t counts tiles of 128 columns: a 256-wide layer needs half the rows)
        for (B, H, W) in ((1, rows, 128), (1, 1, rows * 128 + 1), (rows, 16, 8)):
            g = (B, H, W, 32, wide, k, 1, K.pad_of(k))
            for ops in (K.fwd_ops('raw_stats'), K.fwd_ops('fused')):
                _hold_plan_to_restatement(lib, 'x3', 'fwd', g, cfg, ops)
            assert lib.straps_conv_x3_stat_blocks(B, H, W, 32, wide, k, k, 1, K.pad_of(k), cfg) == _conv_plan(lib, 'x3', 'fwd', g, cfg, {'y', 'stats'}).blocks
            n += 1
        g = (1, 2 * rows, 256, wide, 32, k, 2, K.pad_of(k))                   # dx: 512 x rows pixels in four parity classes
        for form in ('addend', 'bn_out', 'bn_bits'):
            _hold_plan_to_restatement(lib, 'x3', 'dgrad', g, cfg, K.DGRAD_FORMS[form])
        assert lib.straps_conv_dgrad_x3_bn_blocks(*g[:5], k, k, 2, K.pad_of(k), cfg) == _conv_plan(lib, 'x3', 'dgrad', g, cfg, {'y', 'res', 'bnr_raw'}).blocks
    # the size classes above are really on both sides of each threshold
    for t, want in zip(T_EDGES, (3, 7, 7, 5, 5, 12)):
        assert _plan_inst(_conv_plan(lib, 'x3', 'fwd', (1, t, 128, 32, 128, 1, 1, 0), 0, {'y', 'stats'})) == ('x3', want, 1)
    for t, want in zip(T_EDGES, (3, 11, 11, 9, 9, 12)):
        assert _plan_inst(_conv_plan(lib, 'x3', 'dgrad', (1, 2 * t, 256, 128, 32, 1, 2, 0), 0, K.DGRAD_FORMS['addend'])) == ('x3', want, 0)
    # fp32-operand route: 128x64 tiles of a class = 511 / 512 (shared epilogue: never the streaming kernel), one class and four
    for t, co, cfg in itertools.product((511, 512), (64, 128, 192), (0, 1, 2, 5)):
        rows = -(-t // (co // 64))
        for ops in K.X3F_FWD_FORMS.values():
            _hold_plan_to_restatement(lib, 'x3f', 'fwd', (1, rows, 128, 64, co, 1, 1, 0), cfg, ops)
        for ops in K.X3F_DGRAD_FORMS.values():
            _hold_plan_to_restatement(lib, 'x3f', 'dgrad', (1, 2 * rows, 256, co, 64, 1, 2, 0), cfg, ops)
            _hold_plan_to_restatement(lib, 'x3f', 'dgrad', (1, rows, 128, co, 64, 1, 1, 0), cfg, ops)
        n += 1
    assert [_plan_inst(_conv_plan(lib, 'x3f', 'fwd', (1, t, 128, 64, 64, 1, 1, 0), 0, K.X3F_FWD_FORMS['eval']))[:2] for t in (511, 512)] == [('x3f', 2), ('x3f', 1)]
    # ... and the streaming rule's bound M >= 4 x 128 x (256 / N tiles) at M - 1 / M, for each width of its tile and an N-tile count that does not divide 256
    for ci, co, sbn in ((64, 64, 64), (64, 128, 128), (64, 256, 256), (64, 1024, 256), (128, 1024, 128), (64, 192, 64), (128, 64, 64)):
        bound = 4 * 128 * (256 // (co // sbn))
        for M, stream in ((bound - 1, False), (bound, True)):
            for ops in K.X3F_FWD_FORMS.values():
                out = _hold_plan_to_restatement(lib, 'x3f', 'fwd', _m_map(M) + (ci, co, 1, 1, 0), 0, ops)
                lean = 'scale' not in ops
                assert (hipabi.CONV_FAMILIES[out.family] == 'x3f_stream') == (stream and lean) and (not (stream and lean) or out.bn == sbn), (ci, co, M, sorted(ops))
            for name, ops in K.X3F_DGRAD_FORMS.items():
                out = _hold_plan_to_restatement(lib, 'x3f', 'dgrad', _m_map(M) + (co, ci, 1, 1, 0), 0, ops)
                assert (hipabi.CONV_FAMILIES[out.family] == 'x3f_stream') == stream and out.epilogue == (2 if name == 'full' else 1), (ci, co, M, name)      # (a plain stride-1 gradient is the lean FORWARD form)
            g = _m_map(M) + (ci, co, 1, 1, 0)
            assert lib.straps_conv_x3f_stat_blocks(*g[:5], 1, 1, 1, 0, 0) == _conv_plan(lib, 'x3f', 'fwd', g, 0, {'y', 'stats'}).blocks
            g = _m_map(M) + (co, ci, 1, 1, 0)
            assert lib.straps_conv_dgrad_x3f_bn_blocks(*g[:5], 1, 1, 1, 0, 0) == _conv_plan(lib, 'x3f', 'dgrad', g, 0, {'y', 'bnr_raw'}).blocks
            n += 1
    # the geometry grid of the block-count test above: the legacy queries are the plan's fields there too
    maps = [(1, 1, 1), (1, 3, 43), (2, 8, 8), (4, 4, 8), (1, 4, 64), (8, 16, 16), (4, 32, 32), (2, 64, 64), (1, 128, 127), (1, 128, 128), (1, 129, 128), (2, 128, 128),
            (4, 128, 129), (8, 128, 128), (1, 255, 257), (3, 91, 241), (16, 64, 64), (64, 16, 16), (128, 8, 8), (512, 8, 8), (32, 32, 32)]
    for (B, H, W), (ci, co), (k, s), cfg in itertools.product(maps, ((64, 64), (64, 128), (128, 64), (256, 256), (128, 512)), ((3, 1), (3, 2), (1, 1), (1, 2)),
                                                            (0, 1, 3, 5, 6, 9, 12, 13, 256, 512, 1536, 64)):
        g = (B, H, W, ci, co, k, s, K.pad_of(k))
        assert lib.straps_conv_x3_stat_blocks(B, H, W, ci, co, k, k, s, g[7], cfg) == _hold_plan_to_restatement(lib, 'x3', 'fwd', g, cfg, {'y', 'stats'}).blocks
        assert lib.straps_conv_dgrad_x3_bn_blocks(B, H, W, ci, co, k, k, s, g[7], cfg) == _hold_plan_to_restatement(lib, 'x3', 'dgrad', g, cfg, {'y', 'res', 'bnr_raw'}).blocks
        if k == 1 and cfg in (0, 1, 5, 6):
            assert lib.straps_conv_x3f_stat_blocks(B, H, W, ci, co, 1, 1, s, 0, cfg) == _hold_plan_to_restatement(lib, 'x3f', 'fwd', g, cfg, {'y', 'stats'}).blocks
            if s == 1:
                assert lib.straps_conv_dgrad_x3f_bn_blocks(B, H, W, ci, co, 1, 1, s, 0, cfg) == _hold_plan_to_restatement(lib, 'x3f', 'dgrad', g, cfg, {'y', 'bnr_raw'}).blocks
            else:
                assert lib.straps_conv_dgrad_x3f_bn_blocks(B, H, W, ci, co, 1, 1, s, 0, cfg) == _conv_plan(lib, 'x3f', 'dgrad', g, cfg, {'y', 'bnr_raw'}).blocks
        n += 1
    # bf16 route: 255 / 256 / 511 / 512 tile equivalents, M one short of and one past a multiple of 128, cout % 128
    for M, co, (k, s) in itertools.product((1, 127, 128, 129, 255 * 128, 255 * 128 + 1, 256 * 128 - 1, 256 * 128, 256 * 128 + 1, 511 * 128, 511 * 128 + 1, 512 * 128, 1024 * 128),
                                           (64, 128, 192, 256, 320, 512), ((1, 1), (3, 1))):
        for (B, H, W) in ((1, 1, M), (1, M, 1)) + (((M // 128, 16, 8),) if M % 128 == 0 else ()):
            out = _hold_plan_to_restatement(lib, 'bf16', 'fwd', (B, H, W, 64, co, k, s, k // 2), 0, {'y', 'yplanes'})
            assert lib.straps_conv_bf16_tile_choice(B, H, W, 64, co, k, k, s, k // 2) == out.tile
            n += 1
    # fp32 implicit GEMM: straps_conv_stat_blocks is the plan's `blocks` (the fp32 rule reads no operand)
    for (B, H, W), (ci, co), k, cfg in itertools.product(maps, ((64, 64), (64, 128), (256, 256), (128, 512)), (1, 3), (0, 1, 2, 3, 4, 16, 20, 32, 36)):
        out = hipabi.ConvPlanStruct()
        assert lib.straps_conv_plan(hipabi.CONV_ROUTE_F32, hipabi.CONV_KIND_FWD, 3, B, H, W, ci, co, k, k, 1, K.pad_of(k), cfg, C.byref(out)) == 0
        assert hipabi.CONV_FAMILIES[out.family] == 'igemm_f32' and lib.straps_conv_stat_blocks(B, H, W, co, k * k * ci, cfg) == out.blocks == -(-B * H * W // out.bm)
        assert (out.grid_x, out.grid_y, out.threads) == (out.blocks * (co // out.bn), 1, 256)
        assert out.lds_bytes == (2 * (out.bm + out.bn) * 36 * 4 if (cfg & 48) == 16 else 2 * (out.bm + out.bn) * 32 * 4)
        n += 1
    assert n > 7000


def test_the_library_plan_refuses_what_the_entry_points_refuse(lib):
    """every refusal is STRAPS_EINVAL with its reason; a NULL `out` is refused"""
    out = hipabi.ConvPlanStruct()
    F, X, O, H = hipabi.CONV_ROUTE_F32, hipabi.CONV_ROUTE_PLANES, hipabi.CONV_ROUTE_F32_1X1, hipabi.CONV_ROUTE_BF16

    def refused(why, route, kind, geom, cfg=0):
        assert lib.straps_conv_plan(route, kind, 1, *geom, cfg, C.byref(out)) == 1, (why, route, kind, geom)
        err = lib.straps_last_error().decode()
        assert err.startswith('straps_conv_plan: ') and why in err, (why, err)

    ok = (2, 8, 8, 64, 64, 3, 3, 1, 1)
    assert lib.straps_conv_plan(X, 0, 1, *ok, 0, None) == 1 and b'null pointer' in lib.straps_last_error()
    refused('unknown route', 4, 0, ok)
    refused('unknown route', -1, 0, ok)
    refused('kind is 0', X, 2, ok)
    refused('forward only', H, 1, ok)
    for route in (F, X, O, H):
        refused('empty input', route, 0, (0, 8, 8, 64, 64, 1, 1, 1, 0))
    for route in (F, X):
        refused('cin%32==0 and cout%64==0', route, 0, (2, 8, 8, 48, 64, 3, 3, 1, 1))
        refused('cin%32==0 and cout%64==0', route, 0, (2, 8, 8, 32, 96, 3, 3, 1, 1))
        refused('bad filter geometry', route, 0, (2, 8, 8, 64, 64, 5, 5, 1, 2))
        refused('bad filter geometry', route, 0, (2, 8, 8, 64, 64, 3, 3, 0, 1))
        refused('cout%32==0 and cin%64==0', route, 1, (2, 8, 8, 32, 64, 3, 3, 1, 1))
        refused('stride must be 1 or 2', route, 1, (2, 8, 8, 64, 64, 3, 3, 3, 1))
        refused('unsupported filter geometry', route, 1, (2, 8, 8, 64, 64, 3, 3, 1, 3))
    refused('1x1 filters without padding only', O, 0, ok)
    refused('1x1 filters without padding only', O, 0, (2, 8, 8, 64, 64, 1, 1, 1, 1))
    refused('1x1 filters without padding, stride 1 or 2 only', O, 1, ok)
    refused('1x1 filters without padding, stride 1 or 2 only', O, 1, (2, 8, 8, 64, 64, 1, 1, 3, 0))
    refused('cin%64==0 and cout%64==0', H, 0, (2, 8, 8, 32, 64, 3, 3, 1, 1))
    refused('tile_cfg must be in [0, 10]', H, 0, ok, 11)
    refused('tile_cfg must be in [0, 10]', H, 0, ok, -1)
    # the bf16 route's configuration refusals: every (case, configuration) the restatement refuses, with its reason
    n = 0
    for c in K.BF16_EXPLICIT:
        p = K.bf16_problem(c)
        for cfg in K.BF16_TILES:
            why = K.bf16_refusal(p, cfg)
            if why is not None:
                refused('tile_cfg %d: %s' % (cfg, why), H, 0, _bf16_geo(c), cfg)
                n += 1
    assert n > 100


# ----------------------------------------------------------------------------------------------------------------------------------------
# the single-product bf16 inference route (csrc/conv_bf16.hip): the tables of tests/test_gpu_conv_bf16_edges.py

def _bf16_geo(c):
    B, H, W, ci, co, k, s = c
    return (B, H, W, ci, co, k, k, s, k // 2)


def test_bf16_tile_choice_is_the_restated_rule(lib):
    """straps_conv_bf16_tile_choice == pick_tile_bf16 for every case of both tables and on a grid around the rule's thresholds (255 / 256 / 511 /
    512 tile equivalents, M one short of and one past a multiple of 128, cout % 128); the automatic cases land on the configurations they are named for"""
    for c in K.BF16_EXPLICIT + K.BF16_AUTO:
        p = K.bf16_problem(c)
        assert lib.straps_conv_bf16_tile_choice(*_bf16_geo(c)) == K.pick_tile_bf16(p.cls[0].M, p.Cout), c
    assert [K.bf16_route(K.bf16_problem(c), 0)[1] for c in K.BF16_AUTO] == K.BF16_AUTO_WANT
    assert [lib.straps_conv_bf16_tile_choice(*_bf16_geo(c)) for c in K.BF16_AUTO] == K.BF16_AUTO_WANT
    n = 0
    for M, co, (k, s) in itertools.product((1, 127, 128, 129, 255 * 128, 255 * 128 + 1, 256 * 128 - 1, 256 * 128, 256 * 128 + 1, 511 * 128, 511 * 128 + 1, 512 * 128, 1024 * 128),
                                           (64, 128, 192, 256, 320, 512), ((1, 1), (3, 1))):
        for (B, H, W) in ((1, 1, M), (1, M, 1)) + (((M // 128, 16, 8),) if M % 128 == 0 else ()):
            assert lib.straps_conv_bf16_tile_choice(B, H, W, 64, co, k, k, s, k // 2) == K.pick_tile_bf16(M, co), (B, H, W, co, k)
            n += 1
    assert n > 300
    # every configuration the rule can return admits every geometry it returns it for (cfg 3: cout % 64, cfg 1 / 5: only at cout % 128 == 0)
    for c in K.BF16_EXPLICIT + K.BF16_AUTO:
        p = K.bf16_problem(c)
        assert K.bf16_refusal(p, K.pick_tile_bf16(p.cls[0].M, p.Cout)) is None


V = C.c_void_p(8192)          # a non-null, 16-byte aligned address that is never dereferenced: the calls below are refused before any launch


def test_bf16_refusals_are_the_restated_ones(lib):
    """every (case, configuration) the restatement of cfg_refusal refuses is refused by straps_conv_fwd_bf16 with that reason -- the call returns before
    anything is launched (the operand pointers are no memory at all).  That the admitted ones run is asserted on the GPU."""
    n = 0
    why_seen = set()
    for c in K.BF16_EXPLICIT:
        p = K.bf16_problem(c)
        for cfg in K.BF16_TILES:
            why = K.bf16_refusal(p, cfg)
            if why is None:
                continue
            rc = lib.straps_conv_fwd_bf16(V, V, None, None, None, 0, V, V, *_bf16_geo(c), cfg, None)
            assert rc != 0 and why in lib.straps_last_error().decode(), (c, cfg, rc, lib.straps_last_error())
            assert ('tile_cfg %d:' % cfg) in lib.straps_last_error().decode()
            why_seen.add(why)
            n += 1
    assert why_seen == {K.BF16_WHY_N, K.BF16_WHY_K, K.BF16_WHY_HALO[9], K.BF16_WHY_HALO[10]} and n > 100
    assert K.bf16_refusal(K.bf16_problem(K.BF16_EXPLICIT[0]), 11) == 'unknown tile configuration'


def test_bf16_tables_reach_all_ten_configurations_and_hold_every_edge_class():
    """asserted on the tables, so that a later edit cannot drop an edge quietly"""
    got = K.reached()
    for cfg in K.BF16_TILES:
        assert ('bf16', cfg) in got and ('bf16', cfg) in K.REQUIRED
    assert len(set(K.BF16_EXPLICIT)) == len(K.BF16_EXPLICIT) and len(set(K.BF16_AUTO)) == len(K.BF16_AUTO)
    ran = {}          # cfg -> [(case, problem)] of the launches
    refused = {}      # cfg -> [(case, problem, reason)]
    for c in K.BF16_EXPLICIT:
        p = K.bf16_problem(c)
        for cfg in K.BF16_TILES:
            why = K.bf16_refusal(p, cfg)
            (ran if why is None else refused).setdefault(cfg, []).append((c, p) if why is None else (c, p, why))

    # ---- K-loop length: 1x1 layers with 1, 2, 3, 4 stages where PL allows (PL = 1: 2, 4, 6, 8; PL = 4: 1, 2, 3), on every non-halo configuration:
    # fewer chunks than the prologue issues (NST - 1; the pipelined loops NST), exactly as many, and one more
    for cfg in (1, 2, 3, 4, 5, 6, 7, 8):
        n1 = {K.bf16_nchunks(p, cfg) for c, p in ran[cfg] if c[5] == 1}
        assert n1 >= {1: {2, 4, 6, 8}, 4: {1, 2, 3}}.get(K.BF16_PL[cfg], {1, 2, 3, 4}), (cfg, n1)
        pro = K.BF16_NST[cfg] if cfg in K.BF16_PIPE else K.BF16_NST[cfg] - 1
        if K.BF16_PL[cfg] != 1:
            assert {pro - 1, pro, pro + 1} - {0} <= n1, (cfg, pro, n1)
        # 3x3 with the fewest stages per tap the configuration can have (one: the tap rolls over at every stage; PL = 1: two -- cin % 64) and with more
        per_tap = {(p.Cin // 32) // K.BF16_PL[cfg] for c, p in ran[cfg] if c[5] == 3}
        least = 2 if K.BF16_PL[cfg] == 1 else 1
        assert least in per_tap and any(x > least for x in per_tap), (cfg, per_tap)
    assert {c[3] for c, p, why in refused[6] if why == K.BF16_WHY_K and c[5] == 1} >= {64, 192}
    assert (2, 9, 9, 64, 128, 3, 1) in K.BF16_EXPLICIT and (2, 9, 9, 128, 128, 3, 1) in K.BF16_EXPLICIT

    # ---- M edges per row tile: 1, BM - 1, BM, BM + 1, a ragged two-tile M -- on every non-halo configuration of that BM (cfg 6: by its 3x3 / cin 128 cases
    # and M = 1 only -- the 1x1 edges are cin 64)
    for cfg in (1, 2, 3, 4, 5, 7, 8):
        bm = K.BF16_BM[cfg]
        ms = {p.cls[0].M for c, p in ran[cfg]}
        assert {1, bm - 1, bm, bm + 1} <= ms and any(bm + 1 < m < 2 * bm and m % bm for m in ms), (cfg, sorted(ms))
    assert 1 in {p.cls[0].M for c, p in ran[6]} and any(p.cls[0].M % 128 for c, p in ran[6])
    assert (1, 1, 1, 64, 64, 1, 1) in K.BF16_EXPLICIT
    # ---- padding pixels: 3x3 at H = W = 1 and H = 1, W = 3, at PL = 2 and (cin 128) PL = 4
    for hw in ((1, 1), (1, 3)):
        for ci in (64, 128):
            assert (1,) + hw + (ci, 128, 3, 1) in K.BF16_EXPLICIT
    # ---- stride 2 on odd extents, 3x3 and 1x1
    assert (3, 7, 9, 64, 128, 3, 2) in K.BF16_EXPLICIT and (2, 7, 5, 128, 64, 1, 2) in K.BF16_EXPLICIT
    # ---- N edges: cout 64, 128, 192, 320; 192 and 320 run on the 64-wide tiles only, the 128-wide ones refuse them
    assert {c[4] for c in K.BF16_EXPLICIT} >= {64, 128, 192, 320}
    for co in (192, 320):
        for cfg in K.BF16_TILES:
            wide = K.BF16_BN[cfg] == 128
            assert any(c[4] == co and why == K.BF16_WHY_N for c, p, why in refused.get(cfg, [])) == wide, (co, cfg)
            if not wide and cfg not in K.BF16_HALO:
                assert any(c[4] == co for c, p in ran[cfg]), (co, cfg)
    # ---- halo tiles: the slot counts the cases are named for
    slots = {c: K.halo_patch_slots(K.bf16_problem(c)) for c in K.BF16_HALO_RUN + K.BF16_HALO_REFUSED}
    for ci in (64, 128):
        assert [slots[(b, h, w, ci, 128, 3, 1)] for (b, h, w) in ((2, 8, 8), (1, 16, 8), (1, 16, 16), (1, 32, 32))] == [200, 180, 180, 204]
        for (b, h, w) in ((2, 8, 8), (1, 16, 8), (1, 16, 16), (1, 32, 32)):
            assert ((b, h, w, ci, 128, 3, 1), K.bf16_problem((b, h, w, ci, 128, 3, 1))) in ran[9] and ((b, h, w, ci, 128, 3, 1), K.bf16_problem((b, h, w, ci, 128, 3, 1))) in ran[10]
    assert slots[(1, 64, 64, 64, 64, 3, 1)] == slots[(1, 64, 64, 64, 128, 3, 1)] == 264          # cfg 10 alone
    for c in ((1, 64, 64, 64, 64, 3, 1), (1, 64, 64, 64, 128, 3, 1)):
        assert K.bf16_refusal(K.bf16_problem(c), 10) is None and K.bf16_refusal(K.bf16_problem(c), 9) is not None
    assert K.bf16_refusal(K.bf16_problem((1, 64, 64, 64, 128, 3, 1)), 9) == K.BF16_WHY_HALO[9]      # (by the slot limit, not by cout)
    assert slots[(8, 4, 4, 64, 128, 3, 1)] == 288
    kinds = set()
    for c in K.BF16_HALO_REFUSED:
        p = K.bf16_problem(c)
        assert K.bf16_refusal(p, 9) == K.BF16_WHY_HALO[9] and K.bf16_refusal(p, 10) == K.BF16_WHY_HALO[10], c
        kinds.add('slots' if slots[c] > 272 else 'stride' if c[6] == 2 else '1x1' if c[5] == 1 else 'ragged' if p.cls[0].M % 128 else '?')
    assert kinds == {'slots', 'stride', '1x1', 'ragged'}
    # ---- the automatic rule: t128 = 255 / 256 / 511 / 512 at cout 128; 64 and 192 output channels at 512 M tiles
    t = [(-(-K.bf16_problem(c).cls[0].M // 128) * (c[4] // 128), c[4]) for c in K.BF16_AUTO]
    assert t[:4] == [(255, 128), (256, 128), (511, 128), (512, 128)] and (0, 64) in t and (512, 192) in t
    assert all(-(-K.bf16_problem(c).cls[0].M // 128) >= 512 for c in K.BF16_AUTO if c[4] != 128)
    # ---- batch independence: a 128-row tile that spans three images; a halo patch of two images
    assert ((3, 5, 5, 128, 128, 3, 1), 1) in K.BF16_BATCH and ((2, 8, 8, 64, 128, 3, 1), 9) in K.BF16_BATCH
    for c, cfg in K.BF16_BATCH:
        assert K.bf16_refusal(K.bf16_problem(c), cfg) is None and c[1] * c[2] < K.BF16_BM[cfg]
    # ---- split and pack: both sides of the grid cap (the second trip of the grid-stride loop), the small shapes, the 1x3 and 3x1 filters
    n4 = [r * c // 4 for r, c in K.BF16_SPLIT]
    assert any(n == K.BF16_GRID_CAP for n in n4) and any(K.BF16_GRID_CAP < n <= K.BF16_GRID_CAP + 4096 for n in n4)
    assert {(1, 32), (1, 64), (3, 96), (257, 32)} <= set(K.BF16_SPLIT)
    assert any(o * ci * kh * kw > K.BF16_GRID_CAP for o, ci, kh, kw in K.BF16_PACK)
    assert {(64, 32, 1, 1), (64, 64, 3, 3), (192, 96, 3, 3), (1, 32, 3, 3), (64, 64, 1, 3), (64, 64, 3, 1)} <= set(K.BF16_PACK)
