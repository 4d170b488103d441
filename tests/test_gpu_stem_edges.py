"""GPU: the stem kernels (csrc/stem.hip, the stem part of csrc/backward.hip, csrc/stem_dgrad.hip, the proxy builders of csrc/train.hip) at their tile,
channel-pass, mask-word and walk edges, behind redzones (tests/redzone.py) -- the cases of tests/stem_cases.py, which also states what each case
reaches (tests/test_stem_cases_cpu.py holds that statement together).

Common form:
  * every output (y, the statistics partials of exactly straps_stem_stat_blocks rows, mask words, tile bytes, dw, dx, packed weights) and the weight
    gradient's workspace of exactly straps_stem_wgrad_workspace_bytes come from Zone.guarded: NaN-filled (0x5A / 0xEE patterns for words and bytes),
    sentinel margins on both sides, checked after the calls;
  * every operand (x, packed weights, dy, masks, prior gradients) comes from Zone.at_end: poison directly behind its last element, a 256-byte aligned
    start; the margin behind a mask is the NaN word 0x7FC00000 -- bits 22 .. 30 set: an over-read marks cells active, which the exact activity
    comparisons show;
  * references are float64 evaluations on the CPU from the same fp32 operands (tests/stem_cases.py), never another kernel of the library.

Bounds (derived, not tuned: a chain of K fused fp32 terms in any order is within (K - 1) u of its sum of absolute terms, u = 2^-24; the 16 and the 8 are
slack, as in tests/head_cases.py):
  forward raw    |y - ref| <= (49 C + 16) u sum|x w|                     and the older bar 2e-5 + 2e-5 |ref|
  fused          |scale| times that + u |want|
  dw             (B Ho Wo + 16) u sum|x dy|                               and 2e-5 of max|ref|
  dx             (1024 + 16) u sum|dy w|                                  and 1e-5 of max|ref|
  statistics     per (block, channel) against the float64 sum of the kernel's OWN y over the tile's in-range pixels: (n + 8) u sum|terms|
Integer (tracer, single_pixel, proxy_like) cases are compared with ==, statistics partials included.  Every bounded check prints `RATIO <kernel> <worst>`.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import stem_cases as S
import straps_amd  # noqa: F401
import straps_oracle as O
from detgen import det_uniform
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
P = hipabi.ptr
U = S.U
WORD_FILL, BYTE_FILL = 0x5A5A5A5A, 0xEE


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    lib = hipabi.load()
    import os
    assert os.path.abspath(lib._name) == os.path.abspath(hipabi.LIB_PATH), 'these tests run on the product library, not %s' % lib._name
    return torch.device('cuda:0')


def _by_shape(cases):
    d = OrderedDict()
    for c in cases:
        d.setdefault(c.shape, []).append(c)
    return d


FWD = _by_shape(S.cases('fwd'))
WGRAD = _by_shape(S.cases('wgrad'))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b, nan_ok=False):
    """bit for bit; nan_ok (the one-NaN-pixel cases): a NaN may meet a NaN of another payload -- which operand's payload an addition keeps is not
    part of what is tested"""
    if nan_ok:
        a, b = a.detach().cpu(), b.detach().cpu()
        na, nb = torch.isnan(a), torch.isnan(b)
        return bool(torch.equal(na, nb)) and bool(torch.equal(_bits(a)[~na], _bits(b)[~nb]))
    return bool(torch.equal(_bits(a), _bits(b)))


def _plus_zero(t):
    return not bool(_bits(t).any())


def _words(t):
    return t.detach().cpu().numpy().view(np.uint32).reshape(-1)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _bounded(got, want, bound, what, bar=None):
    """element by element |got - want| <= bound wherever the reference is a number, NaN exactly where it is not; -> worst error / bound"""
    got = got.detach().cpu().double()
    nan = torch.isnan(want)
    assert bool(torch.equal(torch.isnan(got), nan)), '%s: NaN pattern differs (an element nobody wrote, a read past an operand, or a skipped NaN)' % what
    ok = ~nan
    assert bool(torch.isfinite(got[ok]).all()), '%s: not finite' % what
    err = (got[ok] - want[ok]).abs()
    ratio = err / bound[ok].clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('RATIO %s %.4f' % (what, worst))
    assert worst <= 1.0, '%s: error %.3e against a bound of %.3e' % (what, float(err[ratio.argmax()]), float(bound[ok][ratio.argmax()]))
    if bar is not None and ratio.numel():
        assert bool((err <= bar[ok] if isinstance(bar, torch.Tensor) else err <= bar).all()), '%s: the older bar no longer holds' % what
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------ runners

def _pack_fwd(z, L, w):
    C = w.shape[1]
    wd = z.at_end(w.contiguous())
    wf = z.guarded((L.straps_stem_weight_floats(C),), name='packed stem weight')
    hipabi.check(L.straps_pack_stem_weight(P(wd), P(wf), C, None), 'pack stem')
    assert _same_bits(wf.cpu(), torch.from_numpy(S.pack_stem_weight_ref(w.numpy()))), 'straps_pack_stem_weight differs from the layout comment'
    return z.at_end(wf)


def _nzmask(z, L, xd, shape):
    B, C, H, W = shape
    nw = L.straps_stem_nzmask_words(B, C, H, W)
    m = z.guarded((nw,), torch.int32, fill=WORD_FILL, name='nzmask')
    hipabi.check(L.straps_stem_nzmask(P(xd), P(m), B, C, H, W, None), 'nzmask')
    return m


def _tile_activity(z, L, maskd, shape):
    B, C, H, W = shape
    t = z.guarded((L.straps_stem_tiles(B, H, W),), torch.uint8, fill=BYTE_FILL, name='tile activity')
    hipabi.check(L.straps_stem_tile_activity(P(maskd), P(t), B, C, H, W, None), 'tile activity')
    return t


def _masks(z, L, xd, case):
    """-> [None, the kernel's own mask, all ones] as operands at the end of poison; the own mask and the tile activity are held to the references"""
    shape = case.shape
    B, C, H, W = shape
    ref = S.case_mask(case).reshape(-1)
    own = _nzmask(z, L, xd, shape)
    assert np.array_equal(_words(own), ref), '%s: straps_stem_nzmask differs from nzmask_ref in %d words' % (case.id, int((_words(own) != ref).sum()))
    refd = z.at_end(torch.from_numpy(ref.view(np.int32).copy()))
    ownd = z.at_end(own)
    want = S.tile_any_ref(S.case_mask(case), B, C, H, W)
    for m in (ownd, refd):
        t = _tile_activity(z, L, m, shape)
        assert np.array_equal(t.cpu().numpy(), want), '%s: straps_stem_tile_activity differs from tile_any_ref' % case.id
    ones = z.at_end(torch.full((ref.size,), -1, dtype=torch.int32))
    return [None, ownd, ones]


def _fwd(z, L, xd, wf, mask, shape, stats=True, scale=None, shift=None, relu=0):
    B, C, H, W = shape
    Ho, Wo = S.out_hw(H, W)
    y = z.guarded((B, Ho, Wo, 64), name='y')
    part = z.guarded((L.straps_stem_stat_blocks(B, H, W), 64, 2), name='statistics partials') if stats else None
    hipabi.check(L.straps_stem_fwd(P(xd), P(wf), P(scale), P(shift), relu, P(y), P(part), P(mask), B, C, H, W, None), 'stem fwd')
    return y, part


def _wgrad(z, L, xd, dyd, mask, shape, accumulate=0, dw=None, ws=None):
    B, C, H, W = shape
    nbytes = L.straps_stem_wgrad_workspace_bytes(B, C, H, W)
    assert nbytes == S.wgrad_workspace_bytes(B, C, H, W) and nbytes % 4 == 0
    if ws is None:
        ws = z.guarded((nbytes // 4,), name='wgrad workspace')           # NaN-filled: a partial read before it is written is a NaN in dw
    if dw is None:
        dw = z.guarded((64, C, 7, 7), name='dw')
    hipabi.check(L.straps_stem_wgrad(P(xd), P(dyd), P(dw), P(ws), P(mask), B, C, H, W, accumulate, None), 'stem wgrad')
    return dw, ws


def _pack_dgrad(z, L, w):
    C = w.shape[1]
    wd = z.at_end(w.contiguous())
    n = L.straps_stem_dgrad_weight_floats(C)
    assert n == S.dgrad_weight_floats(C)
    wp = z.guarded((n,), name='packed dgrad weight')
    hipabi.check(L.straps_pack_stem_dgrad_weight(P(wd), P(wp), C, None), 'pack stem dgrad')
    assert _same_bits(wp.cpu(), torch.from_numpy(S.pack_stem_dgrad_weight_ref(w.numpy()))), 'straps_pack_stem_dgrad_weight differs from the layout comment (zero taps are +0.0)'
    return z.at_end(wp)


def _dgrad(z, L, dyd, wp, shape, accumulate=0, dx=None):
    B, C, H, W = shape
    if dx is None:
        dx = z.guarded((B, C, H, W), name='dx')
    hipabi.check(L.straps_stem_dgrad(P(dyd), P(wp), P(dx), B, C, H, W, accumulate, None), 'stem dgrad')
    return dx


# ------------------------------------------------------------------------------------------------------------------------------------ forward

def _check_stats_exact(part, ref_nchw, shape, what):
    B, C, H, W = shape
    s1, s2, _, _ = S.stats_reference(_nhwc(ref_nchw).float(), B, H, W)
    p = part.cpu().double()
    assert bool(torch.equal(p[:, :, 0], s1)) and bool(torch.equal(p[:, :, 1], s2)), '%s: a statistics partial is not the exact integer' % what


def _check_stats_bound(part, y, shape, what):
    B, C, H, W = shape
    s1, s2, sa, n = S.stats_reference(y.cpu(), B, H, W)
    p = part.cpu()
    k = (n[:, None] + 8) * U
    _bounded(p[:, :, 0], s1, k * sa, 'stem_kernel statistics sum')
    _bounded(p[:, :, 1], s2, k * s2, 'stem_kernel statistics sumsq')


def _forward_case(dev, L, case):
    z = Zone(dev)
    shape = case.shape
    B, C, H, W = shape
    x, w = S.case_x(case), S.case_w(case)
    xd = z.at_end(x)
    assert W % 4 or xd.data_ptr() % 16 == 0
    wf = _pack_fwd(z, L, w)
    runs = [_fwd(z, L, xd, wf, m, shape) for m in _masks(z, L, xd, case)]
    z.check()
    y0, p0 = runs[0]
    nan_ok = case.arg == 'nan'
    for (y, p), how in zip(runs[1:], ('own mask', 'all-ones mask')):
        assert _same_bits(y0, y, nan_ok), '%s: y with the %s differs from the run without a mask' % (case.id, how)
        assert _same_bits(p0, p, nan_ok), '%s: the statistics partials with the %s differ' % (case.id, how)
    ref, sab = S.fwd_reference(x, w)
    got = y0.permute(0, 3, 1, 2).cpu()
    if case.arg == 'zero':
        assert _plus_zero(y0) and _plus_zero(p0), '%s: an all-zero input must give +0.0 everywhere' % case.id
    elif S.case_integer(case):
        assert bool(torch.equal(got.double(), ref)), '%s: %d outputs are not the exact integer' % (case.id, int((got.double() != ref).sum()))
        _check_stats_exact(p0, ref, shape, case.id)
    else:
        if case.arg == 'nan':
            hit = torch.from_numpy(S.window_contains(B, H, W, (S.nan_pixel(shape)[0],) + S.nan_pixel(shape)[2:]))
            assert bool(torch.equal(torch.isnan(got), hit[:, None].expand_as(got))), '%s: NaN outside / missing inside the 7 x 7 windows of the pixel' % case.id
        _bounded(got, ref, (49 * C + 16) * U * sab, 'stem_kernel raw', bar=2e-5 + 2e-5 * ref.abs())
        if case.arg != 'nan':
            _check_stats_bound(p0, y0, shape, case.id)


@pytest.mark.parametrize('shape', list(FWD), ids=[S.sid(s) for s in FWD])
def test_forward(dev, shape):
    """no mask / the kernel's own mask / an all-ones mask: bit-identical y and partials; integer cases exact; dense cases inside the derived bounds"""
    L = hipabi.lib()
    for case in FWD[shape]:
        _forward_case(dev, L, case)


@pytest.mark.parametrize('shape', S.FUSED_SHAPES, ids=[S.sid(s) for s in S.FUSED_SHAPES])
def test_forward_fused_epilogue(dev, shape):
    """scale + shift + ReLU, no statistics"""
    L = hipabi.lib()
    B, C, H, W = shape
    case = S.Case('dense-' + S.sid(shape), 'dense', shape, None)
    z = Zone(dev)
    x, w = S.case_x(case), S.case_w(case)
    sc, sh = S.det((64,), 3, 0.5, 1.5), S.det((64,), 4, -0.5, 0.5)
    sc[::7] *= -1
    xd, wf, scd, shd = z.at_end(x), _pack_fwd(z, L, w), z.at_end(sc), z.at_end(sh)
    ref, sab = S.fwd_reference(x, w)
    pre = ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    want = pre.clamp_min(0)
    bound = sc.double().abs()[None, :, None, None] * (49 * C + 16) * U * sab + U * want.abs()
    outs = []
    for m in _masks(z, L, xd, case):
        y, _ = _fwd(z, L, xd, wf, m, shape, stats=False, scale=scd, shift=shd, relu=1)
        outs.append(y)
        _bounded(y.permute(0, 3, 1, 2), want, bound, 'stem_kernel fused', bar=3e-5 + 3e-5 * want.abs())
    z.check()
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
    assert bool((outs[0] == 0).any()) and bool((outs[0] > 0).any())


# ------------------------------------------------------------------------------------------------------------------------------------ weight gradient

_WREF = {}


def _wgrad_ref(case):
    """float64 reference and sum_abs of a weight-gradient case, computed once per module"""
    if case.id not in _WREF:
        _WREF[case.id] = S.wgrad_reference(S.case_x(case), S.case_dy(case))
    return _WREF[case.id]


def _wgrad_case(dev, L, case):
    z = Zone(dev)
    shape = case.shape
    B, C, H, W = shape
    Ho, Wo = S.out_hw(H, W)
    x, dy = S.case_x(case), S.case_dy(case)
    xd, dyd = z.at_end(x), z.at_end(_nhwc(dy))
    masks = _masks(z, L, xd, case)
    runs = [_wgrad(z, L, xd, dyd, m, shape) for m in masks]
    dw0, ws0 = runs[0]
    nan_ok = case.arg == 'nan'
    for (dw, _), how in zip(runs[1:], ('own mask', 'all-ones mask')):
        assert _same_bits(dw0, dw, nan_ok), '%s: dw with the %s differs from the run without a mask' % (case.id, how)
    # the workspace of the run without a mask: [partials | the kernel's own non-zero map | activity bytes per (channel group, tile)]
    nf, nw, nt, _ = S.wgrad_workspace_layout(B, C, H, W)
    assert np.array_equal(_words(ws0[nf:nf + nw]), S.case_mask(case).reshape(-1)), '%s: the internally computed non-zero map' % case.id
    tact = ws0[nf + nw:].contiguous().view(torch.uint8)[:nt].cpu().numpy()
    assert np.array_equal(tact, S.tile_act_ref(S.case_mask(case), B, C, H, W).reshape(-1)), '%s: stem_tileact_kernel differs from tile_act_ref' % case.id
    # a second call into the same, not refilled workspace
    dw1, _ = _wgrad(z, L, xd, dyd, masks[1], shape, ws=runs[1][1])
    assert _same_bits(dw0, dw1, nan_ok), '%s: a second call into the same workspace gives other bits' % case.id
    # accumulate = 1 onto a prior
    prior = S.det((64, C, 7, 7), 91)
    acc = z.guarded((64, C, 7, 7), name='dw accumulate')
    acc.copy_(prior)
    _wgrad(z, L, xd, dyd, masks[1], shape, accumulate=1, dw=acc)
    z.check()
    assert _same_bits(acc.cpu(), prior + dw0.cpu(), nan_ok), '%s: accumulate = 1 is not prior + dw in fp32' % case.id
    ref, sab = _wgrad_ref(case)
    if case.arg == 'zero':
        assert _plus_zero(dw0) and _same_bits(acc.cpu(), prior), '%s: an all-zero input must give +0.0 and leave an accumulated prior alone' % case.id
    elif S.case_integer(case):
        assert bool(torch.equal(dw0.cpu().double(), ref)), '%s: %d weight gradients are not the exact integer' % (case.id, int((dw0.cpu().double() != ref).sum()))
    else:
        got = dw0.cpu().double()
        if case.arg == 'nan':
            # every tap the reference makes NaN is NaN, and no OTHER channel is touched.  Inside the NaN pixel's own channel the kernel may have more NaN
            # taps than the reference: a ragged tile contracts its out-of-range pixels with dy = 0, and 0 x NaN is NaN (a finite input never shows this)
            extra = torch.isnan(got) & ~torch.isnan(ref)
            c = S.nan_pixel(shape)[1]
            assert bool(torch.isnan(got)[torch.isnan(ref)].all()) and not bool(extra[:, :c].any()) and not bool(extra[:, c + 1:].any()), case.id
            got[extra] = ref[extra]
        fin = ref[~torch.isnan(ref)]
        _bounded(got, ref, (B * Ho * Wo + 16) * U * sab, 'stem_wgrad_kernel', bar=2e-5 * float(fin.abs().max()))


@pytest.mark.parametrize('shape', list(WGRAD), ids=[S.sid(s) for s in WGRAD])
def test_weight_gradient(dev, shape):
    """mask absent / own / all ones: bit-identical dw; integer cases exact; accumulate; NaN-filled workspace of exactly the advertised size; the
    internal non-zero map and the per-group tile activity against their references"""
    L = hipabi.lib()
    for case in WGRAD[shape]:
        _wgrad_case(dev, L, case)


# ------------------------------------------------------------------------------------------------------------------------------------ data gradient

DGRAD = OrderedDict()
for _c in S.dgrad_cases():
    DGRAD.setdefault(_c[0], []).append(_c)


@pytest.mark.parametrize('cin', list(DGRAD), ids=['cin%d' % c for c in DGRAD])
def test_data_gradient(dev, cin):
    """every channel count (stem_dgrad_kernel<1 .. 5>, with and without a preceding full-chunk launch): tracer weights and gradients exact, dense ones
    inside the bound, accumulate = 1 equal to prior + dx in fp32"""
    L = hipabi.lib()
    for (_, B, H, W) in DGRAD[cin]:
        shape = (B, cin, H, W)
        Ho, Wo = S.out_hw(H, W)
        for family in ('tracer', 'dense'):
            z = Zone(dev)
            w = S.tracer_w(cin) if family == 'tracer' else S.dense_w(cin, 12)
            dy = S.tracer_dy(B, Ho, Wo) if family == 'tracer' else S.det((B, 64, Ho, Wo), 13)
            wp, dyd = _pack_dgrad(z, L, w), z.at_end(_nhwc(dy))
            dx = _dgrad(z, L, dyd, wp, shape)
            prior = S.det(shape, 92)
            acc = z.guarded(shape, name='dx accumulate')
            acc.copy_(prior)
            _dgrad(z, L, dyd, wp, shape, accumulate=1, dx=acc)
            z.check()
            what = 'dgrad %s %s' % (family, S.sid(shape))
            assert _same_bits(acc.cpu(), prior + dx.cpu()), '%s: accumulate = 1 is not prior + dx in fp32' % what
            ref, sab = S.dgrad_reference(dy, w, H, W)
            if family == 'tracer':
                assert bool(torch.equal(dx.cpu().double(), ref)), '%s: %d input gradients are not the exact integer' % (what, int((dx.cpu().double() != ref).sum()))
            else:
                _bounded(dx, ref, (1024 + 16) * U * sab, 'stem_dgrad_kernel', bar=1e-5 * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------------------ proxy builders

def _proxy_inputs(B, NJ, WH, std):
    """the joints of test_build_proxy_input_with_nonzero_map_equals_the_two_passes: inside, on every border, in the corners, outside, negative"""
    j = torch.from_numpy(det_uniform((B, NJ, 2), 41, -12.0, WH + 12.0))
    edge = [(0.0, 0.0), (WH - 1.0, WH - 1.0), (0.4, WH - 0.6), (WH - 1.0, 3.0), (-0.9, 17.2), (WH + 7.9, 40.0), (2 * std - 1.0, 2 * std + 0.0), (-2.0 * std, 50.0),
            (WH - 2.0 * std, WH / 2.0), (WH + 2.0 * std - 1.0, 9.0)]
    for k, (ex, ey) in enumerate(edge):
        j[k % B, k % NJ] = torch.tensor([ex, ey])
    seg = (torch.from_numpy(det_uniform((B, WH, WH), 42, 0.0, 1.0)) > 0.9).float() * torch.from_numpy(np.floor(det_uniform((B, WH, WH), 43, 1.0, 6.999)))
    seg[:, : WH // 2, : WH // 3] = 0.0
    return seg, j


@pytest.mark.parametrize('wh', S.PROXY_STD_WH)
def test_proxy_builders_against_the_oracle(dev, wh):
    """straps_build_proxy_input_std (and _nz where wh % 8 == 0) against O.multiclass_to_binary / O.joints2d_to_heatmaps(j, wh, std): the non-zero
    pattern exact, values at the golden test's bar, the map equal to nzmask_ref of the oracle's planes; outputs guarded"""
    L = hipabi.lib()
    B, NJ = 2, 7
    for std in S.proxy_stds(wh):
        seg, j = _proxy_inputs(B, NJ, wh, std)
        want = torch.cat([O.multiclass_to_binary(seg).unsqueeze(1), O.joints2d_to_heatmaps(j, wh, std)], dim=1)
        assert int((want[:, 1:] != 0).sum()) > 0
        z = Zone(dev)
        segd, jd = z.at_end(seg), z.at_end(j)
        outs = []
        out = z.guarded((B, NJ + 1, wh, wh), name='proxy planes')
        hipabi.check(L.straps_build_proxy_input_std(P(segd), P(jd), P(out), B, NJ, wh, std, None), 'build_proxy_input_std')
        outs.append(out)
        if wh in S.PROXY_NZ_WH:
            out2 = z.guarded((B, NJ + 1, wh, wh), name='proxy planes (nz)')
            m = z.guarded((L.straps_stem_nzmask_words(B, NJ + 1, wh, wh),), torch.int32, fill=WORD_FILL, name='proxy nzmask')
            hipabi.check(L.straps_build_proxy_input_nz(P(segd), P(jd), P(out2), P(m), B, NJ, wh, std, None), 'build_proxy_input_nz')
            outs.append(out2)
            assert np.array_equal(_words(m), S.nzmask_ref(want).reshape(-1)), 'wh %d std %d: the map differs from nzmask_ref of the oracle planes' % (wh, std)
        z.check()
        for o in outs:
            got = o.cpu()
            assert bool(torch.isfinite(got).all())
            assert bool(torch.equal(got != 0, want != 0)), 'wh %d std %d: non-zero pattern differs in %d pixels' % (wh, std, int(((got != 0) != (want != 0)).sum()))
            assert bool(torch.equal(got[:, 0], want[:, 0]))
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-6, atol=1e-7)
        if len(outs) == 2:
            assert _same_bits(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------------------------ determinism

def test_three_launches_give_identical_bits(dev):
    L = hipabi.lib()
    shape = S.DETERMINISM_SHAPE
    B, C, H, W = shape
    case = S.Case('dense-' + S.sid(shape), 'dense', shape, None)
    z = Zone(dev)
    x, w, dy = S.case_x(case), S.case_w(case), S.case_dy(case)
    xd, dyd, wf, wp = z.at_end(x), z.at_end(_nhwc(dy)), _pack_fwd(z, L, w), _pack_dgrad(z, L, w)
    f = [_fwd(z, L, xd, wf, None, shape) for _ in range(3)]
    g = [_wgrad(z, L, xd, dyd, None, shape)[0] for _ in range(3)]
    d = [_dgrad(z, L, dyd, wp, shape) for _ in range(3)]
    z.check()
    for k in (1, 2):
        assert _same_bits(f[0][0], f[k][0]) and _same_bits(f[0][1], f[k][1]) and _same_bits(g[0], g[k]) and _same_bits(d[0], d[k])
