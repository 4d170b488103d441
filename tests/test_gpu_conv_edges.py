"""GPU: every convolution kernel at its tile edges, behind redzones (tests/redzone.py) -- the cases of tests/conv_cases.py, which also states which
kernel instantiation each case reaches (tests/test_conv_cases_cpu.py holds that statement to the library).

Common form of every case:
  * every output, statistics / BatchNorm partial buffer and split-K workspace comes from Zone.guarded: NaN-filled, exactly the advertised size,
    sentinel margins on both sides (a write outside it, or a partial the reduction reads and no workgroup wrote, shows);
  * every fp32 operand comes from Zone.at_end (NaN directly behind its last element); every plane operand is re-homed by Zone.planes with a gap of
    bf16 NaNs behind EVERY plane (split3 gives ps == n: a read past plane 0 would land in plane 1) -- a used over-read is a NaN in the result;
  * the reference is the float64 F.conv2d / autograd evaluation on the CPU; det_uniform data with the scalings of the existing tests.

After each call: (a) the result is finite and within the existing bar of its entry point (quoted where used), (b) where a twin exists -- a lean epilogue
against the same tile with the shared epilogue, the fp32-operand route against the plane route at the twin tile, the _bits forms against the fp32-mask
forms -- bit equality, (c) zone.check().
"""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as K
import straps_amd  # noqa: F401
from detgen import det_uniform
from redzone import Zone
from straps_amd import hipabi
from straps_amd.encoder_exec import split3, weight_planes

pytestmark = pytest.mark.gpu
P = hipabi.ptr


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    lib = hipabi.load()
    # the PRODUCT library: the halo twins pass tile_cfg bit 6, which a tools build (-DSTRAPS_TOOLS) reads as an ablation kernel -- wrong results by design
    import os
    assert os.path.abspath(lib._name) == os.path.abspath(hipabi.LIB_PATH), 'these tests compare bit for bit on the product library, not %s' % lib._name
    return torch.device('cuda:0')


_PERIOD = (1 << 19) + 17          # (odd against every channel count and row length of the tables)


def _det(shape, seed, lo=-1.0, hi=1.0):
    """det_uniform data as a CPU tensor; beyond 2^19 elements one det_uniform block repeated (the generator makes ten million values a second, the
    large automatic-rule cases hold a few hundred million)"""
    n = 1
    for d in shape:
        n *= d
    if n <= _PERIOD:
        return torch.from_numpy(det_uniform(tuple(shape), seed, lo, hi))
    blk = torch.from_numpy(det_uniform((_PERIOD,), seed, lo, hi))
    return blk.repeat(-(-n // _PERIOD))[:n].view(tuple(shape)).contiguous()


def _nhwc(t):
    return t.float().permute(0, 2, 3, 1).contiguous()


def _act_planes(z, t_nhwc):
    """CPU fp32 NHWC tensor -> (chunk-major planes with NaN gaps, plane stride, the fp32 tensor on the device at the end of poison)"""
    td = z.at_end(t_nhwc)
    pl, _ = split3(hipabi.lib(), td)
    out, ps = z.planes(pl, td.numel())
    return out, ps, td


def _w_planes(z, w, dgrad=False):
    pl, _ = weight_planes(hipabi.lib(), w.float().contiguous().to(z.device), dgrad)
    return z.planes(pl, w.numel())


def _bits(y):
    """[..., C] activation -> int32 words [rows][C / 32], bit (c & 31) = (y > 0)  (what straps_bn_apply_bits_x3 writes)"""
    C = y.shape[-1]
    b = (y.reshape(-1, C // 32, 32) > 0).to(torch.int64)
    wd = (b << torch.arange(32, dtype=torch.int64, device=y.device)).sum(-1)
    return torch.where(wd >= 2 ** 31, wd - 2 ** 32, wd).to(torch.int32).contiguous()


def _weights(cout, cin, k, seed):
    return _det((cout, cin, k, k), seed) * (2.0 / (cin * k * k)) ** 0.5


def _assert_fwd_bar(got, ref, what, a=2e-5, r=2e-5):
    """the forward bar of tests/test_gpu_conv_x3.py::test_conv_fwd_x3_vs_float64: |err| <= 2e-5 + 2e-5 |ref| element-wise"""
    assert bool(torch.isfinite(got).all()), '%s: not finite' % what
    err = (got.double() - ref).abs()
    worst = float((err - (a + r * ref.abs())).max())
    print('%s: max abs err %.3e' % (what, float(err.max())))
    assert worst <= 0, '%s: max abs err %.3e' % (what, float(err.max()))


def _assert_stats(part, ref_nhwc, what):
    """statistics partials, summed over the M tiles: rtol 1e-4 / atol 1e-3 (test_conv_fwd_x3_vs_float64)"""
    assert bool(torch.isfinite(part).all()), '%s: statistics partials not finite (a partial block nobody wrote?)' % what
    s = part.double().sum(0)
    r2 = ref_nhwc.reshape(-1, ref_nhwc.shape[-1])
    torch.testing.assert_close(s[:, 0], r2.sum(0), rtol=1e-4, atol=1e-3, msg=lambda m: '%s sum: %s' % (what, m))
    torch.testing.assert_close(s[:, 1], (r2 * r2).sum(0), rtol=1e-4, atol=1e-3, msg=lambda m: '%s sum of squares: %s' % (what, m))


def _assert_grad_bar(got, ref, what, bar=2e-5):
    """the gradient bar of test_conv_dgrad_x3_vs_float64 / test_conv_wgrad_x3_vs_float64: 2e-5 of the maximum (4e-5 after an accumulate call)"""
    assert bool(torch.isfinite(got).all()), '%s: not finite' % what
    err = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print('%s: relative-to-max error %.3e' % (what, err))
    assert err < bar, '%s: relative-to-max error %.3e' % (what, err)


# ----------------------------------------------------------------------------------------------------------------------------------------
# forward on the planes

def _call_fwd(z, c, cfg, x3, xps, w3, wps, sc=None, sh=None, res=None, relu=0, stats=False, tag=''):
    L = hipabi.lib()
    B, H, W, ci, co, k, s, _ = c
    pad = K.pad_of(k)
    Ho, Wo = K.out_hw(H, W, k, s, pad)
    y = z.guarded((B, Ho, Wo, co), name='y' + tag)
    part = None
    if stats:
        nb = L.straps_conv_x3_stat_blocks(B, H, W, ci, co, k, k, s, pad, cfg)
        assert nb == K.x3_route(K.fwd_problem(B, H, W, ci, co, k, s, pad), cfg, {'y', 'stats'})[2]
        part = z.guarded((nb, co, 2), name='stats' + tag)
    hipabi.check(L.straps_conv_fwd_x3(P(x3), xps, P(w3), wps, P(sc), P(sh), P(res), int(relu), P(y), P(part), B, H, W, ci, co, k, k, s, pad, cfg, None),
                 'conv_fwd_x3' + tag)
    z.check()
    return y, part


@pytest.mark.parametrize('c', K.FWD_EXPLICIT + K.FWD_AUTO, ids=K.conv_case_id)
def test_conv_fwd_x3_at_tile_edges(dev, c):
    """straps_conv_fwd_x3, raw + statistics and the fused scale / shift / residual / ReLU epilogue: every explicit tile at M = BM + 1, 2 BM - 1 and
    below BM / 2 with one and two K chunks, H = 1 and W = 1 maps, stride 2; the automatic rule's size classes one row short of and past a tile
    multiple (lean forward epilogue) and the halo kernels -- a lean launch against the same tile with the shared epilogue bit for bit."""
    B, H, W, ci, co, k, s, cfg = c
    pad = K.pad_of(k)
    p = K.fwd_problem(B, H, W, ci, co, k, s, pad)
    x = _det((B, ci, H, W), 1)
    w = _weights(co, ci, k, 2)
    ref = F.conv2d(x.double(), w.double(), None, s, pad).permute(0, 2, 3, 1).contiguous().to(dev)
    z = Zone(dev)
    x3, xps, _ = _act_planes(z, _nhwc(x))
    w3, wps = _w_planes(z, w)
    y, part = _call_fwd(z, c, cfg, x3, xps, w3, wps, stats=True)
    _assert_fwd_bar(y, ref, 'raw')
    _assert_stats(part, ref, 'statistics')
    inst = K.x3_route(p, cfg, K.fwd_ops('raw_stats'))[0]
    if inst[2]:          # a lean form: the same tile / halo kernel with the shared epilogue
        tw = K.twin_cfg(p, cfg, K.fwd_ops('raw_stats'))
        y2, part2 = _call_fwd(z, c, tw, x3, xps, w3, wps, stats=True, tag=' (twin)')
        assert torch.equal(y, y2) and torch.equal(part, part2), 'lean forward epilogue differs from the shared epilogue on the same tile'
    sc = z.at_end(_det((co,), 3, 0.5, 1.5))
    sh = z.at_end(_det((co,), 4, -0.5, 0.5))
    res = z.at_end(_det(tuple(ref.shape), 5))
    want = F.relu(ref * sc.double() + sh.double() + res.double())
    y3, _ = _call_fwd(z, c, cfg, x3, xps, w3, wps, sc=sc, sh=sh, res=res, relu=1, tag=' (fused)')
    _assert_fwd_bar(y3, want, 'fused epilogue')


@pytest.mark.parametrize('c', K.FWD_PLANES, ids=K.conv_case_id)
@pytest.mark.parametrize('with_y', [True, False], ids=['y', 'y_null'])
def test_conv_fwd_x3p_plane_output_with_a_guarded_gap(dev, c, with_y):
    """straps_conv_fwd_x3p: y_plane_stride larger than the extent, the gap behind every plane guarded; ragged M on the 64x64 and a 128-wide tile; the
    planes equal a split pass over the fp32 result bit for bit (tests/test_gpu_conv_x3.py), y both given and NULL."""
    L = hipabi.lib()
    B, H, W, ci, co, k, s, cfg = c
    pad = K.pad_of(k)
    Ho, Wo = K.out_hw(H, W, k, s, pad)
    x = _det((B, ci, H, W), 1)
    w = _weights(co, ci, k, 2)
    ref = F.conv2d(x.double(), w.double(), None, s, pad).permute(0, 2, 3, 1).contiguous().to(dev)
    z = Zone(dev)
    x3, xps, _ = _act_planes(z, _nhwc(x))
    w3, wps = _w_planes(z, w)
    sc = z.at_end(_det((co,), 3, 0.5, 1.5))
    sh = z.at_end(_det((co,), 4, -0.5, 0.5))
    res = z.at_end(_det(tuple(ref.shape), 5))
    want = F.relu(ref * sc.double() + sh.double() + res.double())
    n = B * Ho * Wo * co
    y = z.guarded((B, Ho, Wo, co), name='y') if with_y else None
    yp, yps = z.guarded_planes(n, name='y_planes')
    assert yps > n
    hipabi.check(L.straps_conv_fwd_x3p(P(x3), xps, P(w3), wps, P(sc), P(sh), P(res), 1, P(y), P(yp), yps, B, H, W, ci, co, k, k, s, pad, cfg, None), 'conv_fwd_x3p')
    z.check()
    # the planes' sum is the fp32 result exactly (three bf16 parts of 8 significant bits each)
    got = (yp[:, :n].to(torch.int32) << 16).view(torch.float32).double().sum(0)
    cm = got.view(co // 32, B * Ho * Wo, 32).permute(1, 0, 2).reshape(B, Ho, Wo, co)      # chunk-major -> NHWC (csrc/common.h cm_index)
    _assert_fwd_bar(cm.float(), want, 'plane output')
    if with_y:
        _assert_fwd_bar(y, want, 'y')
        want_pl, _ = split3(L, y)
        assert torch.equal(yp[:, :n], want_pl[:, :n]), 'the plane output is not the split of y'


# ----------------------------------------------------------------------------------------------------------------------------------------
# data gradient on the planes

class _Dgrad:
    """operands of one data-gradient case on the device, and the float64 reference"""

    def __init__(self, dev, z, c):
        self.c, self.z = c, z
        B, H, W, ci, co, k, s, cfg = c
        pad = K.pad_of(k)
        Ho, Wo = K.out_hw(H, W, k, s, pad)
        self.p = K.dgrad_problem(B, H, W, ci, co, k, s, pad)
        w = _weights(co, ci, k, 2)
        dy = _det((B, co, Ho, Wo), 3) * 1e-3          # gradient-sized values
        xx = torch.zeros(B, ci, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, w.double(), None, s, pad).backward(dy.double())
        self.grad = xx.grad.permute(0, 2, 3, 1).contiguous().to(dev)
        self.g3, self.gps, self.dyd = _act_planes(z, _nhwc(dy))
        self.w3, self.wps = _w_planes(z, w, dgrad=True)
        shape = (B, H, W, ci)
        self.add = z.at_end(_det(shape, 4) * 1e-3)                                     # unmasked gradient of the later unit's output ...
        y_next = _det(shape, 9).to(dev)                                                # ... and that unit's activation (its sign masks the addend)
        self.dz = z.at_end(torch.where(y_next > 0, self.add, torch.zeros_like(self.add)))
        self.abits = z.at_end(_bits(y_next))
        self.raw = z.at_end(_det(shape, 5, -2, 2))
        self.msc, self.msh = z.at_end(_det((ci,), 6, 0.5, 1.5)), z.at_end(_det((ci,), 7, -0.5, 0.5))
        self.out = z.at_end(torch.relu(self.raw * self.msc + self.msh + _det(shape, 8).to(dev)))      # a residual unit's output
        self.obits = z.at_end(_bits(self.out))
        self.mean = z.at_end(self.raw.mean(dim=(0, 1, 2)))
        self.invstd = z.at_end((self.raw.var(dim=(0, 1, 2), unbiased=False) + 1e-5).rsqrt())
        self.shape = shape

    def run(self, form, cfg, tag=''):
        """one call of the entry point the form names -> (dx, partials or None); outputs guarded, the zone checked"""
        L, z = hipabi.lib(), self.z
        B, H, W, ci, co, k, s, _ = self.c
        geo = (B, H, W, ci, co, k, k, s, K.pad_of(k), cfg)
        dx = z.guarded(self.shape, name='dx %s%s' % (form, tag))
        head = (P(self.g3), self.gps, P(self.w3), self.wps)
        part = None
        if form.startswith('bn'):
            nb = L.straps_conv_dgrad_x3_bn_blocks(*geo)
            assert nb == K.x3_route(self.p, cfg, K.DGRAD_FORMS[form])[2] > 0
            part = z.guarded((nb, ci, 2), torch.float64, name='bn partials %s%s' % (form, tag))
            bn = (P(self.raw), P(self.mean), P(self.invstd), P(part))
        if form == 'plain':
            rc = L.straps_conv_dgrad_x3(*head, None, P(dx), *geo, None)
        elif form == 'addend':
            rc = L.straps_conv_dgrad_x3(*head, P(self.dz), P(dx), *geo, None)
        elif form == 'bits':
            rc = L.straps_conv_dgrad_x3_bits(*head, P(self.add), P(dx), *geo, P(self.abits), None)
        elif form == 'bn_out':          # fp32 masks: the activation itself, the masked addend
            rc = L.straps_conv_dgrad_x3_bn(*head, P(self.dz), P(dx), *geo, bn[0], P(self.out), None, None, *bn[1:], None)
        elif form == 'bn_mask':         # the mask re-derived from raw
            rc = L.straps_conv_dgrad_x3_bn(*head, P(self.dz), P(dx), *geo, bn[0], None, P(self.msc), P(self.msh), *bn[1:], None)
        elif form == 'bn_bits':         # both masks as bits
            rc = L.straps_conv_dgrad_x3_bn_bits(*head, P(self.add), P(dx), *geo, bn[0], None, None, None, *bn[1:], P(self.abits), P(self.obits), None)
        else:
            assert form == 'bn_noadd'
            rc = L.straps_conv_dgrad_x3_bn_bits(*head, None, P(dx), *geo, bn[0], None, None, None, *bn[1:], None, P(self.obits), None)
        hipabi.check(rc, 'dgrad %s%s' % (form, tag))
        z.check()
        return dx, part

    def check_sums(self, dx, part, mask, what):
        """the bar of test_dgrad_x3_with_fused_batchnorm_sums: |S - S_float64| <= 1e-9 x scale, on the kernel's own dx"""
        assert bool(torch.isfinite(part).all()), '%s: BatchNorm partials not finite' % what
        gd = torch.where(mask, dx, torch.zeros_like(dx)).double()
        dev_ = self.raw.double() - self.mean.double()
        s1 = gd.sum(dim=(0, 1, 2))
        s2 = (gd * dev_).sum(dim=(0, 1, 2)) * self.invstd.double()
        got = part.sum(0)
        scale1 = float(gd.abs().sum(dim=(0, 1, 2)).max())
        scale2 = float((gd * dev_).abs().sum(dim=(0, 1, 2)).max() * self.invstd.max())
        assert float((got[:, 0] - s1).abs().max()) <= 1e-9 * scale1 + 1e-30, '%s S1' % what
        assert float((got[:, 1] - s2).abs().max()) <= 1e-9 * scale2 + 1e-30, '%s S2' % what


def _dgrad_case(dev, c):
    """the forms of K.dgrad_run(c), in its order (K.reached() counts from the same list); a lean launch flagged there runs again under K.twin_cfg"""
    B, H, W, ci, co, k, s, cfg = c
    z = Zone(dev)
    d = _Dgrad(dev, z, c)
    got = {}
    for form, with_twin in K.dgrad_run(c):
        dx, part = got[form] = d.run(form, cfg)
        if form == 'plain':          # no addend: the gradient itself; the dead positions of a 1x1 / stride-2 filter must read exactly +0.0
            _assert_grad_bar(dx, d.grad, form)
            if k == 1 and s == 2:
                live = torch.zeros(d.shape, dtype=torch.bool, device=dev)
                live[:, ::2, ::2] = True
                assert bool((dx[~live] == 0).all()) and not bool(torch.signbit(dx[~live]).any()), 'dead positions of a 1x1 / stride-2 gradient must be +0.0'
        elif form == 'addend':       # a (masked) addend as an fp32 tensor
            _assert_grad_bar(dx, d.grad + d.dz.double(), form)
        elif form == 'bn_noadd':
            assert torch.equal(dx, got['plain'][0])
        else:                        # every other form writes the dx of the addend form, bit for bit (bits against fp32 masks)
            assert torch.equal(dx, got['addend'][0]), '%s writes another dx than straps_conv_dgrad_x3 with the masked addend' % form
        # fused BatchNorm sums under the three mask sources; the bit form equals the fp32-mask form bit for bit
        if form in ('bn_out', 'bn_bits', 'bn_noadd'):
            d.check_sums(dx, part, d.out > 0, form)
        if form == 'bn_bits':
            assert torch.equal(part, got['bn_out'][1]), 'straps_conv_dgrad_x3_bn_bits: partials differ from the fp32-mask form'
        if form == 'bn_mask':
            # (the mask as the kernel forms it: fma(raw, scale, shift) > 0, evaluated in float64 and rounded once -- no value of this data within half an ulp of a tie)
            d.check_sums(dx, part, (d.raw.double() * d.msc.double() + d.msh.double()).float() > 0, form)
        if with_twin and K.x3_route(d.p, cfg, K.DGRAD_FORMS[form])[0][2]:          # a lean form: the same tile / halo kernel with the shared epilogue
            dx2, part2 = d.run(form, K.twin_cfg(d.p, cfg, K.DGRAD_FORMS[form]), ' (twin)')
            assert torch.equal(dx, dx2), '%s: the lean epilogue differs from the shared epilogue on the same tile' % form
            assert part is None or torch.equal(part, part2), '%s: BatchNorm partials of the lean epilogue differ from the shared epilogue\'s' % form


@pytest.mark.parametrize('c', K.DGRAD_EXPLICIT + K.DGRAD_S2_SMALL, ids=K.conv_case_id)
def test_conv_dgrad_x3_at_tile_edges(dev, c):
    """straps_conv_dgrad_x3, _bits, _bn, _bn_bits: every explicit tile at the forward's edge rows with the reduction on 32 and 64 output channels, stride 2;
    stride-2 gradients at 1x1 ... 2x5 maps (one, two and four parity classes, dead classes of a 1x1 filter, with and without an addend)."""
    _dgrad_case(dev, c)


@pytest.mark.parametrize('c', K.DGRAD_AUTO, ids=K.conv_case_id)
def test_conv_dgrad_x3_automatic_rule_and_lean_epilogue(dev, c):
    """the automatic rule's size classes as gradients (tiles 7, 5, 12, 11, 3, both lean halo kernels; the stride-2 classes with a ragged class each): the
    lean data-gradient epilogue with an addend, ReLU bits and the fused BatchNorm sums under both of its mask sources, against float64 and against the
    shared epilogue on the same tile bit for bit."""
    _dgrad_case(dev, c)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the fp32-operand route

X3F_TWINS = {1: 2, 2: 3}          # x3f tile -> the plane route's tile of the same shape and loop form (tests/test_gpu_conv_x3f.py)


def _call_fwd_x3f(z, c, x, w3, wps, a_sc=None, a_sh=None, a_relu=0, sc=None, sh=None, res=None, relu=0, stats=False, tag=''):
    L = hipabi.lib()
    B, H, W, ci, co, s, cfg = c
    Ho, Wo = K.out_hw(H, W, 1, s, 0)
    y = z.guarded((B, Ho, Wo, co), name='y' + tag)
    part = None
    if stats:
        nb = L.straps_conv_x3f_stat_blocks(B, H, W, ci, co, 1, 1, s, 0, cfg)
        assert nb == K.x3f_stat_blocks(B, H, W, ci, co, 1, s, 0, cfg) > 0
        part = z.guarded((nb, co, 2), name='stats' + tag)
    hipabi.check(L.straps_conv_fwd_x3f(P(x), P(a_sc), P(a_sh), int(a_relu), P(w3), wps, P(sc), P(sh), P(res), int(relu), P(y), P(part), B, H, W, ci, co, 1, 1, s, 0,
                                       cfg, None), 'conv_fwd_x3f' + tag)
    z.check()
    return y, part


@pytest.mark.parametrize('c', K.X3F_FWD, ids=K.x3f_case_id)
def test_conv_fwd_x3f_at_tile_edges(dev, c):
    """straps_conv_fwd_x3f at tiles 0, 1, 2 and 5 with a 64-channel reduction: M = BM +- 1, stride 2 on odd maps, the streaming kernel with fewer tiles
    than workgroups and with one tile more than a multiple of its grid (resident-weight and ring forms).  Every form of K.X3F_FWD_FORMS: raw + statistics
    and the eval epilogue, each without and with the producer's BatchNorm + ReLU in the operand path.  Bars of tests/test_gpu_conv_x3f.py: 2e-5 + 2e-5 |ref|
    against float64 for the raw form, 4e-5 + 2e-5 |ref| behind the operand-path BatchNorm (its fp32 fmaf adds a rounding) and for the eval epilogue; every
    form bit-equal to the plane route with the same epilogue at the twin tile -- on split planes of x, or on the planes straps_bn_apply_x3 writes."""
    L = hipabi.lib()
    B, H, W, ci, co, s, cfg = c
    p = K.fwd_problem(B, H, W, ci, co, 1, s, 0)
    x = _det((B, ci, H, W), 1201)
    w = _weights(co, ci, 1, 1202)
    z = Zone(dev)
    xd = z.at_end(_nhwc(x))
    w3, wps = _w_planes(z, w)
    a_sc, a_sh = z.at_end(_det((ci,), 1303, 0.5, 1.5)), z.at_end(_det((ci,), 1304, -0.5, 0.5))
    sc, sh = z.at_end(_det((co,), 1403, 0.5, 1.5)), z.at_end(_det((co,), 1404, -0.5, 0.5))
    Ho, Wo = K.out_hw(H, W, 1, s, 0)
    res = z.at_end(_det((B, Ho, Wo, co), 1405))
    act = (x.double() * a_sc.cpu().double().view(1, -1, 1, 1) + a_sh.cpu().double().view(1, -1, 1, 1)).clamp_min(0)
    refs = {False: F.conv2d(x.double(), w.double(), stride=s).permute(0, 2, 3, 1).contiguous().to(dev),
            True: F.conv2d(act, w.double(), stride=s).permute(0, 2, 3, 1).contiguous().to(dev)}
    # the plane route's operands: the split of x; the planes an apply pass writes
    rows = B * H * W
    aps = (rows * ci + 7) // 8 * 8
    apl = torch.empty(3, aps, device=dev, dtype=torch.int16)
    hipabi.check(L.straps_bn_apply_x3(P(xd), P(a_sc), P(a_sh), None, 1, None, P(apl), aps, rows, ci, None), 'bn_apply_x3')
    planes = {False: _act_planes(z, _nhwc(x))[:2], True: z.planes(apl, rows * ci)}
    for form, ops in K.X3F_FWD_FORMS.items():
        abn, ev, stats = 'a_scale' in ops, 'scale' in ops, 'stats' in ops
        epi = dict(sc=sc, sh=sh, res=res, relu=1) if ev else {}
        y, part = _call_fwd_x3f(z, c, xd, w3, wps, a_sc=a_sc if abn else None, a_sh=a_sh if abn else None, a_relu=int(abn), stats=stats, tag=' ' + form, **epi)
        want = F.relu(refs[abn] * sc.double() + sh.double() + res.double()) if ev else refs[abn]
        _assert_fwd_bar(y, want, form, a=4e-5 if (abn or ev) else 2e-5)
        if stats:
            _assert_stats(part, refs[abn], form + ' statistics')
        inst = K.x3f_route(p, cfg, ops)[0]
        tw = X3F_TWINS[inst[1]] if inst[0] == 'x3f' else 0
        x3, xps = planes[abn]
        yp, pp = _call_fwd(z, (B, H, W, ci, co, 1, s, tw), tw, x3, xps, w3, wps, stats=stats, tag=' %s (plane route)' % form, **epi)
        assert torch.equal(y, yp), '%s differs from the plane route' % form
        if stats and inst[0] == 'x3f':
            assert torch.equal(part, pp), '%s: statistics partials differ from the plane route at the twin tile' % form


@pytest.mark.parametrize('c', K.X3F_DGRAD, ids=K.x3f_case_id)
def test_conv_dgrad_x3f_at_tile_edges(dev, c):
    """straps_conv_dgrad_x3f, plain and with every optional operand (addend masked by bits, fused BatchNorm sums masked by bits), at the forward's shapes.
    Bars of test_conv_dgrad_x3f_vs_float64_and_the_plane_route: 2e-5 of the maximum; sums 1e-5 / 1e-4 of their scale; dx bit-equal to the plane route at
    the twin tile, partials bit-equal at stride 2 (shared epilogue); else (the lean form pre-sums 16 values in fp32) within 2e-6 of the sum of their terms' magnitudes -- a NEW
    bar, derived below from the fp32 format, not the existing test's 1e-6 of max(sum |partials|, 1), which is an absolute 1e-6 on this gradient-sized data."""
    L = hipabi.lib()
    B, H, W, ci, co, s, cfg = c
    z = Zone(dev)
    d = _Dgrad(dev, z, (B, H, W, ci, co, 1, s, cfg))
    w3, wps = d.w3, d.wps
    geo = (B, H, W, ci, co, 1, 1, s, 0, cfg)

    def run(full, tag):
        dx = z.guarded(d.shape, name='dx' + tag)
        part = None
        if full:
            nb = L.straps_conv_dgrad_x3f_bn_blocks(*geo)
            assert nb == K.dgrad_x3f_bn_blocks(B, H, W, ci, co, 1, s, 0, cfg) > 0
            part = z.guarded((nb, ci, 2), torch.float64, name='bn partials' + tag)
            rc = L.straps_conv_dgrad_x3f(P(d.dyd), P(w3), wps, P(d.add), P(d.abits), P(dx), *geo, P(d.raw), P(d.obits), None, None, P(d.mean), P(d.invstd), P(part), None)
        else:
            rc = L.straps_conv_dgrad_x3f(P(d.dyd), P(w3), wps, None, None, P(dx), *geo, None, None, None, None, None, None, None, None)
        hipabi.check(rc, 'conv_dgrad_x3f' + tag)
        z.check()
        return dx, part

    res_ = {form: run(form == 'full', ' ' + form) for form in K.X3F_DGRAD_FORMS}          # (the list K.reached() counts from)
    dx0, _ = res_['plain']
    _assert_grad_bar(dx0, d.grad, 'plain')
    if s == 2:
        live = torch.zeros(d.shape, dtype=torch.bool, device=dev)
        live[:, ::2, ::2] = True
        assert bool((dx0[~live] == 0).all()), 'dead positions of a 1x1 / stride-2 gradient must be 0.0'
    dx, part = res_['full']
    want = d.grad + d.dz.double()
    _assert_grad_bar(dx, want, 'addend + bits')
    assert bool(torch.isfinite(part).all())
    g = want * (d.out > 0)
    dev_ = d.raw.double() - d.mean.double()
    s1, s2 = g.sum(dim=(0, 1, 2)), (g * dev_).sum(dim=(0, 1, 2)) * d.invstd.double()
    ps_ = part.sum(0)
    scale = g.abs().sum(dim=(0, 1, 2)).clamp_min(1e-30)
    assert bool(((ps_[:, 0] - s1).abs() <= 1e-5 * scale).all()) and bool(((ps_[:, 1] - s2).abs() <= 1e-4 * scale).all())
    inst = K.x3f_route(d.p, cfg, {'y', 'res', 'res_bits', 'bnr_raw'})[0]
    tw = X3F_TWINS.get(inst[1], 0) if inst[0] == 'x3f' else 0
    d.c = (B, H, W, ci, co, 1, s, tw)
    dxp, pp = d.run('bn_bits', tw, ' (plane route)')
    assert torch.equal(dx, dxp), 'dx differs from the plane route'
    if inst[0] == 'x3f':
        assert pp.shape == part.shape
        if s == 2:
            assert torch.equal(part, pp)
        else:
            # the lean form adds a unit's 16 values in fp32 before the double accumulation, the plane route adds every value in double: 15 additions,
            # the product's and the subtraction's rounding, 2^-24 each, of the sum of the terms' magnitudes: 1.01e-6 at worst -- the bar is 2e-6 of it
            t1, t2 = g.abs().sum(dim=(0, 1, 2)), (g * dev_).abs().sum(dim=(0, 1, 2)) * d.invstd.double()
            diff = (part.sum(0) - pp.sum(0)).abs()
            print('partials against the plane route: %.3e / %.3e of the terms' % (float((diff[:, 0] / t1).max()), float((diff[:, 1] / t2).max())))
            assert bool((diff[:, 0] <= 2e-6 * t1).all()) and bool((diff[:, 1] <= 2e-6 * t2).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# weight gradients

def _wgrad_id(c):
    return 'B%d_%dx%d_%dto%d_k%ds%d' % c[:7] + ('_bn%d' % c[7] if len(c) > 7 else '')


def _wgrad_operands(B, H, W, ci, co, k, s):
    Ho, Wo = K.out_hw(H, W, k, s, K.pad_of(k))
    return _det((B, ci, H, W), 31), _det((B, co, Ho, Wo), 32) * 1e-3


def _workspace(z, nbytes, co, ci, k):
    """guarded workspace of exactly the advertised size.  Its margins are at least one split's partials long (Cout x taps x Cin floats): a plan with one
    split more than advertised lands in the margin -- inside the test's own allocation -- and is reported, instead of leaving it"""
    split = co * k * k * ci * 4
    return z.guarded((nbytes // 4,), name='workspace', margin=max(64 << 10, (split + 255) // 256 * 256))


def _wgrad_twice(z, call, ref, co, ci, k, what):
    """accumulate = 0, then 1, against float64: 2e-5 / 4e-5 of the maximum (test_conv_wgrad_x3_vs_float64); dw guarded, the zone checked after each call"""
    dw = z.guarded((co, ci, k, k), name='dw')
    hipabi.check(call(dw, 0), what)
    z.check()
    _assert_grad_bar(dw, ref, what)
    hipabi.check(call(dw, 1), what + ' accumulate')
    z.check()
    _assert_grad_bar(dw, 2 * ref, what + ' accumulate', bar=4e-5)


@pytest.mark.parametrize('c', K.WGRAD_HALO + K.WGRAD_TAP, ids=_wgrad_id)
def test_conv_wgrad_x3_on_planes_inside_the_advertised_workspace(dev, c):
    """straps_conv_wgrad_x3 with planes (the fp32 tensors NULL): the halo-patch plan at its smallest and oddest geometries (32- and 64-pixel chunks,
    nchunks no multiple of chunks_per_split), the per-tap kernel at every block of wgrad_x3_block, M = 1 ... 129, short and EMPTY last splits, every bound
    of the split count.  The workspace is guarded, NaN-filled and exactly straps_conv_wgrad_workspace_bytes long -- sized by the fp32 plan, while these
    kernels choose their own blocks and splits."""
    L = hipabi.lib()
    B, H, W, ci, co, k, s = c
    pad = K.pad_of(k)
    assert L.straps_conv_wgrad_x3_on_planes(B, H, W, ci, co, k, k, s, pad) == 1
    x, dy = _wgrad_operands(B, H, W, ci, co, k, s)
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dy.double(), stride=s, padding=pad).to(dev)
    z = Zone(dev)
    x3, xps, _ = _act_planes(z, _nhwc(x))
    g3, gps, _ = _act_planes(z, _nhwc(dy))
    nbytes = L.straps_conv_wgrad_workspace_bytes(B, H, W, ci, co, k, k, s, pad)
    assert nbytes == K.wgrad_workspace_bytes(B, H, W, ci, co, k, s, pad)
    ws = _workspace(z, nbytes, co, ci, k)
    _wgrad_twice(z, lambda dw, acc: L.straps_conv_wgrad_x3(None, None, P(x3), xps, P(g3), gps, P(dw), P(ws), B, H, W, ci, co, k, k, s, pad, acc, None), ref, co, ci, k,
                 'wgrad_x3 %s' % (K.wgrad_plan(B, H, W, ci, co, k, s, pad).inst,))


@pytest.mark.parametrize('c', K.WGRAD_F32, ids=_wgrad_id)
def test_conv_wgrad_fp32_kernels_inside_the_advertised_workspace(dev, c):
    """straps_conv_wgrad, and straps_conv_wgrad_x3 without planes (the same kernels): both square blocks and the fp32 halo-patch kernel"""
    L = hipabi.lib()
    B, H, W, ci, co, k, s = c
    pad = K.pad_of(k)
    x, dy = _wgrad_operands(B, H, W, ci, co, k, s)
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dy.double(), stride=s, padding=pad).to(dev)
    z = Zone(dev)
    xd, gd = z.at_end(_nhwc(x)), z.at_end(_nhwc(dy))
    ws = _workspace(z, L.straps_conv_wgrad_workspace_bytes(B, H, W, ci, co, k, k, s, pad), co, ci, k)
    _wgrad_twice(z, lambda dw, acc: L.straps_conv_wgrad(P(xd), P(gd), P(dw), P(ws), B, H, W, ci, co, k, k, s, pad, acc, None), ref, co, ci, k, 'wgrad')
    ws.fill_(float('nan'))
    _wgrad_twice(z, lambda dw, acc: L.straps_conv_wgrad_x3(P(xd), P(gd), None, 0, None, 0, P(dw), P(ws), B, H, W, ci, co, k, k, s, pad, acc, None), ref, co, ci, k,
                 'wgrad_x3 (no planes)')


@pytest.mark.parametrize('c', K.WGRAD_X3F, ids=lambda c: 'B%d_%dx%d_%dto%d_s%d_bn%d' % c)
def test_conv_wgrad_x3f_inside_the_advertised_workspace(dev, c):
    """straps_conv_wgrad_x3f: every channel block, with and without the operand-path BatchNorm + ReLU, at M = 1 ... 129, ragged and empty last splits, the
    workspace guarded and exactly straps_conv_wgrad_x3f_workspace_bytes long"""
    L = hipabi.lib()
    B, H, W, ci, co, s, bn = c
    x, dy = _wgrad_operands(B, H, W, ci, co, 1, s)
    sc, sh = _det((ci,), 1703, 0.5, 1.5), _det((ci,), 1704, -0.5, 0.5)
    act = x.double()
    if bn:
        act = (x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).double().clamp_min(0)      # (the fp32 fmaf's rounding is inside the bar)
    ref = torch.nn.grad.conv2d_weight(act, (co, ci, 1, 1), dy.double(), stride=s).to(dev)
    z = Zone(dev)
    xd, gd = z.at_end(_nhwc(x)), z.at_end(_nhwc(dy))
    scd, shd = (z.at_end(sc), z.at_end(sh)) if bn else (None, None)
    nbytes = L.straps_conv_wgrad_x3f_workspace_bytes(B, H, W, ci, co, 1, 1, s, 0)
    assert nbytes == K.wgrad_x3f_workspace_bytes(B, H, W, ci, co, 1, s, 0) > 0
    ws = _workspace(z, nbytes, co, ci, 1)
    _wgrad_twice(z, lambda dw, acc: L.straps_conv_wgrad_x3f(P(xd), P(scd), P(shd), int(bn), P(gd), P(dw), P(ws), B, H, W, ci, co, 1, 1, s, 0, acc, None), ref, co, ci, 1,
                 'wgrad_x3f')
