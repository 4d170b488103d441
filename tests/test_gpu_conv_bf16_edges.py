"""GPU: the single-product bf16 inference convolutions (straps_conv_fwd_bf16, csrc/conv_bf16.hip: the PL != 0 instantiations of conv_x3_kernels.h with
the EPI = 3 plane epilogue) at their tile and K-stage edges, behind redzones (tests/redzone.py), and the route's split and pack kernels at theirs --
the cases of tests/conv_cases.py (BF16_*), which also states which of the ten tile configurations each case reaches and which refuse it
(tests/test_conv_cases_cpu.py holds that statement to the library).

Common form of every convolution case, as in tests/test_gpu_conv_edges.py:
  * y and y_plane come from Zone.guarded, exactly B*Ho*Wo*cout elements (the plane is int16, pre-filled with the bf16 NaN 0x7FC0), sentinel margins
    on both sides: a write in front of either, or past the plane's advertised extent, shows;
  * scale, shift and residual come from Zone.at_end (NaN directly behind the last element); the activation plane and the weight plane are made by
    straps_split_bf16_cm / straps_pack_conv_weight_bf16 into scratch and copied with Zone.at_end, so that 0x7FC0 words lie directly in front of and
    behind them -- an over-read of a chunk whose value is used (a padding pixel that does not read the zero constant in every K slot of its stage, a
    K loop one stage too long) is a NaN in the result;
  * the reference is the route's exact model (tests/test_gpu_conv_bf16.py): the float64 convolution of rn_bf16(x) and rn_bf16(w), epilogue in float64,
    on the CPU; det_uniform data, weights scaled by (2 / (cin k k))^0.5.

Every case runs under EVERY configuration 1..10 (the automatic-rule cases under tile_cfg 0): where conv_cases.bf16_refusal admits it, three epilogue
forms (raw; folded BatchNorm + ReLU; folded BatchNorm + residual + ReLU), each asserting (a) finite and within the route's bars -- 2e-5 abs + 2e-5 rel
raw, 3e-5 + 3e-5 fused, (b) y_plane == rn_bf16(y) bit for bit in chunk-major order, the same plane bits with y = NULL, the same y bits with
y_plane = NULL, (c) the same bits on a second call, (d) the guards; where it refuses, (e) a non-zero return code, the stated reason in
straps_last_error(), outputs still all NaN and guards intact.  No configuration is skipped: a refusal where the table says it runs fails, and so does
a run where the table says refused.

Bit equality BETWEEN tile configurations is not promised and not asserted.  Each case prints whether the plain and the software-pipelined loop of the
same tile (cfg 4 / 5 and cfg 1 / 7) agree; DESIGN.md records the observation.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as K
import straps_amd  # noqa: F401
from bf16x3_emul import bf16_bits_to_f32, bf16_rn_bits
from detgen import det_uniform
from redzone import BF16_NAN, Zone
from straps_amd import hipabi
from straps_amd.encoder_exec import weight_planes

pytestmark = pytest.mark.gpu
P = hipabi.ptr
RAW_BAR, FUSED_BAR = 2e-5, 3e-5          # tests/test_gpu_conv_bf16.py: |err| <= bar + bar |ref|
FORMS = ('raw', 'bn_relu', 'bn_res_relu')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    lib = hipabi.load()
    assert os.path.abspath(lib._name) == os.path.abspath(hipabi.LIB_PATH), 'these tests compare bit for bit on the product library, not %s' % lib._name
    return torch.device('cuda:0')


_PERIOD = (1 << 19) + 17          # (odd against every channel count and row length of the tables)


def _det(shape, seed, lo=-1.0, hi=1.0):
    """det_uniform data as a CPU tensor; beyond 2^19 elements one det_uniform block repeated"""
    n = 1
    for d in shape:
        n *= d
    if n <= _PERIOD:
        return torch.from_numpy(det_uniform(tuple(shape), seed, lo, hi))
    blk = torch.from_numpy(det_uniform((_PERIOD,), seed, lo, hi))
    return blk.repeat(-(-n // _PERIOD))[:n].view(tuple(shape)).contiguous()


def _rn64(t):
    """rn_bf16 of a float32 CPU tensor, as float64"""
    return torch.from_numpy(bf16_bits_to_f32(bf16_rn_bits(t.numpy())).astype(np.float64)).reshape(t.shape)


def _cm(t):
    """chunk-major order (csrc/common.h cm_index: element (row, c) at ((c / 32) * rows + row) * 32 + c % 32) of a tensor [..., C], flat"""
    C = t.shape[-1]
    return t.reshape(-1, C // 32, 32).permute(1, 0, 2).contiguous().reshape(-1)


def _rn_plane(y):
    """fp32 [..., C] (any device) -> what the plane must hold: bf16_rn_bits of the values (oracle/bf16x3_emul.py) in chunk-major order, int16 on the CPU"""
    return torch.from_numpy(bf16_rn_bits(_cm(y.cpu()).numpy()).view(np.int16))


def _bits(y):
    return y.view(torch.int32)


class _Conv:
    """one geometry on the device: operand planes between NaN words, the epilogue operands at the end of poison, four guarded outputs that every call
    of the case re-fills and re-uses, and the float64 model of the three epilogue forms"""

    def __init__(self, dev, c, x=None):
        L = hipabi.lib()
        self.c, self.dev = c, dev
        B, H, W, ci, co, k, s = c
        self.pad = k // 2
        self.p = K.bf16_problem(c)
        Ho, Wo = K.out_hw(H, W, k, s, self.pad)
        self.shape = (B, Ho, Wo, co)
        self.n = B * Ho * Wo * co
        self.x = _det((B, ci, H, W), 1).permute(0, 2, 3, 1).contiguous() if x is None else x          # NHWC
        self.w = _det((co, ci, k, k), 2) * (2.0 / (ci * k * k)) ** 0.5
        z = self.z = Zone(dev)
        # the planes: made in scratch, re-homed so that 0x7FC0 lies directly in front of the first and behind the last element
        xd, wd = z.at_end(self.x), z.at_end(self.w)
        x1 = torch.empty(xd.numel(), dtype=torch.int16, device=dev)
        w1 = torch.empty(wd.numel(), dtype=torch.int16, device=dev)
        hipabi.check(L.straps_split_bf16_cm(P(xd), P(x1), B * H * W, ci, None), 'split')
        hipabi.check(L.straps_pack_conv_weight_bf16(P(wd), P(w1), co, ci, k, k, None), 'pack')
        torch.cuda.synchronize()
        self.x1, self.w1 = z.at_end(x1), z.at_end(w1)
        assert self.x1.data_ptr() % 16 == 0 and self.w1.data_ptr() % 16 == 0          # (what the entry point requires)
        self.sc = z.at_end(_det((co,), 3, 0.5, 1.5))
        self.sh = z.at_end(_det((co,), 4, -0.5, 0.5))
        self.res = z.at_end(_det(self.shape, 5))
        self.y = [z.guarded(self.shape, name='y %d' % i) for i in (0, 1)]
        self.yp = [z.guarded((self.n,), torch.int16, fill=BF16_NAN, name='y_plane %d' % i) for i in (0, 1)]
        self._ref = None

    def ref(self, form):
        """float64 on the device: conv(rn_bf16(x), rn_bf16(w)), then scale / shift, residual, ReLU"""
        if self._ref is None:
            B, H, W, ci, co, k, s = self.c
            raw = F.conv2d(_rn64(self.x).permute(0, 3, 1, 2), _rn64(self.w), None, s, self.pad).permute(0, 2, 3, 1).contiguous().to(self.dev)
            bn = raw * self.sc.double() + self.sh.double()
            self._ref = {'raw': raw, 'bn_relu': bn.clamp_min(0), 'bn_res_relu': (bn + self.res.double()).clamp_min(0)}
        return self._ref[form]

    def call(self, cfg, form, slot, want_y=True, want_plane=True):
        """one call into output slot 0 / 1 (both outputs of the slot NaN-filled first) -> return code; the zone is checked"""
        B, H, W, ci, co, k, s = self.c
        self.y[slot].fill_(float('nan'))
        self.yp[slot].fill_(BF16_NAN)
        bn, res = form != 'raw', form == 'bn_res_relu'
        rc = hipabi.lib().straps_conv_fwd_bf16(P(self.x1), P(self.w1), P(self.sc if bn else None), P(self.sh if bn else None), P(self.res if res else None),
                                               int(bn), P(self.y[slot] if want_y else None), P(self.yp[slot] if want_plane else None),
                                               B, H, W, ci, co, k, k, s, self.pad, cfg, None)
        self.z.check()
        return rc

    def untouched(self, slot):
        return bool(torch.isnan(self.y[slot]).all()) and bool((self.yp[slot] == BF16_NAN).all())

    def run_admitted(self, cfg, tag):
        """assertions (a) - (d) for every epilogue form -> ({form: worst error as a fraction of its bar}, {form: the bits of y})"""
        worst, bits = {}, {}
        for form in FORMS:
            what = '%s cfg %d %s' % (tag, cfg, form)
            rc = self.call(cfg, form, 0)
            assert rc == 0, '%s: refused where the table says it runs: %s' % (what, hipabi.lib().straps_last_error().decode())
            y, yp = self.y[0], self.yp[0]
            assert bool(torch.isfinite(y).all()), '%s: not finite' % what
            bar = RAW_BAR if form == 'raw' else FUSED_BAR
            ref = self.ref(form)
            worst[form] = float(((y.double() - ref).abs() / (bar + bar * ref.abs())).max())
            assert worst[form] <= 1.0, '%s: %.3f of the %.0e bar' % (what, worst[form], bar)
            assert torch.equal(yp.cpu(), _rn_plane(y)), '%s: y_plane != rn_bf16(y) in chunk-major order' % what
            assert self.call(cfg, form, 1, want_y=False) == 0 and torch.equal(self.yp[1], yp), '%s: the plane differs with y = NULL' % what
            assert bool(torch.isnan(self.y[1]).all())
            assert self.call(cfg, form, 1, want_plane=False) == 0 and torch.equal(_bits(self.y[1]), _bits(y)), '%s: y differs with y_plane = NULL' % what
            assert bool((self.yp[1] == BF16_NAN).all())
            assert self.call(cfg, form, 1) == 0 and torch.equal(_bits(self.y[1]), _bits(y)) and torch.equal(self.yp[1], yp), '%s: a second call gives other bits' % what
            bits[form] = _bits(y).clone()
        return worst, bits

    def run_refused(self, cfg, why, tag):
        """assertion (e)"""
        rc = self.call(cfg, 'bn_res_relu', 0)
        err = hipabi.lib().straps_last_error().decode()
        assert rc != 0, '%s cfg %d ran where the table says refused (%s)' % (tag, cfg, why)
        assert why in err and ('tile_cfg %d:' % cfg) in err, '%s cfg %d: refused with %r, expected %r' % (tag, cfg, err, why)
        assert self.untouched(0), '%s cfg %d: a refused call wrote its outputs' % (tag, cfg)


def _report(tag, worst, bits):
    """one line per case for the log: the worst error over configurations and forms as a fraction of its bar, and whether the plain and the pipelined
    loop of the same tile gave the same bits (an observation, not an assertion: the code does not promise it)"""
    raw = max(w['raw'] for w in worst.values())
    fused = max(max(w['bn_relu'], w['bn_res_relu']) for w in worst.values())
    pairs = []
    for a, b in ((4, 5), (1, 7)):
        if a in bits and b in bits:
            pairs.append('cfg %d == cfg %d: %s' % (a, b, all(torch.equal(bits[a][f], bits[b][f]) for f in FORMS)))
    print('bf16 edges %s: worst raw %.4f of the %.0e bar, worst fused %.4f of the %.0e bar; %s' % (tag, raw, RAW_BAR, fused, FUSED_BAR, '; '.join(pairs) or 'no pair'))


@pytest.mark.parametrize('c', K.BF16_EXPLICIT, ids=K.bf16_case_id)
def test_conv_fwd_bf16_every_configuration_at_tile_and_stage_edges(dev, c):
    """K loops of 1, 2, 3, 4 stages (fewer than, exactly and one more than the prologue issues, both pipelined loops among them), the tap rolling over
    at every stage, M = 1, BM - 1, BM, BM + 1 and ragged two-tile M for every row tile, padding pixels in every K slot, stride 2 on odd extents, cout
    64 / 128 / 192 / 320, the halo-patch tiles at 180 ... 264 slots and their refusals -- one geometry, all ten configurations, one reference."""
    cv = _Conv(dev, c)
    tag = K.bf16_case_id(c)
    worst, bits = {}, {}
    for cfg in K.BF16_TILES:
        why = K.bf16_refusal(cv.p, cfg)
        if why is None:
            worst[cfg], bits[cfg] = cv.run_admitted(cfg, tag)
        else:
            cv.run_refused(cfg, why, tag)
    assert worst, 'no configuration admits the case'
    _report(tag, worst, bits)


@pytest.mark.parametrize('c,want', list(zip(K.BF16_AUTO, K.BF16_AUTO_WANT)), ids=lambda v: K.bf16_case_id(v) if isinstance(v, tuple) else 'cfg%d' % v)
def test_conv_fwd_bf16_automatic_rule_at_its_thresholds(dev, c, want):
    """tile_cfg = 0 at 255 / 256 / 511 / 512 tile equivalents (cfg 3 / 1 / 1 / 5) and at 64 and 192 output channels with 512 M tiles (cfg 3): the rule
    picks the stated configuration, and the launch it makes gives the bits of that configuration named explicitly"""
    L = hipabi.lib()
    B, H, W, ci, co, k, s = c
    assert L.straps_conv_bf16_tile_choice(B, H, W, ci, co, k, k, s, k // 2) == want == K.bf16_route(K.bf16_problem(c), 0)[1]
    cv = _Conv(dev, c)
    tag = K.bf16_case_id(c) + '_cfg0'
    worst, bits = cv.run_admitted(0, tag)
    assert cv.call(want, 'bn_res_relu', 1) == 0 and torch.equal(_bits(cv.y[1]), bits['bn_res_relu']), 'tile_cfg 0 and the configuration it names give other bits'
    _report(tag, {0: worst}, {})


@pytest.mark.parametrize('c,cfg', K.BF16_BATCH, ids=lambda v: K.bf16_case_id(v) if isinstance(v, tuple) else 'cfg%d' % v)
def test_conv_fwd_bf16_bodies_do_not_see_each_other(dev, c, cfg):
    """tiles that span several images (a 128-row im2col tile over three 5x5 maps; a halo patch of two 8x8 images): the rows of a body are the same bits
    whatever the other bodies hold -- NaN in all of them -- and, where the configuration admits a batch of one, the same bits as the body alone"""
    B, H, W, ci, co, k, s = c
    full = _Conv(dev, c)
    assert full.call(cfg, 'bn_res_relu', 0) == 0, hipabi.lib().straps_last_error().decode()
    y, yp = full.y[0].clone(), full.yp[0].clone()
    assert bool(torch.isfinite(y).all())
    rows = y.shape[1] * y.shape[2]
    plane = yp.view(co // 32, B, rows, 32)          # chunk-major: [chunk][body][pixel][32]
    for b in range(B):
        x = torch.full_like(full.x, float('nan'))
        x[b] = full.x[b]
        other = _Conv(dev, c, x=x)
        assert other.call(cfg, 'bn_res_relu', 0) == 0
        assert torch.equal(_bits(other.y[0][b]), _bits(y[b])), 'body %d changes with the other bodies of the batch' % b
        assert torch.equal(other.yp[0].view(co // 32, B, rows, 32)[:, b], plane[:, b]), 'body %d: the plane changes with the other bodies' % b
        c1 = (1,) + tuple(c[1:])
        if K.bf16_refusal(K.bf16_problem(c1), cfg) is None:
            alone = _Conv(dev, c1, x=full.x[b:b + 1].contiguous())
            alone.res.copy_(full.res[b:b + 1])
            assert alone.call(cfg, 'bn_res_relu', 0) == 0
            assert torch.equal(_bits(alone.y[0][0]), _bits(y[b])), 'body %d alone differs from its rows in the batch' % b
            assert torch.equal(alone.yp[0].view(co // 32, rows, 32), plane[:, b]), 'body %d alone: the plane differs' % b


# ----------------------------------------------------------------------------------------------------------------------------------------
# split and pack: exactly bf16_rn_bits of oracle/bf16x3_emul.py, which defines the bits of EVERY pattern (it rounds the bit pattern: the canonical
# quiet NaN 0x7FC00000 stays 0x7FC0), so NaN positions are compared bit for bit like the rest

SPECIALS = np.array([
    0x3F808000, 0x3F818000,          # exact ties: upper half even (stays 0x3F80), odd (rounds up to 0x3F82)
    0x3F807FFF, 0x3F808001,          # just below / above a tie
    0xBF818000, 0xBF807FFF,          # the same with the sign set
    0x3F7FFFFF,                      # a mantissa carry into the exponent (-> 0x3F80)
    0x7F7FFFFF,                      # the largest finite fp32 (the emulator rounds it to 0x7F80, +inf: round to nearest has no larger finite bf16)
    0x00800000,                      # the smallest normal
    0x00000001, 0x00008000, 0x007FFFFF, 0x80008001,          # denormals: the smallest, a tie to zero, the largest (carries into the normals), negative
    0x00000000, 0x80000000,          # +-0
    0x7F800000, 0xFF800000,          # +-inf
    0x7FC00000,                      # a NaN
], dtype=np.uint32)


def _plant(flat, trip):
    """SPECIALS at the first elements, the last elements and (if the array reaches it) the first elements of the second grid trip, at element `trip`;
    an array too short for all of them gets the first half in front and the last half at the end"""
    v = torch.from_numpy(SPECIALS.view(np.float32).copy())
    n, m = flat.numel(), min(len(SPECIALS), flat.numel() // 2)
    flat[:m] = v[:m]
    flat[n - m:] = v[len(v) - m:]
    if n >= trip + len(v):
        flat[trip:trip + len(v)] = v
    return flat


@pytest.mark.parametrize('rows,c', K.BF16_SPLIT, ids=lambda v: str(v))
def test_split_bf16_cm_is_rn_bf16_at_its_edges(dev, rows, c):
    """one row, one chunk, several chunks, a row count that is no multiple of anything, exactly the grid cap and four rows past it (the second trip of
    the grid-stride loop); ties, carries, the largest finite value, denormals, zeros, infinities and a NaN at the first, the last and the first
    second-trip element; the output guarded and exactly rows * c elements"""
    L = hipabi.lib()
    x = _plant(_det((rows * c,), 6, -4.0, 4.0), 4 * K.BF16_GRID_CAP).view(rows, c)
    z = Zone(dev)
    xd = z.at_end(x)
    out = z.guarded((rows * c,), torch.int16, fill=BF16_NAN, name='plane')
    hipabi.check(L.straps_split_bf16_cm(P(xd), P(out), rows, c, None), 'split')
    z.check()
    want = torch.from_numpy(bf16_rn_bits(_cm(x).numpy()).view(np.int16))
    got = out.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, 'first difference at plane element %d: 0x%04x, expected 0x%04x' % (int(bad[0]), int(got[bad[0]]) & 0xFFFF, int(want[bad[0]]) & 0xFFFF)
    # the planted patterns round as the table above says (the emulator's answers, spelled out once)
    assert [int(v) for v in bf16_rn_bits(SPECIALS.view(np.float32))[:8]] == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0xBF82, 0xBF80, 0x3F80, 0x7F80]
    assert [int(v) for v in bf16_rn_bits(SPECIALS.view(np.float32))[8:]] == [0x0080, 0, 0, 0x0080, 0x8001, 0, 0x8000, 0x7F80, 0xFF80, 0x7FC0]


def test_split_bf16_cm_refusals_write_nothing(dev):
    L = hipabi.lib()
    z = Zone(dev)
    xd = z.at_end(_det((4, 64), 6))
    out = z.guarded((4 * 64,), torch.int16, fill=BF16_NAN, name='plane')
    assert L.straps_split_bf16_cm(P(xd), P(out), 4, 48, None) != 0 and 'c % 32' in L.straps_last_error().decode()
    assert L.straps_split_bf16_cm(ctypes.c_void_p(xd.data_ptr() + 4), P(out), 3, 64, None) != 0 and 'aligned' in L.straps_last_error().decode()
    assert L.straps_split_bf16_cm(P(xd), ctypes.c_void_p(out.data_ptr() + 2), 3, 64, None) != 0 and 'aligned' in L.straps_last_error().decode()
    z.check()
    assert bool((out == BF16_NAN).all())


@pytest.mark.parametrize('co,ci,kh,kw', K.BF16_PACK, ids=lambda v: str(v))
def test_pack_conv_weight_bf16_is_rn_bf16_in_the_stated_layout(dev, co, ci, kh, kw):
    """element (o, tap, c) at ((tap * (cin / 32) + c / 32) * cout + o) * 32 + c % 32 (include/straps_hip.h, csrc/conv_bf16.hip), evaluated in numpy; one
    output channel, one chunk, 1x3 and 3x1 filters, a tensor past the grid cap; the output guarded and exactly cout * cin * kh * kw elements; for the
    square filters of the networks it is plane 0 of the bf16x3 weight pack"""
    L = hipabi.lib()
    rs = kh * kw
    w = _plant(_det((co * ci * rs,), 7) * (2.0 / (ci * rs)) ** 0.5, K.BF16_GRID_CAP).view(co, ci, kh, kw)
    z = Zone(dev)
    wd = z.at_end(w)
    out = z.guarded((co * ci * rs,), torch.int16, fill=BF16_NAN, name='w_plane')
    hipabi.check(L.straps_pack_conv_weight_bf16(P(wd), P(out), co, ci, kh, kw, None), 'pack')
    z.check()
    bits = bf16_rn_bits(w.numpy()).reshape(co, ci // 32, 32, rs)                  # [o][c / 32][c % 32][tap]
    want = torch.from_numpy(np.ascontiguousarray(bits.transpose(3, 1, 0, 2)).reshape(-1).view(np.int16))          # [tap][c / 32][o][c % 32]
    got = out.cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, 'first difference at plane element %d: 0x%04x, expected 0x%04x' % (int(bad[0]), int(got[bad[0]]) & 0xFFFF, int(want[bad[0]]) & 0xFFFF)
    if kh == kw and co % 32 == 0:
        w3, _ = weight_planes(L, wd)
        assert torch.equal(out, w3[0, :out.numel()]), 'not plane 0 of the bf16x3 weight pack'
