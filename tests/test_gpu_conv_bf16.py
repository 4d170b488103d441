"""GPU: the single-product bf16 convolution (straps_conv_fwd_bf16, csrc/conv_bf16.hip) against its EXACT model -- a float64 convolution of
rn_bf16(x) and rn_bf16(w) with the epilogue in float64.  The products are exact in the fp32 accumulator, so only the summation order
differs from the model: the bars are the fp32 chain's of tests/test_gpu_conv_x3.py (2e-5 abs + 2e-5 rel raw, 3e-5 fused).  The output
plane is rn_bf16 of the fp32 output bit for bit; on bf16-exact operands the route agrees with the validated bf16x3 route.  The tile and
K-stage edges of every configuration, behind redzones and with stated refusals, are in tests/test_gpu_conv_bf16_edges.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import straps_amd
from bf16x3_emul import bf16_bits_to_f32, bf16_rn_bits
from straps_amd import hipabi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
from sweep_conv_bf16 import eval_conv_shapes  # noqa: E402

pytestmark = pytest.mark.gpu
NCFG = 10


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _rn(t):
    """rn_bf16 of a float32 CPU tensor, as float64"""
    return torch.from_numpy(bf16_bits_to_f32(bf16_rn_bits(t.numpy())).astype(np.float64)).reshape(t.shape)


def _cm(t):
    """chunk-major order (csrc/common.h cm_index) of an NHWC tensor [..., C]"""
    C = t.shape[-1]
    return t.reshape(-1, C // 32, 32).permute(1, 0, 2).contiguous().reshape(-1)


def _run(dev, x, w, ss, res, relu, stride, pad, cfg, want_y=True, want_plane=True):
    """x NHWC fp32 CPU, w OIHW fp32 CPU -> (y [B,Ho,Wo,Cout] or None, plane (int16, chunk-major) or None, return code)"""
    L = hipabi.lib()
    B, H, W, cin = x.shape
    cout, _, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xd, wd = x.to(dev).contiguous(), w.to(dev).contiguous()
    x1 = torch.empty(xd.numel(), dtype=torch.int16, device=dev)
    w1 = torch.empty(wd.numel(), dtype=torch.int16, device=dev)
    hipabi.check(L.straps_split_bf16_cm(hipabi.ptr(xd), hipabi.ptr(x1), B * H * W, cin, None), 'split')
    hipabi.check(L.straps_pack_conv_weight_bf16(hipabi.ptr(wd), hipabi.ptr(w1), cout, cin, k, k, None), 'pack')
    y = torch.full((B, Ho, Wo, cout), float('nan'), device=dev) if want_y else None
    yp = torch.full(((B * Ho * Wo * cout + 7) // 8 * 8,), -1, dtype=torch.int16, device=dev) if want_plane else None
    ssd = ss.to(dev) if ss is not None else None
    resd = res.to(dev).contiguous() if res is not None else None
    rc = L.straps_conv_fwd_bf16(hipabi.ptr(x1), hipabi.ptr(w1), hipabi.ptr(ssd[0] if ssd is not None else None),
                                hipabi.ptr(ssd[1] if ssd is not None else None), hipabi.ptr(resd), int(relu), hipabi.ptr(y), hipabi.ptr(yp),
                                B, H, W, cin, cout, k, k, stride, pad, cfg, None)
    torch.cuda.synchronize()
    return (y.cpu() if y is not None else None), (yp.cpu() if yp is not None else None), rc


def _model(x, w, ss, res, relu, stride, pad):
    """float64: conv(rn_bf16(x), rn_bf16(w)), then scale / shift, residual, ReLU"""
    xr = _rn(x).permute(0, 3, 1, 2)
    y = F.conv2d(xr, _rn(w), None, stride, pad).permute(0, 2, 3, 1)
    if ss is not None:
        y = y * ss[0].double() + ss[1].double()
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0) if relu else y


def _check(y, ref, tol, what):
    err = float(((y.double() - ref).abs() / (tol + tol * ref.abs())).max())
    assert err <= 1.0, '%s: %.3f of the %.0e bar' % (what, err, tol)


def _operands(B, H, W, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, H, W, cin, generator=g) * 2 - 1
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    return x, w, g


SHAPES = sorted(set(eval_conv_shapes(18) + eval_conv_shapes(50)))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_%d-%d_k%d_s%d' % s[:6])
def test_every_eval_shape_every_tile_against_exact_model(dev, shape):
    """every resnet18/50 eval convolution shape (B = 1, 256 x 256 input), fused epilogue (folded BatchNorm, residual, ReLU) on every tile
    configuration the geometry admits -- the automatic rule's among them -- and the raw convolution on the rule's; the plane output equals
    rn_bf16 of the fp32 output bit for bit"""
    H, W, cin, cout, k, s, p, _ = shape
    x, w, g = _operands(1, H, W, cin, cout, k, hash(shape) & 0xffff)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    ss = torch.stack([torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) - 0.5])
    res = torch.rand(1, Ho, Wo, cout, generator=g) - 0.5
    ref = _model(x, w, ss, res, True, s, p)
    rule = hipabi.lib().straps_conv_bf16_tile_choice(1, H, W, cin, cout, k, k, s, p)
    assert 1 <= rule <= NCFG
    ran = []
    for cfg in range(1, NCFG + 1):
        y, yp, rc = _run(dev, x, w, ss, res, True, s, p, cfg)
        if rc != 0:
            assert cfg != rule, 'the rule picked a configuration the geometry does not admit: %s' % hipabi.lib().straps_last_error().decode()
            continue
        ran.append(cfg)
        _check(y, ref, 3e-5, 'cfg %d fused' % cfg)
        want = torch.from_numpy(bf16_rn_bits(_cm(y).numpy()).view(np.int16))
        assert torch.equal(yp[:want.numel()], want), 'cfg %d: output plane != rn_bf16(y)' % cfg
    assert rule in ran
    y, _, rc = _run(dev, x, w, None, None, False, s, p, 0, want_plane=False)
    assert rc == 0
    _check(y, _model(x, w, None, None, False, s, p), 2e-5, 'raw, automatic tile')


@pytest.mark.parametrize('geom', [(3, 7, 9, 64, 128, 3, 2, 1), (2, 5, 11, 128, 64, 1, 1, 0), (1, 9, 9, 256, 128, 3, 1, 1), (5, 8, 8, 512, 512, 3, 1, 1)])
def test_ragged_tiles_and_output_forms(dev, geom):
    """ragged last M tiles (M not a multiple of any tile), plane-only and fp32-only outputs, every admitted configuration"""
    B, H, W, cin, cout, k, s, p = geom
    x, w, g = _operands(B, H, W, cin, cout, k, 7 + cin)
    ss = torch.stack([torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) - 0.5])
    ref = _model(x, w, ss, None, True, s, p)
    for cfg in range(0, NCFG + 1):
        y, yp_full, rc = _run(dev, x, w, ss, None, True, s, p, cfg)
        if rc != 0:
            continue
        _check(y, ref, 3e-5, 'cfg %d' % cfg)
        _, yp, rc = _run(dev, x, w, ss, None, True, s, p, cfg, want_y=False)
        assert rc == 0 and torch.equal(yp, yp_full), 'cfg %d: plane-only output differs' % cfg
        y2, _, rc = _run(dev, x, w, ss, None, True, s, p, cfg, want_plane=False)
        assert rc == 0 and torch.equal(y2, y), 'cfg %d: fp32-only output differs' % cfg


@pytest.mark.parametrize('geom', [(2, 16, 16, 64, 64, 3, 1, 1), (1, 16, 16, 128, 256, 3, 2, 1), (2, 8, 8, 256, 512, 1, 2, 0), (1, 8, 8, 2048, 512, 1, 1, 0)])
def test_agrees_with_bf16x3_on_bf16_exact_operands(dev, geom):
    """operands that are already bf16-exact have zero lower planes: the bf16x3 route computes the same exact products, and the two routes
    differ by accumulation order only -- each within the fp32 bar of the float64 model, and of each other"""
    B, H, W, cin, cout, k, s, p = geom
    x, w, g = _operands(B, H, W, cin, cout, k, 99)
    x, w = _rn(x).float(), _rn(w).float()
    ss = torch.stack([torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) - 0.5])
    ref = _model(x, w, ss, None, True, s, p)
    y1, _, rc = _run(dev, x, w, ss, None, True, s, p, 0)
    assert rc == 0
    from straps_amd.encoder_exec import split3, weight_planes
    L = hipabi.lib()
    xd = x.to(dev).contiguous()
    x3, xps = split3(L, xd)
    assert int((x3[1:] != 0).sum()) == 0          # (the lower planes of bf16-exact values are zero)
    w3, wps = weight_planes(L, w.to(dev))
    y3 = torch.empty_like(y1, device=dev)
    ssd = ss.to(dev)
    hipabi.check(L.straps_conv_fwd_x3(hipabi.ptr(x3), xps, hipabi.ptr(w3), wps, hipabi.ptr(ssd[0]), hipabi.ptr(ssd[1]), None, 1, hipabi.ptr(y3), None,
                                      B, H, W, cin, cout, k, k, s, p, 0, None), 'x3')
    y3 = y3.cpu()
    _check(y1, ref, 3e-5, 'bf16 route')
    _check(y3, ref, 3e-5, 'bf16x3 route')
    _check(y1, y3.double(), 6e-5, 'bf16 vs bf16x3')


def test_split_and_pack_are_rn_bf16(dev):
    L = hipabi.lib()
    x, w, _ = _operands(3, 5, 7, 96, 64, 3, 5)
    x[0, 0, 0, :4] = torch.tensor([float('inf'), -float('inf'), 1e-40, -0.0])
    xd = x.to(dev)
    x1 = torch.empty(xd.numel(), dtype=torch.int16, device=dev)
    hipabi.check(L.straps_split_bf16_cm(hipabi.ptr(xd), hipabi.ptr(x1), 3 * 5 * 7, 96, None), 'split')
    assert torch.equal(x1.cpu(), torch.from_numpy(bf16_rn_bits(_cm(x).numpy()).view(np.int16)))
    # the single plane is plane 0 of the bf16x3 split and of the bf16x3 weight pack
    from straps_amd.encoder_exec import split3, weight_planes
    x3, _ = split3(L, xd)
    assert torch.equal(x1, x3[0, :x1.numel()])
    wd = w.to(dev)
    w1 = torch.empty(wd.numel(), dtype=torch.int16, device=dev)
    hipabi.check(L.straps_pack_conv_weight_bf16(hipabi.ptr(wd), hipabi.ptr(w1), 64, 96, 3, 3, None), 'pack')
    w3, _ = weight_planes(L, wd)
    assert torch.equal(w1, w3[0, :w1.numel()])
