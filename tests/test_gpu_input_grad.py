"""GPU: gradients w.r.t. the proxy input -- the stem data-gradient kernel (straps_stem_dgrad) against float64 conv2d_input, the regressor's
x.grad against autograd of the float64 oracle on the GPU's ReLU / max-pool decisions, frozen parameters, unchanged parameter gradients,
the standalone encoder (reg.ief_module(reg.image_encoder(x))) and unchanged no-grad forwards."""
import json
import os

import numpy as np
import pytest
import torch

import straps_amd
import straps_oracle as O
import decisions
from detgen import det_uniform, det_state_dict
from straps_amd import hipabi

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
MP = straps_amd.synthetic_mean_params(0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    hipabi.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device('cuda:0')


def _maxrel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _stem_dgrad(dy, w, H, W, dx=None, accumulate=0):
    L = hipabi.lib()
    B, cin = dy.shape[0], w.shape[1]
    wp = torch.empty(L.straps_stem_dgrad_weight_floats(cin), device=dy.device, dtype=torch.float32)
    hipabi.check(L.straps_pack_stem_dgrad_weight(hipabi.ptr(w), hipabi.ptr(wp), cin, hipabi.stream_ptr()), 'straps_pack_stem_dgrad_weight')
    if dx is None:
        dx = torch.empty(B, cin, H, W, device=dy.device, dtype=torch.float32)
    hipabi.check(L.straps_stem_dgrad(hipabi.ptr(dy), hipabi.ptr(wp), hipabi.ptr(dx), B, cin, H, W, accumulate, hipabi.stream_ptr()),
                 'straps_stem_dgrad')
    torch.cuda.synchronize()
    return dx


def _ref(dy, w, H, W):
    return torch.nn.grad.conv2d_input((dy.shape[0], w.shape[1], H, W), w.cpu().double(), dy.cpu().double().permute(0, 3, 1, 2),
                                      stride=2, padding=3)


def _operands(B, cin, H, W, seed, dev):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.from_numpy(det_uniform((B, Ho, Wo, 64), seed, -1.0, 1.0)).to(dev)
    w = torch.from_numpy(det_uniform((64, cin, 7, 7), seed + 1, -0.5, 0.5)).to(dev)
    return dy, w


@pytest.mark.parametrize('hw', [(7, 7), (9, 13), (33, 50), (255, 257), (256, 256)])
@pytest.mark.parametrize('cin', [1, 3, 17, 18, 19, 64])
def test_stem_dgrad_vs_float64(dev, cin, hw):
    H, W = hw
    for B in (1, 3):
        dy, w = _operands(B, cin, H, W, 100 * cin + H + W + B, dev)
        dx = _stem_dgrad(dy, w, H, W)
        assert bool(torch.isfinite(dx).all()), 'non-finite element (an unwritten output on NaN-poisoned memory)'
        ref = _ref(dy, w, H, W)
        err = _maxrel(dx, ref)
        print('stem dgrad B=%d cin=%d %dx%d: max-norm rel err %.2e' % (B, cin, H, W, err))
        assert err <= 1e-5
        # accumulate = 1 adds to what is there
        base = torch.from_numpy(det_uniform(tuple(dx.shape), 7 + cin, -1.0, 1.0)).to(dev)
        acc = _stem_dgrad(dy, w, H, W, dx=base.clone(), accumulate=1)
        erra = _maxrel(acc, ref + base.cpu().double())
        assert erra <= 1e-5, erra


def test_stem_dgrad_b64_vs_float64(dev):
    B, cin, H, W = 64, 18, 256, 256
    dy, w = _operands(B, cin, H, W, 4242, dev)
    dx = _stem_dgrad(dy, w, H, W)
    assert bool(torch.isfinite(dx).all())
    worst = 0.0
    scale = 0.0
    errs = []
    for b0 in range(0, B, 16):
        ref = _ref(dy[b0:b0 + 16], w, H, W)
        errs.append(float((dx[b0:b0 + 16].cpu().double() - ref).abs().max()))
        scale = max(scale, float(ref.abs().max()))
    worst = max(errs) / scale
    print('stem dgrad B=64 cin=18 256x256: max-norm rel err %.2e' % worst)
    assert worst <= 1e-5


# ------------------------------------------------------------------------------------------ through the regressor
def _load_det(layers, dev, prec, train):
    reg = straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP)
    man = json.load(open(os.path.join(GOLD, 'state_dict_keys_r%d.json' % layers)))['keys']
    sd = {k: torch.from_numpy(v) for k, v in det_state_dict(man).items()}
    reg.load_state_dict(sd, strict=True)
    reg = reg.to(dev)
    reg.image_encoder.conv_precision = prec
    reg.train(train)
    return reg, sd


def _proxy_input(B, seed, dev):
    """proxy-like: a silhouette box in channel 0, Gaussian joint blobs in most heat-map channels, whole channels empty -- dx is checked
    where x is exactly zero"""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 18, 256, 256), np.float32)
    yy, xx = np.mgrid[0:256, 0:256]
    for b in range(B):
        y0, x0 = rng.integers(30, 90, 2)
        x[b, 0, y0:y0 + 140, x0:x0 + 90] = 1.0
        for j in range(1, 18):
            if j % 4 == 1:
                continue            # empty joint channel
            cy, cx = rng.integers(20, 236, 2)
            x[b, j] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * 4.0 ** 2)) * (np.abs(yy - cy) <= 8) * (np.abs(xx - cx) <= 8)
    return torch.from_numpy(x).to(dev)


CASES = [(18, 'bf16x3', False), (18, 'bf16x3', True), (18, 'fp32', False), (18, 'fp32', True), (50, 'bf16x3', False), (50, 'bf16x3', True)]


def _coef(B, dev):
    return torch.from_numpy(det_uniform((B, 157), 556)).to(dev)


def _taped_grad(reg, x, coef, freeze=False):
    """x.grad and {name: .grad} of loss = sum(outputs * coef) with the module's autograd"""
    reg.zero_grad(set_to_none=True)
    for p in reg.parameters():
        p.requires_grad_(not freeze)
    xr = x.clone().requires_grad_(True)
    out = torch.cat(reg(xr), 1)
    (out * coef).sum().backward()
    grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in reg.named_parameters()}
    for p in reg.parameters():
        p.requires_grad_(True)
    return xr.grad, grads, out.detach()


@pytest.mark.parametrize('layers,prec,train', CASES)
def test_regressor_input_grad_vs_float64_oracle(dev, layers, prec, train):
    reg, sd = _load_det(layers, dev, prec, train)
    B = 2
    x = _proxy_input(B, 11 + layers, dev)
    coef = _coef(B, dev)
    dec, feat = decisions.gpu_encoder_decisions(reg.image_encoder, x)
    masks = decisions.gpu_ief_masks(reg.ief_module, feat)
    gx, _, _ = _taped_grad(reg, x, coef)
    assert gx is not None and bool(torch.isfinite(gx).all())
    sd64 = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    x64 = x.cpu().double().requires_grad_(True)
    _, _, _, est = O.regressor_forward(x64, sd64, O.ief_init_estimate(MP['pose'], MP['shape']).double(), layers, 3, training=train,
                                       ief_masks=masks, enc_decisions={'relu': dec['relu'], 'pool': dec['pool']})
    (est * coef.cpu().double()).sum().backward()
    err = _maxrel(gx, x64.grad)
    zero = (x == 0).cpu()
    err0 = float((gx.cpu().double() - x64.grad)[zero].abs().max() / x64.grad.abs().max())
    bar = 2e-4 if layers == 18 else (1e-3 if train else 5e-4)
    print('r%d %s %s: x.grad max-norm rel err %.2e (where x == 0: %.2e; %.0f %% of x is zero)'
          % (layers, prec, 'train' if train else 'eval', err, err0, 100.0 * float(zero.float().mean())))
    assert err <= bar


@pytest.mark.parametrize('layers,prec,train', CASES)
def test_frozen_parameters_and_unchanged_parameter_grads(dev, layers, prec, train):
    """frozen parameters: x.grad bit-identical, every .grad stays None; parameter gradients bit-identical with or without x.grad (the dense
    stem-tail gradient an input gradient needs leaves conv1.weight's gradient alone)"""
    reg, _ = _load_det(layers, dev, prec, train)
    B = 2
    x = _proxy_input(B, 5, dev)
    coef = _coef(B, dev)
    gx, g1, out1 = _taped_grad(reg, x, coef)
    gx_f, gf, out_f = _taped_grad(reg, x, coef, freeze=True)
    assert torch.equal(gx, gx_f)
    assert torch.equal(out1, out_f)
    assert all(g is None for g in gf.values())
    # parameter gradients without an input gradient
    reg.zero_grad(set_to_none=True)
    out0 = torch.cat(reg(x), 1)
    (out0 * coef).sum().backward()
    for n, p in reg.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, g1[n]), n


@pytest.mark.parametrize('layers,prec,train', [(18, 'bf16x3', False), (18, 'bf16x3', True), (50, 'bf16x3', True), (18, 'fp32', False)])
def test_standalone_encoder_matches_regressor(dev, layers, prec, train):
    """reg.ief_module(reg.image_encoder(x)) in grad mode = reg(x): same launches, so features, outputs, parameter gradients and x.grad are
    bit-identical; in training mode the running statistics are updated exactly once either way"""
    reg, _ = _load_det(layers, dev, prec, train)
    B = 2
    x = _proxy_input(B, 9, dev)
    coef = _coef(B, dev)
    buf0 = {n: b.clone() for n, b in reg.named_buffers()}

    def restore():
        with torch.no_grad():
            for n, b in reg.named_buffers():
                b.copy_(buf0[n])
    gx, g1, out1 = _taped_grad(reg, x, coef)
    buf1 = {n: b.clone() for n, b in reg.named_buffers()}
    restore()
    # the encoder half of reg(x): the same taped forward
    _, feat_taped = decisions.gpu_encoder_decisions(reg.image_encoder, x)
    restore()
    reg.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    feat = reg.image_encoder(xr)
    assert feat.requires_grad and feat.grad_fn is not None
    assert torch.equal(feat.detach(), feat_taped)
    out2 = torch.cat(reg.ief_module(feat), 1)
    (out2 * coef).sum().backward()
    assert torch.equal(out2.detach(), out1)
    assert torch.equal(xr.grad, gx)
    for n, p in reg.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, g1[n]), n
    for n, b in reg.named_buffers():
        assert torch.equal(b, buf1[n]), n       # (train: one update, num_batches_tracked + 1, like reg(x); eval: untouched)
    if train:
        assert any(not torch.equal(buf1[n], buf0[n]) for n in buf0 if n.endswith('running_mean'))
    # a standalone encoder with x not requiring grad: its parameters get gradients (they used to stay None)
    reg.zero_grad(set_to_none=True)
    restore()
    (reg.image_encoder(x) * 1.0).sum().backward()
    assert all(p.grad is not None for p in reg.image_encoder.parameters())


@pytest.mark.parametrize('train', [False, True])
def test_no_grad_forward_unchanged_by_taped_backward(dev, train):
    reg, _ = _load_det(18, dev, 'bf16x3', train)
    B = 2
    x = _proxy_input(B, 3, dev)
    with torch.no_grad():
        y0 = torch.cat(reg(x), 1).clone()
        f0 = reg.image_encoder(x).clone()
    _taped_grad(reg, x, _coef(B, dev))
    _taped_grad(reg, x, _coef(B, dev), freeze=True)
    with torch.no_grad():
        y1 = torch.cat(reg(x), 1)
        f1 = reg.image_encoder(x)
    # (training mode normalises with batch statistics: its output does not depend on the running statistics the taped runs updated)
    assert torch.equal(y0, y1) and torch.equal(f0, f1)
