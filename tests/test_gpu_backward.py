"""GPU parity tests of the gradient kernels (conv dgrad/wgrad, BatchNorm, pooling, IEF, rot6d, SMPL,
loss, Adam, input construction) against the CPU oracle / autograd of the oracle and against the golden
vectors captured from the reference (tests/golden/grad_checks_r*.json, small_golden.npz).

Tolerances: gradients are sums over up to 1e6 fp32 products in a different order than the CPU
kernels -> rel 2e-3 of the tensor's max magnitude unless stated otherwise.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import straps_amd
import straps_oracle as O
import decisions
from detgen import det_uniform, det_state_dict
from loss_cases import oracle_loss
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
MP = straps_amd.synthetic_mean_params(0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    hipabi.load()
    return torch.device('cuda:0')


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


@pytest.mark.parametrize('B,Cin,Cout,H,k,stride', [(2, 64, 64, 16, 3, 1), (2, 64, 128, 16, 3, 2), (3, 128, 64, 9, 3, 1), (2, 64, 128, 16, 1, 2),
                                                   (1, 256, 512, 8, 3, 2), (2, 256, 64, 8, 1, 1), (2, 128, 128, 15, 3, 2)])
def test_conv_dgrad_wgrad(dev, B, Cin, Cout, H, k, stride):
    L = hipabi.lib()
    pad = 1 if k == 3 else 0
    x = torch.from_numpy(det_uniform((B, Cin, H, H), 1, -1, 1)).double().requires_grad_()
    w = (torch.from_numpy(det_uniform((Cout, Cin, k, k), 2, -1, 1)) * (2.0 / (Cin * k * k)) ** 0.5).double().requires_grad_()
    y = F.conv2d(x, w, None, stride, pad)
    dy = torch.from_numpy(det_uniform(tuple(y.shape), 3, -1, 1)).double()
    y.backward(dy)
    Ho = y.shape[2]
    xd, dyd, wd = nhwc(x.detach().float(), dev), nhwc(dy.float(), dev), w.detach().float().to(dev)
    wpk = torch.empty_like(wd)
    hipabi.check(L.straps_pack_conv_weight_dgrad(hipabi.ptr(wd), hipabi.ptr(wpk), Cout, Cin, k, k, None), 'pack dgrad')
    add = torch.from_numpy(det_uniform((B, H, H, Cin), 4, -1, 1)).to(dev)
    dx = torch.empty(B, H, H, Cin, device=dev)
    hipabi.check(L.straps_conv_dgrad(hipabi.ptr(dyd), hipabi.ptr(wpk), hipabi.ptr(add), hipabi.ptr(dx), B, H, H, Cin, Cout, k, k, stride, pad, 0, None), 'dgrad')
    want = x.grad.permute(0, 2, 3, 1) + add.cpu().double()
    assert _relerr(dx, want) < 2e-5
    ws = torch.empty(L.straps_conv_wgrad_workspace_bytes(B, H, H, Cin, Cout, k, k, stride, pad) // 4, device=dev)
    dw = torch.empty_like(wd)
    hipabi.check(L.straps_conv_wgrad(hipabi.ptr(xd), hipabi.ptr(dyd), hipabi.ptr(dw), hipabi.ptr(ws), B, H, H, Cin, Cout, k, k, stride, pad, 0, None), 'wgrad')
    assert _relerr(dw, w.grad) < 2e-5
    hipabi.check(L.straps_conv_wgrad(hipabi.ptr(xd), hipabi.ptr(dyd), hipabi.ptr(dw), hipabi.ptr(ws), B, H, H, Cin, Cout, k, k, stride, pad, 1, None), 'wgrad acc')
    assert _relerr(dw, 2 * w.grad) < 2e-5


@pytest.mark.parametrize('B,Cin,Cout,H,W,k,stride', [
    (2, 128, 256, 64, 64, 1, 1),      # 128x128-tile per-tap kernel (big 1x1 layer)
    (8, 128, 128, 64, 64, 1, 2),      # the same through a strided 1x1 (down-sample branch)
    (3, 64, 64, 20, 12, 3, 2),        # non-square, 3x3/s2: incremental pixel coordinates with Wo = 6
    (2, 64, 64, 10, 24, 3, 1),        # non-square, W not a power of two: per-tap kernel for a 3x3/s1 layer
    (2, 64, 128, 12, 32, 3, 1),       # non-square through the halo-patch kernel (cw = 32, one row per chunk)
    (1, 64, 64, 4, 4, 3, 1),          # 16 pixels in all: a single partial step
    (5, 64, 64, 7, 9, 1, 1)])         # ragged pixel count (315) through the pointwise path
def test_conv_wgrad_shapes(dev, B, Cin, Cout, H, W, k, stride):
    """weight gradient on shapes outside the resnet geometry (all three kernels) vs autograd fp64."""
    L = hipabi.lib()
    pad = 1 if k == 3 else 0
    x = torch.from_numpy(det_uniform((B, Cin, H, W), 21, -1, 1)).double()
    w = (torch.from_numpy(det_uniform((Cout, Cin, k, k), 22, -1, 1)) * (2.0 / (Cin * k * k)) ** 0.5).double().requires_grad_()
    y = F.conv2d(x, w, None, stride, pad)
    dy = torch.from_numpy(det_uniform(tuple(y.shape), 23, -1, 1)).double()
    y.backward(dy)
    xd, dyd = nhwc(x.float(), dev), nhwc(dy.float(), dev)
    ws = torch.empty(L.straps_conv_wgrad_workspace_bytes(B, H, W, Cin, Cout, k, k, stride, pad) // 4, device=dev)
    dw = torch.full((Cout, Cin, k, k), float('nan'), device=dev)
    hipabi.check(L.straps_conv_wgrad(hipabi.ptr(xd), hipabi.ptr(dyd), hipabi.ptr(dw), hipabi.ptr(ws), B, H, W, Cin, Cout, k, k, stride, pad, 0, None), 'wgrad')
    assert _relerr(dw, w.grad) < 2e-5


@pytest.mark.parametrize('B,C,H,W', [(2, 18, 64, 64), (1, 1, 40, 72), (3, 18, 33, 50)])
def test_stem_wgrad(dev, B, C, H, W):
    L = hipabi.lib()
    x = torch.from_numpy(det_uniform((B, C, H, W), 6, 0, 1)).double()
    w = torch.zeros(64, C, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, 2, 3)
    dy = torch.from_numpy(det_uniform(tuple(y.shape), 7, -1, 1)).double()
    y.backward(dy)
    xd, dyd = x.float().to(dev), nhwc(dy.float(), dev)
    ws = torch.empty(L.straps_stem_wgrad_workspace_bytes(B, C, H, W) // 4, device=dev)
    dw = torch.empty(64, C, 7, 7, device=dev)
    hipabi.check(L.straps_stem_wgrad(hipabi.ptr(xd), hipabi.ptr(dyd), hipabi.ptr(dw), hipabi.ptr(ws), None, B, C, H, W, 0, None), 'stem wgrad')
    assert _relerr(dw, w.grad) < 2e-5


def test_stem_wgrad_zero_skipping_is_exact(dev):
    """proxy-like input (mostly exact zeros): probing, mask-driven and skip-defeated runs agree (the first two bit for bit)."""
    L = hipabi.lib()
    B, C, H, W = 3, 18, 96, 128
    x = torch.zeros(B, C, H, W)
    blob = torch.from_numpy(det_uniform((B, C, 16, 16), 40, 0.1, 1.0))
    for b in range(B):
        for c in range(C):
            if (b + c) % 5 == 4:
                continue                                   # some channels stay entirely zero
            y0, x0 = (7 * c + 13 * b) % (H - 16), (11 * c + 5 * b) % (W - 16)
            x[b, c, y0:y0 + 16, x0:x0 + 16] = blob[b, c]
    x[:, 0, 20:80, 40:90] = 1.0                            # silhouette-like channel
    w = torch.zeros(64, C, 7, 7, dtype=torch.float64, requires_grad=True)
    yref = F.conv2d(x.double(), w, None, 2, 3)
    dy = torch.from_numpy(det_uniform(tuple(yref.shape), 41, -1, 1))
    yref.backward(dy.double())
    xd, dyd = x.to(dev), nhwc(dy, dev)
    ws = torch.empty(L.straps_stem_wgrad_workspace_bytes(B, C, H, W) // 4, device=dev)
    mask = torch.empty(L.straps_stem_nzmask_words(B, C, H, W), device=dev, dtype=torch.int32)
    hipabi.check(L.straps_stem_nzmask(hipabi.ptr(xd), hipabi.ptr(mask), B, C, H, W, None), 'nzmask')
    outs = []
    for inp, m in ((xd, None), (xd, mask), (torch.where(xd == 0, torch.full_like(xd, 1e-30), xd), None)):
        dw = torch.empty(64, C, 7, 7, device=dev)
        hipabi.check(L.straps_stem_wgrad(hipabi.ptr(inp), hipabi.ptr(dyd), hipabi.ptr(dw), hipabi.ptr(ws), hipabi.ptr(m), B, C, H, W, 0, None), 'stem wgrad')
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])
    assert float((outs[0] - outs[2]).abs().max()) < 1e-20          # nothing skipped vs skipped: only the 1e-30 fill differs
    assert _relerr(outs[0], w.grad) < 2e-5


@pytest.mark.parametrize('C,relu,B,H', [(64, True, 3, 7), (512, True, 3, 7), (2048, False, 3, 7), (128, False, 3, 7),
                                        # rows % 4 == 0 and C % 256 == 0: the tiled form of the apply pass (4 rows x 256 channels per trip)
                                        (256, True, 2, 6), (512, True, 4, 8), (2048, False, 1, 4), (1024, True, 5, 10)])
def test_bn_backward(dev, C, relu, B, H):
    L = hipabi.lib()
    rows = B * H * H
    x = torch.from_numpy(det_uniform((B, C, H, H), 8, -1, 1)).double().requires_grad_()
    g = torch.from_numpy(det_uniform((C,), 9, 0.5, 1.5)).double().requires_grad_()
    b = torch.from_numpy(det_uniform((C,), 10, -0.5, 0.5)).double().requires_grad_()
    y = F.batch_norm(x, None, None, g, b, True, 0.1, 1e-5)
    out = F.relu(y) if relu else y
    dy = torch.from_numpy(det_uniform(tuple(y.shape), 11, -1, 1)).double()
    out.backward(dy)
    xs = x.detach()
    mean = xs.mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(xs.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    raw, dyd, outd = nhwc(xs.float(), dev), nhwc(dy.float(), dev), nhwc(out.detach().float(), dev)
    md, isd, gd = mean.float().to(dev), invstd.float().to(dev), g.detach().float().to(dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    draw, dz = torch.empty_like(raw), torch.empty_like(raw)
    ws = torch.empty(L.straps_bn_bwd_workspace_bytes(rows, C) // 4, device=dev)
    hipabi.check(L.straps_bn_bwd(hipabi.ptr(dyd), hipabi.ptr(outd if relu else None), hipabi.ptr(raw), hipabi.ptr(md), hipabi.ptr(isd), hipabi.ptr(gd),
                                 None, None, hipabi.ptr(dg), hipabi.ptr(db), hipabi.ptr(draw), hipabi.ptr(dz), hipabi.ptr(ws), rows, C, 0, None), 'bn bwd')
    assert _relerr(draw.permute(0, 3, 1, 2), x.grad) < 5e-5
    assert _relerr(dg, g.grad) < 5e-5 and _relerr(db, b.grad) < 5e-5
    mask = (out.detach() > 0).double() if relu else torch.ones_like(dy)
    assert _relerr(dz.permute(0, 3, 1, 2), dy * mask) < 1e-6
    if relu:
        # mask re-derived from raw with the forward's scale / shift == mask read from the forward's own activation, bit for bit
        sc = gd * isd
        sh = b.detach().float().to(dev) - md * sc
        act = torch.empty_like(raw)
        hipabi.check(L.straps_bn_apply(hipabi.ptr(raw), hipabi.ptr(sc), hipabi.ptr(sh), None, 1, hipabi.ptr(act), rows, C, None), 'bn apply')
        outs = []
        for kw in ((act, None, None), (None, sc, sh)):
            dg2, db2, draw2, dz2 = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty_like(raw), torch.empty_like(raw)
            hipabi.check(L.straps_bn_bwd(hipabi.ptr(dyd), hipabi.ptr(kw[0]), hipabi.ptr(raw), hipabi.ptr(md), hipabi.ptr(isd), hipabi.ptr(gd),
                                         hipabi.ptr(kw[1]), hipabi.ptr(kw[2]), hipabi.ptr(dg2), hipabi.ptr(db2), hipabi.ptr(draw2), hipabi.ptr(dz2),
                                         hipabi.ptr(ws), rows, C, 0, None), 'bn bwd')
            outs.append((dg2, db2, draw2, dz2))
        for u, v in zip(*outs):
            assert torch.equal(u, v)
        assert _relerr(outs[1][2].permute(0, 3, 1, 2), x.grad) < 5e-5


def test_maxpool_and_gap_backward(dev):
    L = hipabi.lib()
    B, C, H, W = 2, 64, 17, 22
    # ReLU-like input with many exact ties at zero (the arg-max rule matters)
    x = F.relu(torch.from_numpy(det_uniform((B, C, H, W), 12, -1, 1))).requires_grad_()
    y = F.max_pool2d(x, 3, 2, 1)
    dy = torch.from_numpy(det_uniform(tuple(y.shape), 13, -1, 1))
    y.backward(dy)
    xd, dyd = nhwc(x.detach(), dev), nhwc(dy, dev)
    yd = torch.empty(B, y.shape[2], y.shape[3], C, device=dev)
    idx = torch.empty(B, y.shape[2], y.shape[3], C, device=dev, dtype=torch.uint8)
    hipabi.check(L.straps_maxpool_fwd_idx(hipabi.ptr(xd), hipabi.ptr(yd), hipabi.ptr(idx), B, H, W, C, None), 'maxpool idx')
    assert torch.equal(yd.permute(0, 3, 1, 2).cpu(), y.detach())
    dx = torch.empty_like(xd)
    hipabi.check(L.straps_maxpool_bwd(hipabi.ptr(dyd), hipabi.ptr(idx), hipabi.ptr(dx), B, H, W, C, None), 'maxpool bwd')
    assert _relerr(dx.permute(0, 3, 1, 2), x.grad) < 1e-6
    df = torch.from_numpy(det_uniform((B, C), 14, -1, 1)).to(dev)
    dg = torch.empty(B, H * W, C, device=dev)
    hipabi.check(L.straps_gap_bwd(hipabi.ptr(df), hipabi.ptr(dg), B, H * W, C, None), 'gap bwd')
    assert _relerr(dg, (df / (H * W))[:, None, :].expand(B, H * W, C)) < 1e-6


def test_rot6d_backward(dev):
    x = torch.from_numpy(det_uniform((5, 144), 15, -1.5, 1.5))
    xo = x.clone().double().requires_grad_()
    R = O.rot6d_to_rotmat(xo)
    g = torch.from_numpy(det_uniform((120, 3, 3), 16, -1, 1))
    R.backward(g.double())
    xg = x.to(dev).requires_grad_()
    Rg = straps_amd.rot6d_to_rotmat(xg)
    Rg.backward(g.to(dev))
    assert _relerr(xg.grad, xo.grad) < 2e-5


def _load_det(reg, layers, dev):
    man = json.load(open(os.path.join(GOLD, 'state_dict_keys_r%d.json' % layers)))['keys']
    sd = {k: torch.from_numpy(v) for k, v in det_state_dict(man).items()}
    reg.load_state_dict(sd, strict=True)
    return reg.to(dev), sd


def test_gemm_multi_vs_float64(dev):
    """straps_gemm_multi: eight problems of different shapes and stride patterns in one launch (transposed A, stacked K, a constant-one A =
    column sums, ragged M / N / K), every epilogue feature (addend, mask, accumulate, second accumulating output), against float64."""
    L = hipabi.lib()
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    B, H, P, F_ = 37, 96, 157, 72
    dh = r(3, B, H).to(dev)
    h1 = r(3, B, H).to(dev)
    est = r(4, B, 160).to(dev)
    feat = r(B, F_).to(dev)
    w = r(H, H).to(dev)
    w3 = r(P, H).to(dev)
    mask = r(B, H).to(dev)
    add = r(B, 160).to(dev)
    one = torch.ones(4, device=dev)
    dW2, dW1, dW3, y1, y2, y2b, cs, cs2 = (torch.full(sh, float('nan'), device=dev) for sh in
                                          ((H, H), (H, F_ + P), (P, H), (B, H), (B, 160), (B, H), (H,), (P,)))
    y2b = r(B, H).to(dev)
    y2b0 = y2b.clone()
    acc0 = r(B, H).to(dev)
    y1.copy_(acc0)
    D = hipabi.gemm_desc
    hipabi.gemm_multi([
        D(dh, 1, H, h1, H, 1, dW2, H, H, H, 3 * B),                                        # dh^T h1 over the three stacked blocks
        D(dh[0], 1, H, feat, F_, 1, dW1, F_ + P, H, F_, B),                                 # into a column block of a wider matrix
        D(dh, 1, H, est, 160, 1, dW1.data_ptr() + 4 * F_, F_ + P, H, P, 3 * B),             # the other column block, ragged N = 157
        D(est[1], 1, 160, h1, H, 1, dW3, H, P, H, 3 * B),                                   # ragged M = 157
        D(dh[1], H, 1, w, H, 1, y1, H, B, H, H, accumulate=1, mask=mask, ldmask=H, c2=y2b, ldc2=H, accumulate2=1),
        D(dh[2], H, 1, w3, 1, H, y2, 160, B, P, H, addend=add, ldadd=160),                  # B(k, n) = w3[n][k]
        D(one, 0, 0, dh, H, 1, cs, H, 1, H, 3 * B),                                         # column sums
        D(one, 0, 0, est[1], 160, 1, cs2, P, 1, P, 3 * B)])
    torch.cuda.synchronize()
    d64 = lambda t: t.double().cpu()
    dhf, h1f, estf = d64(dh).reshape(3 * B, H), d64(h1).reshape(3 * B, H), d64(est)

    def close(got, want, name):
        err = float((d64(got) - want).abs().max() / want.abs().max())
        assert err < 2e-6, '%s: %.3e' % (name, err)
    close(dW2, dhf.T @ h1f, 'dW2')
    close(dW1[:, :F_], d64(dh[0]).T @ d64(feat), 'dW1 feature block')
    close(dW1[:, F_:], dhf.T @ estf[:3].reshape(3 * B, 160)[:, :P], 'dW1 estimate block')
    close(dW3, estf[1:].reshape(3 * B, 160)[:, :P].T @ h1f, 'dW3')
    v = (d64(dh[1]) @ d64(w)) * (d64(mask) > 0)
    close(y1, d64(acc0) + v, 'masked accumulate')
    close(y2b, d64(y2b0) + v, 'second output')
    close(y2[:, :P], d64(dh[2]) @ d64(w3).T + d64(add)[:, :P], 'addend')
    assert torch.isnan(y2[:, P:]).all()                                                    # columns beyond N stay untouched
    close(cs, dhf.sum(0), 'column sums')
    close(cs2, estf[1:].reshape(3 * B, 160)[:, :P].sum(0), 'column sums (ragged)')
    assert L.straps_gemm_multi(None, 1, None) != 0


@pytest.mark.parametrize('layers,F_', [(18, 512), (50, 2048)])
def test_ief_backward_vs_oracle_autograd(dev, layers, F_):
    reg, sd = _load_det(straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP), layers, dev)
    feat = torch.from_numpy(det_uniform((5, F_), 31, 0.0, 2.0))
    coef = torch.from_numpy(det_uniform((5, 157), 32, -1, 1))
    names = ['ief_module.fc%d.%s' % (i, t) for i in (1, 2, 3) for t in ('weight', 'bias')]
    sdo = {k: v.clone().double() for k, v in sd.items() if k.startswith('ief_module.')}
    for n in names:
        sdo[n].requires_grad_()
    fo = feat.clone().double().requires_grad_()
    _, _, _, est = O.ief_forward(fo, sdo, O.ief_init_estimate(MP['pose'], MP['shape']).double(), 3)
    (est * coef.double()).sum().backward()
    fg = feat.to(dev).requires_grad_()
    cam, pose, shape = reg.ief_module(fg)
    (torch.cat([cam, pose, shape], 1) * coef.to(dev)).sum().backward()
    assert _relerr(fg.grad, fo.grad) < 5e-5
    for n in names:
        p = dict(reg.named_parameters())[n]
        assert _relerr(p.grad, sdo[n].grad) < 5e-5, n


@pytest.mark.parametrize('layers', [18, 50])
def test_regressor_param_grads_vs_reference_golden(dev, layers):
    """loss.backward() through encoder + IEF (training-mode BatchNorm) against the parameter gradients the
    reference itself produced (oracle/make_golden.py, grad_checks_r*.json)."""
    gold = json.load(open(os.path.join(GOLD, 'grad_checks_r%d.json' % layers)))
    reg, sd = _load_det(straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP), layers, dev)
    reg.train()
    x = torch.from_numpy(det_uniform((2, 18, 256, 256), 4242, 0.0, 1.0)).to(dev)
    coef = torch.from_numpy(det_uniform((2, 157), 555)).to(dev)
    cam, pose, shape = reg(x)
    (torch.cat([cam, pose, shape], 1) * coef).sum().backward()
    # This B=2 training-mode problem is ill-conditioned: on the CPU the SAME graph in fp64 differs from the reference's
    # fp32 result by 0.24 % in gradient norm and up to 8 % in single elements (ReLU masks / batch statistics of 2
    # samples amplify round-off).  Every kernel is checked tightly on its own above; this end-to-end test guards the
    # wiring: norms within 1 % (resnet50: 2 % -- which way its tied ReLU decisions fall moves single tensors by 1.1 %, and that changes with the
    # summation order of a tile choice) of the reference golden, direction (cosine) vs the oracle's autograd >= 0.995 (measured: r18 0.99992, r50 0.9989 worst tensor).
    # What these loose bars hide is pinned below on the GPU's own decisions.
    sdo = {k: v.clone() for k, v in sd.items()}
    names = [n for n, _ in reg.named_parameters()]
    for n in names:
        sdo[n].requires_grad_(True)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    _, _, _, est = O.regressor_forward(x.cpu(), sdo, O.ief_init_estimate(MP['pose'], MP['shape']), layers, 3, training=True)
    (est * coef.cpu()).sum().backward()
    worst, worst_cos = 0.0, 1.0
    for n, p in reg.named_parameters():
        ref_norm, ref_head = gold[n]
        assert p.grad is not None, n
        g = p.grad.cpu().double().reshape(-1)
        go = sdo[n].grad.double().reshape(-1)
        err = abs(float(g.norm()) - ref_norm) / max(ref_norm, 1e-12)
        cos = float((g @ go) / (g.norm() * go.norm()).clamp_min(1e-30))
        worst, worst_cos = max(worst, err), min(worst_cos, cos)
        assert err < (1e-2 if layers == 18 else 2e-2), '%s: grad norm %.6e vs reference %.6e' % (n, float(g.norm()), ref_norm)
        assert cos > 0.995, '%s: cosine vs oracle autograd %.6f' % (n, cos)
    print('r%d worst grad-norm rel err %.2e, worst cosine %.6f' % (layers, worst, worst_cos))
    # ... and what those loose bars hide is decisions, not arithmetic: the float64 oracle evaluated on the ReLU / max-pool decisions the
    # GPU took (tests/decisions.py; every differing decision a tie) agrees with the GPU's gradients to 2e-4 (resnet50: 1e-3) relative L2 in every tensor
    reg.zero_grad()
    dec, feat = decisions.gpu_encoder_decisions(reg.image_encoder, x)          # (a second training-mode forward: same batch statistics)
    masks = decisions.gpu_ief_masks(reg.ief_module, feat)
    cam, pose, shape = reg(x)
    (torch.cat([cam, pose, shape], 1) * coef).sum().backward()
    rec64 = {'record': True}
    sd64 = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    O.regressor_forward(x.cpu().double(), sd64, O.ief_init_estimate(MP['pose'], MP['shape']).double(), layers, 3, training=True, enc_decisions=rec64)
    # (training-mode BatchNorm over a batch of TWO bodies: the statistics of 2 x H x W samples amplify the evaluation error of the deep resnet50
    #  layers -- measured 2.1e-4 of the layer's largest pre-activation on its worst layer, 1e-5 for resnet18; the whole-step tests at 8 .. 64 bodies
    #  keep the tighter caps of tests/decisions.py)
    n_relu, n_pool, tie_relu, tie_pool, act_err = decisions.compare_encoder_decisions(dec, rec64, decisions.ERR_CAP if layers == 18 else 1e-3)
    assert tie_relu <= 4.0 and tie_pool <= 4.0
    sd64 = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for n in names:
        sd64[n].requires_grad_(True)
    _, _, _, est = O.regressor_forward(x.cpu().double(), sd64, O.ief_init_estimate(MP['pose'], MP['shape']).double(), layers, 3, training=True,
                                       ief_masks=masks, enc_decisions={'relu': dec['relu'], 'pool': dec['pool']})
    (est * coef.cpu().double()).sum().backward()
    worst = 0.0
    for n, p in reg.named_parameters():
        r = sd64[n].grad.reshape(-1)
        e = float((p.grad.cpu().double().reshape(-1) - r).norm() / r.norm().clamp_min(1e-30))
        worst = max(worst, e)
        assert e < (2e-4 if layers == 18 else 1e-3), '%s: %.3e vs the float64 oracle on the GPU decisions' % (n, e)      # (measured: 2.0e-5 / 2.0e-4 worst; two samples per batch statistic)
    print('r%d: %d ReLU / %d pooling decisions differ from float64 (ties); worst relative gradient error on the GPU decisions %.2e' % (layers, n_relu, n_pool, worst))


@pytest.mark.parametrize('layers,prec', [(18, 'bf16x3'), (18, 'fp32'), (50, 'bf16x3')])
def test_eval_mode_gradients_through_frozen_batchnorm_vs_float64_oracle(dev, layers, prec):
    """reg.eval() + loss.backward(): nn.BatchNorm2d in eval mode back-propagates through its running statistics as constants
    (models/resnet.py:47,147; fine-tuning with frozen statistics).  Eval mode is well conditioned (no batch statistics), so the bars are
    tight: outputs 2e-5, every parameter gradient (incl. BatchNorm weight / bias) 2e-4 (resnet50: 5e-4) of the tensor's maximum against autograd of the
    float64 oracle with training=False -- evaluated on the GPU's ReLU / max-pool decisions where a rounding-level tie was decided the other
    way (tests/decisions.py); running statistics and num_batches_tracked untouched; the no-grad eval output unchanged by the taped run."""
    reg, sd = _load_det(straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP), layers, dev)
    reg.image_encoder.conv_precision = prec
    reg.eval()
    B = 3
    x = torch.from_numpy(det_uniform((B, 18, 256, 256), 4343, 0.0, 1.0)).to(dev)
    x[:, 1:, ::2] = 0.0
    coef = torch.from_numpy(det_uniform((B, 157), 556)).to(dev)
    with torch.no_grad():
        y0 = torch.cat(reg(x), 1).clone()
    buf0 = {n: b.clone() for n, b in reg.named_buffers()}
    cam, pose, shape = reg(x)
    y1 = torch.cat([cam, pose, shape], 1)
    (y1 * coef).sum().backward()
    assert float((y1.detach() - y0).abs().max()) < 2e-5
    for n, b in reg.named_buffers():
        assert torch.equal(b, buf0[n]), n
    names = [n for n, _ in reg.named_parameters()]
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    init = O.ief_init_estimate(MP['pose'], MP['shape'])

    def oracle(dtype, **kw):
        sdo = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        for n in names:
            sdo[n].requires_grad_(True)
        _, _, _, est = O.regressor_forward(x.cpu().to(dtype), sdo, init.to(dtype), layers, 3, training=False, **kw)
        (est * coef.cpu().to(dtype)).sum().backward()
        return est.detach(), {n: sdo[n].grad for n in names}
    rec64, taps64 = {'record': True}, []
    est, g64 = oracle(torch.float64, enc_decisions=rec64, ief_taps=taps64)
    assert float((y1.detach().cpu().double() - est).abs().max()) < 2e-4
    # the decisions the GPU took (taped forward = the forward of the backward above), unit by unit against float64's
    dec, feat = decisions.gpu_encoder_decisions(reg.image_encoder, x)
    masks = decisions.gpu_ief_masks(reg.ief_module, feat)
    n_relu, n_pool, tie_relu, tie_pool, act_err = decisions.compare_encoder_decisions(dec, rec64, decisions.ERR_CAP if layers == 18 else decisions.ERR_CAP_R50)
    n_ief = sum(int((m != (z > 0)).sum()) for pair, zs in zip(masks, taps64) for m, z in zip(pair, zs))
    total_units = sum(m.numel() for m in dec['relu'])
    print('eval-mode r%d %s: %d of %d encoder ReLU decisions, %d of %d pooling windows and %d IEF ReLU decisions differ from float64 '
          '(|z64| / float64 gap of the differing ones: <= %.2f x / %.2f x the activation error observed on the same layer)'
          % (layers, prec, n_relu, total_units, n_pool, dec['pool'].numel(), n_ief, tie_relu, tie_pool))
    # every differing decision is a TIE: the float64 pre-activation (gap between the window's two candidates) lies within a few times the
    # evaluation error measured on the units of the same layer that both sides agree on.  One such unit moves a whole term of every
    # gradient upstream of it (measured on this input with tools/debug_eval_stem2.py: ONE of the stem's 786 432 pooling windows,
    # candidates 1.323754461 / 1.323754109, moves conv1.weight by 2.4e-3 of its maximum while every other tensor sits at 1e-5), so the
    # gradients are compared with the float64 oracle evaluating the function the GPU did differentiate: the GPU's decisions forced.
    assert tie_relu <= 4.0 and tie_pool <= 4.0
    assert n_relu <= 1e-5 * total_units + 3
    if n_relu or n_pool or n_ief:
        _, g64 = oracle(torch.float64, enc_decisions={'relu': dec['relu'], 'pool': dec['pool']}, ief_masks=masks)
    worst, bad = 0.0, []
    for n, p in reg.named_parameters():
        assert p.grad is not None, n
        err = _relerr(p.grad, g64[n])
        worst = max(worst, err)
        if not err < (2e-4 if layers == 18 else 5e-4):          # (measured: 2.1e-5 / 1.3e-6 resnet18 bf16x3 / fp32, 2.5e-4 resnet50 bf16x3)
            bad.append('%s: %.3e' % (n, err))
    print('eval-mode r%d %s: worst max-norm relative gradient error vs float64 (GPU decisions): %.2e over %d tensors' % (layers, prec, worst, len(names)))
    assert not bad, '\n'.join(bad)


def test_fused_stem_tail_equals_unfused(dev):
    """bn1 + relu + maxpool fused (straps_bn_relu_maxpool_fwd / straps_bn_bwd_pooled: the stem activation and its gradient are
    never materialised) against the unfused calls (straps_bn_apply, straps_maxpool_fwd_idx, straps_maxpool_bwd, straps_bn_bwd):
    same arithmetic in the same order, so features, running statistics and every parameter gradient behind the stem agree bit for
    bit (the stem's own three gradients to 1e-5: see below); also an odd-sized input (pool windows clipped at the border)."""
    for shape in ((3, 18, 256, 256), (2, 18, 120, 88)):
        outs = []
        for unfused in (False, True):
            reg, _ = _load_det(straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP), 18, dev)
            reg.train()
            reg.image_encoder.unfused_stem_tail = unfused
            x = torch.from_numpy(det_uniform(shape, 77, 0.0, 1.0)).to(dev)
            x[:, 1:, ::3] = 0.0
            coef = torch.from_numpy(det_uniform((shape[0], 157), 78)).to(dev)
            cam, pose, shp = reg(x)
            (torch.cat([cam, pose, shp], 1) * coef).sum().backward()
            outs.append((torch.cat([cam, pose, shp], 1).detach().clone(), {n: p.grad.clone() for n, p in reg.named_parameters()},
                         {n: b.clone() for n, b in reg.named_buffers()}))
        (ya, ga, ba), (yb, gb, bb) = outs
        assert torch.equal(ya, yb)
        for n in ga:
            if n in ('image_encoder.conv1.weight', 'image_encoder.bn1.weight', 'image_encoder.bn1.bias'):
                # the fused tail takes bn1's two backward sums over the POOLED grid (one term per pooled element, in double) instead of
                # over the un-pooled gradient: the same numbers in another summation order
                err = float((ga[n] - gb[n]).abs().max() / gb[n].abs().max().clamp_min(1e-30))
                assert err < 1e-5, (n, err)
            else:
                assert torch.equal(ga[n], gb[n]), n
        for n in ba:
            assert torch.equal(ba[n], bb[n]), n


@pytest.mark.parametrize('layers', [18, 50])
def test_relu_bits_backward_equals_the_fp32_mask_backward(dev, layers):
    """ABI 8 (encoder_exec._RELU_BITS): a residual unit's ReLU decisions travel to the backward pass as bits -- the last BatchNorm's two
    passes, the sums fused into the data gradient that feeds it and the skip connection's share of the gradient read 1 / 32 of the bytes, and
    the masked copy dz of the gradient is never written.  Nothing else changes: outputs, running statistics and EVERY parameter gradient of
    the regressor are bit-identical with the switch off (the fp32-mask entry points of rounds 1-3).  Basic blocks with and without a
    downsample branch (resnet18), bottlenecks (resnet50)."""
    from straps_amd import encoder_exec
    outs = []
    rows0 = encoder_exec.X3F_MIN_ROWS
    try:
        # (a statement about the plane kernels' two mask forms: the fp32-operand route of the long 1x1 layers -- round 6 -- has bit forms only, and its lean
        #  epilogue pre-sums 16 values in fp32, so it is switched off for both runs; its own parity: tests/test_gpu_conv_x3f.py)
        encoder_exec.X3F_MIN_ROWS = 0
        for on in (True, False):
            encoder_exec._RELU_BITS = on
            reg, _ = _load_det(straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP), layers, dev)
            reg.train()
            x = torch.from_numpy(det_uniform((3, 18, 128, 96), 81, 0.0, 1.0)).to(dev)
            coef = torch.from_numpy(det_uniform((3, 157), 82)).to(dev)
            cam, pose, shp = reg(x)
            (torch.cat([cam, pose, shp], 1) * coef).sum().backward()
            outs.append((torch.cat([cam, pose, shp], 1).detach().clone(), {n: p.grad.clone() for n, p in reg.named_parameters()},
                         {n: b.clone() for n, b in reg.named_buffers()}))
    finally:
        encoder_exec._RELU_BITS = True
        encoder_exec.X3F_MIN_ROWS = rows0
    (ya, ga, ba), (yb, gb, bb) = outs
    assert torch.equal(ya, yb)
    assert all(bool(torch.isfinite(g).all()) for g in ga.values())
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    for n in ba:
        assert torch.equal(ba[n], bb[n]), n


def test_sparse_stem_tail_writes_only_what_the_weight_gradient_reads(dev):
    """straps_bn_bwd_pooled_sparse on a proxy-like input (a silhouette box + a few heat-map blobs, whole channels empty): the tiles
    straps_stem_tile_activity marks are written bit for bit as by the dense call, the others are left untouched, dgamma / dbeta are the
    dense call's -- and through the module the stem's weight gradient equals the unfused route's (1e-5 of its maximum, the bar of
    test_fused_stem_tail_equals_unfused), every other gradient bit for bit."""
    L = hipabi.lib()
    B, C, H, W = 3, 18, 256, 256
    x = torch.zeros(B, C, H, W)
    dense = torch.from_numpy(det_uniform((B, C, H, W), 91, 0.1, 1.0))
    x[:, 0, 60:200, 90:170] = dense[:, 0, 60:200, 90:170]                     # silhouette
    for j in range(1, 9):                                                     # heat-map blobs; channels 9..17 stay empty
        x[:, j, 20 * j:20 * j + 16, 25 * j:25 * j + 16] = dense[:, j, 20 * j:20 * j + 16, 25 * j:25 * j + 16]
    x = x.to(dev)
    nz = torch.empty(L.straps_stem_nzmask_words(B, C, H, W), device=dev, dtype=torch.int32)
    hipabi.check(L.straps_stem_nzmask(hipabi.ptr(x), hipabi.ptr(nz), B, C, H, W, None), 'nzmask')
    nt = L.straps_stem_tiles(B, H, W)
    assert nt == B * 64 * 4
    act = torch.full((nt,), 7, device=dev, dtype=torch.uint8)
    hipabi.check(L.straps_stem_tile_activity(hipabi.ptr(nz), hipabi.ptr(act), B, C, H, W, None), 'tile activity')
    # the map against its definition: any non-zero in input rows 4ty-3 .. 4ty+5, columns 64tx-3 .. 64tx+68 (bit-map granularity: 4-row
    # cells x 8-column bytes, so the kernel's patch is that rectangle widened to whole cells -- a superset, never a subset)
    anynz = (x != 0).any(1).float()[:, None]
    exact = torch.nn.functional.max_pool2d(torch.nn.functional.pad(anynz, (3, 5, 3, 5)), (9, 72), (4, 64)).reshape(-1) > 0
    wide = torch.nn.functional.max_pool2d(torch.nn.functional.pad(anynz, (11, 13, 7, 9)), (17, 88), (4, 64)).reshape(-1) > 0
    a = act.bool()
    assert bool((a | ~exact).all()) and bool((~a | wide).all())
    assert 0.2 < float(a.float().mean()) < 0.8
    # kernel level: sparse call == dense call on the marked tiles, untouched elsewhere
    Ho, Wo, Cc = 128, 128, 64
    raw = torch.from_numpy(det_uniform((B, Ho, Wo, Cc), 92, -1, 1)).to(dev)
    mean = torch.from_numpy(det_uniform((Cc,), 93, -0.1, 0.1)).to(dev)
    invstd = torch.from_numpy(det_uniform((Cc,), 94, 0.5, 2.0)).to(dev)
    gamma = torch.from_numpy(det_uniform((Cc,), 95, 0.5, 1.5)).to(dev)
    msc, msh = (gamma * invstd).contiguous(), (-mean * gamma * invstd + 0.05).contiguous()
    y = torch.relu(raw * msc + msh)
    yp = torch.empty(B, 64, 64, Cc, device=dev)
    idx = torch.empty(B, 64, 64, Cc, device=dev, dtype=torch.uint8)
    hipabi.check(L.straps_maxpool_fwd_idx(hipabi.ptr(y), hipabi.ptr(yp), hipabi.ptr(idx), B, Ho, Wo, Cc, None), 'maxpool')
    dyp = torch.from_numpy(det_uniform((B, 64, 64, Cc), 96, -1, 1)).to(dev)
    ws = torch.empty(L.straps_bn_bwd_workspace_bytes(B * Ho * Wo, Cc) // 4, device=dev)
    res = []
    for tact in (None, act):
        dg, db = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
        draw = torch.full((B, Ho, Wo, Cc), float('nan'), device=dev)
        hipabi.check(L.straps_bn_bwd_pooled_sparse(hipabi.ptr(dyp), hipabi.ptr(idx), hipabi.ptr(raw), hipabi.ptr(mean), hipabi.ptr(invstd),
                                                   hipabi.ptr(gamma), hipabi.ptr(msc), hipabi.ptr(msh), hipabi.ptr(dg), hipabi.ptr(db),
                                                   hipabi.ptr(draw), hipabi.ptr(ws), B, Ho, Wo, Cc, 0, hipabi.ptr(tact), None), 'bn_bwd_pooled_sparse')
        torch.cuda.synchronize()
        res.append((dg, db, draw))
    (dg0, db0, d0), (dg1, db1, d1) = res
    assert torch.equal(dg0, dg1) and torch.equal(db0, db1) and not bool(torch.isnan(d0).any())
    m = act.view(B, 64, 1, 4, 1, 1).expand(B, 64, 2, 4, 32, Cc).reshape(B, Ho, Wo, Cc).bool()
    assert torch.equal(d1[m], d0[m]) and bool(torch.isnan(d1[~m]).all())
    # module level: the fused (sparse) tail against the unfused calls
    outs = []
    for unfused in (False, True):
        reg, _ = _load_det(straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP), 18, dev)
        reg.train()
        reg.image_encoder.unfused_stem_tail = unfused
        coef = torch.from_numpy(det_uniform((B, 157), 97)).to(dev)
        cam, pose, shp = reg(x)
        (torch.cat([cam, pose, shp], 1) * coef).sum().backward()
        outs.append({n: p.grad.clone() for n, p in reg.named_parameters()})
    ga, gb = outs
    for n in ga:
        if n in ('image_encoder.conv1.weight', 'image_encoder.bn1.weight', 'image_encoder.bn1.bias'):
            err = float((ga[n] - gb[n]).abs().max() / gb[n].abs().max().clamp_min(1e-30))
            assert err < 1e-5, (n, err)
        else:
            assert torch.equal(ga[n], gb[n]), n


def test_smpl_backward_vs_oracle_autograd(dev):
    model = straps_amd.synthetic_smpl_model(0)
    for B in (3, 37):
        smpl = straps_amd.SMPL(model, batch_size=B).to(dev)
        betas = torch.from_numpy(det_uniform((B, 10), 40 + B, -2, 2))
        aa = torch.from_numpy(det_uniform((B, 72), 41 + B, -0.8, 0.8))
        R = O.batch_rodrigues(aa.reshape(-1, 3)).view(B, 24, 3, 3)
        gv = torch.from_numpy(det_uniform((B, 6890, 3), 42, -1, 1))
        gj = torch.from_numpy(det_uniform((B, 90, 3), 43, -1, 1))
        bo, Ro = betas.double().requires_grad_(), R.double().requires_grad_()
        v, j = O.smpl_forward(model, bo, rotmats=Ro, dtype=torch.float64)
        ((v * gv.double()).sum() + (j * gj.double()).sum()).backward()
        bg, Rg = betas.to(dev).requires_grad_(), R.to(dev).requires_grad_()
        out = smpl(body_pose=Rg[:, 1:], global_orient=Rg[:, 0:1], betas=bg, pose2rot=False)
        ((out.vertices * gv.to(dev)).sum() + (out.joints * gj.to(dev)).sum()).backward()
        assert _relerr(bg.grad, bo.grad) < 1e-4, 'dbetas B=%d' % B
        assert _relerr(Rg.grad, Ro.grad) < 1e-4, 'drotmats B=%d' % B
    # joints-only and verts-only gradients (NULL inputs)
    bg, Rg = betas.to(dev).requires_grad_(), R.to(dev).requires_grad_()
    out = smpl(body_pose=Rg[:, 1:], global_orient=Rg[:, 0:1], betas=bg, pose2rot=False)
    (out.joints * gj.to(dev)).sum().backward()
    bo.grad = None; Ro.grad = None
    v, j = O.smpl_forward(model, bo, rotmats=Ro, dtype=torch.float64)
    (j * gj.double()).sum().backward()
    assert _relerr(bg.grad, bo.grad) < 1e-4 and _relerr(Rg.grad, Ro.grad) < 1e-4


def test_criterion_module_vs_reference_golden(dev):
    small = np.load(os.path.join(GOLD, 'small_golden.npz'))
    ck = json.load(open(os.path.join(GOLD, 'criterion_keys.json')))
    B = 4
    w = {'verts': 1.0, 'joints2D': 0.1, 'pose_params': 0.1, 'shape_params': 0.1, 'joints3D': 1.0}
    crit = straps_amd.HomoscedasticUncertaintyWeightedMultiTaskLoss(['verts', 'shape_params', 'pose_params', 'joints2D', 'joints3D'],
                                                                   init_loss_weights=w, reduction='mean').to(dev)
    assert list(crit.state_dict().keys()) == list(ck['keys'].keys())
    assert [n for n, _ in crit.named_parameters()] == ck['param_order']
    for k, v in ck['keys'].items():
        assert float(crit.state_dict()[k]) == pytest.approx(v, rel=1e-6)
    lab = {'verts': torch.from_numpy(det_uniform((B, 6890, 3), 40)), 'joints2D': torch.from_numpy(det_uniform((B, 17, 2), 41, -40.0, 300.0)),
           'joints3D': torch.from_numpy(det_uniform((B, 14, 3), 42)), 'shape_params': torch.from_numpy(det_uniform((B, 10), 43, -2, 2)),
           'pose_params_rot_matrices': torch.from_numpy(det_uniform((B, 24, 3, 3), 44))}
    lab['vis'] = O.check_joints2d_visibility(lab['joints2D'])
    lab = {k: v.to(dev) for k, v in lab.items()}
    outp = {'verts': torch.from_numpy(det_uniform((B, 6890, 3), 45)), 'joints2D': torch.from_numpy(det_uniform((B, 17, 2), 46)),
            'joints3D': torch.from_numpy(det_uniform((B, 14, 3), 47)), 'shape_params': torch.from_numpy(det_uniform((B, 10), 48, -2, 2)),
            'pose_params_rot_matrices': torch.from_numpy(det_uniform((B, 24, 3, 3), 49))}
    outp = {k: v.to(dev).requires_grad_() for k, v in outp.items()}
    total, parts = crit(lab, outp)
    total.backward()
    assert float(total) == pytest.approx(float(small['loss_total']), rel=2e-5)
    order = ('verts', 'joints2D', 'joints3D', 'shape_params', 'pose_params')
    np.testing.assert_allclose([float(parts[k]) for k in order], small['loss_parts'], rtol=2e-5)
    np.testing.assert_allclose([float(getattr(crit, k + '_log_var').grad) for k in order], small['loss_grad_logvars'], rtol=2e-5)
    np.testing.assert_allclose(outp['joints2D'].grad.cpu().numpy(), small['loss_grad_j2d'], rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(outp['shape_params'].grad.cpu().numpy(), small['loss_grad_shape'], rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(outp['verts'].grad.reshape(-1)[:64].cpu().numpy(), small['loss_grad_verts_head'], rtol=1e-4, atol=1e-10)
    np.testing.assert_allclose(outp['joints3D'].grad.cpu().numpy(), small['loss_grad_j3d'], rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(outp['pose_params_rot_matrices'].grad.reshape(-1)[:64].cpu().numpy(), small['loss_grad_pose_head'], rtol=1e-4, atol=1e-10)
    # reduction='sum' (constructor contract, losses/multi_task_loss.py:13-17)
    crit_s = straps_amd.HomoscedasticUncertaintyWeightedMultiTaskLoss(['verts', 'shape_params', 'pose_params', 'joints2D', 'joints3D'],
                                                                     init_loss_weights=w, reduction='sum').to(dev)
    for v_ in outp.values():
        v_.grad = None
    total_s, parts_s = crit_s(lab, outp)
    total_s.backward()
    assert float(total_s) == pytest.approx(float(small['loss_sum_total']), rel=2e-5)
    np.testing.assert_allclose([float(parts_s[k]) for k in order], small['loss_sum_parts'], rtol=2e-5)
    np.testing.assert_allclose([float(getattr(crit_s, k + '_log_var').grad) for k in order], small['loss_sum_grad_logvars'], rtol=2e-5)
    np.testing.assert_allclose(outp['joints2D'].grad.cpu().numpy(), small['loss_sum_grad_j2d'], rtol=1e-4, atol=1e-8)
    with pytest.raises(AssertionError):
        straps_amd.HomoscedasticUncertaintyWeightedMultiTaskLoss(['verts'], reduction='max')


def test_fused_loss_vs_oracle(dev):
    """straps_loss_fwd_bwd (heads + 5 losses + gradients in one call) vs the oracle composed with autograd."""
    L = hipabi.lib()
    B = 6
    joints = torch.from_numpy(det_uniform((B, 90, 3), 60, -1, 1))
    est = torch.zeros(B, 160)
    est[:, :157] = torch.from_numpy(det_uniform((B, 157), 61, -1, 1))
    est[:, 0] = est[:, 0].abs() + 0.5
    prot = torch.from_numpy(det_uniform((B, 24, 3, 3), 62))
    pverts = torch.from_numpy(det_uniform((B, 6890, 3), 63))
    tverts = torch.from_numpy(det_uniform((B, 6890, 3), 64))
    tj2d = torch.from_numpy(det_uniform((B, 17, 2), 65, -40.0, 300.0))
    tj3d = torch.from_numpy(det_uniform((B, 14, 3), 66))
    tshape = torch.from_numpy(det_uniform((B, 10), 67, -2, 2))
    trot = torch.from_numpy(det_uniform((B, 24, 3, 3), 68))
    lv0 = O.init_log_vars({'verts': 1.0, 'joints2D': 0.1, 'pose_params': 0.1, 'shape_params': 0.1, 'joints3D': 1.0})
    order = ('verts', 'joints2D', 'joints3D', 'shape_params', 'pose_params')
    # oracle with autograd (the composition shared with tests/test_gpu_loss_head_edges.py)
    total, parts, lab, leaf, lv = oracle_loss(joints, est, prot, pverts, tverts, tj2d, tj3d, tshape, trot, lv0)
    J, E, PR, PV = leaf['J'], leaf['E'], leaf['PR'], leaf['PV']
    d = lambda t: t.to(dev).contiguous()
    tens = [d(pverts), d(joints), d(est), d(prot), d(tverts), d(tj2d), d(tj3d), d(tshape), d(trot)]
    lvd = torch.tensor([lv0[k] for k in order], dtype=torch.float32, device=dev)
    loss = torch.empty(12, device=dev)
    dv, dj, de, dr, dl = torch.empty(B, 6890, 3, device=dev), torch.empty(B, 90, 3, device=dev), torch.empty(B, 160, device=dev), torch.empty(B, 24, 3, 3, device=dev), torch.empty(5, device=dev)
    ws = torch.empty(L.straps_loss_workspace_bytes(B) // 4, device=dev)
    hipabi.check(L.straps_loss_fwd_bwd(hipabi.ptr(tens[0]), hipabi.ptr(tens[1]), hipabi.ptr(tens[2]), 160, hipabi.ptr(tens[3]), hipabi.ptr(tens[4]),
                                       hipabi.ptr(tens[5]), hipabi.ptr(tens[6]), hipabi.ptr(tens[7]), hipabi.ptr(tens[8]), hipabi.ptr(lvd), hipabi.ptr(loss),
                                       hipabi.ptr(dv), hipabi.ptr(dj), hipabi.ptr(de), hipabi.ptr(dr), hipabi.ptr(dl), hipabi.ptr(ws), B, 256, None), 'loss')
    lo = loss.cpu()
    assert float(lo[0]) == pytest.approx(float(total), rel=2e-5)
    np.testing.assert_allclose(lo[1:6].numpy(), [float(parts[k]) for k in order], rtol=2e-5)
    assert int(lo[11]) == int(lab['vis'].sum())
    np.testing.assert_allclose(dl.cpu().numpy(), [float(lv[k].grad) for k in order], rtol=2e-5)
    assert _relerr(dv, PV.grad) < 1e-5 and _relerr(dj, J.grad) < 1e-5 and _relerr(dr, PR.grad) < 1e-5
    assert _relerr(de, E.grad) < 1e-5


def test_global_masked_mean_loss_two_virtual_ranks_equal_the_global_batch(dev):
    """straps_loss_fwd_bwd_gm + straps_count_visible (data parallel with the GLOBAL visibility-masked mean): a batch of 6 bodies split over
    two "ranks" of 3 with very different numbers of visible joints.  Each half evaluated with the job-wide count (scaled by 1 / world):
    the AVERAGE of the two ranks' losses, log-variance gradients and head gradients -- what the step's sum all-reduce + 1 / world
    computes -- equals the single-process result on the 6-body batch (float64 oracle), which the per-rank masked means do not."""
    L = hipabi.lib()
    B, Bh = 6, 3
    joints = torch.from_numpy(det_uniform((B, 90, 3), 60, -1, 1))
    est = torch.zeros(B, 160)
    est[:, :157] = torch.from_numpy(det_uniform((B, 157), 61, -1, 1))
    est[:, 0] = est[:, 0].abs() + 0.5
    prot = torch.from_numpy(det_uniform((B, 24, 3, 3), 62))
    pverts = torch.from_numpy(det_uniform((B, 6890, 3), 63))
    tverts = torch.from_numpy(det_uniform((B, 6890, 3), 64))
    tj2d = torch.from_numpy(det_uniform((B, 17, 2), 65, 20.0, 230.0))
    tj2d[Bh:, :13] = 300.0                                    # the second rank sees 4 joints per body, the first all 17
    tj3d = torch.from_numpy(det_uniform((B, 14, 3), 66))
    tshape = torch.from_numpy(det_uniform((B, 10), 67, -2, 2))
    trot = torch.from_numpy(det_uniform((B, 24, 3, 3), 68))
    lv0 = O.init_log_vars({'verts': 1.0, 'joints2D': 0.1, 'pose_params': 0.1, 'shape_params': 0.1, 'joints3D': 1.0})
    order = ('verts', 'joints2D', 'joints3D', 'shape_params', 'pose_params')
    J, E = joints.double().requires_grad_(), est.double().requires_grad_()
    lv = {k: torch.tensor(lv0[k], dtype=torch.float64, requires_grad=True) for k in order}
    outp = {'verts': pverts.double(), 'joints2D': O.orthographic_project(J[:, O.ALL_JOINTS_TO_COCO_MAP], E[:, :3]),
            'joints3D': J[:, O.ALL_JOINTS_TO_H36M_MAP][:, O.H36M_TO_J14], 'shape_params': E[:, 147:157], 'pose_params_rot_matrices': prot.double()}
    lab = {'verts': tverts.double(), 'joints2D': tj2d.double(), 'joints3D': tj3d.double(), 'shape_params': tshape.double(),
           'pose_params_rot_matrices': trot.double(), 'vis': O.check_joints2d_visibility(tj2d)}
    total, parts = O.multi_task_loss(lab, outp, lv)
    total.backward()
    d = lambda t: t.to(dev).contiguous()
    lvd = torch.tensor([lv0[k] for k in order], dtype=torch.float32, device=dev)

    def rank(sl, count_dev, scale):
        n = sl.stop - sl.start
        t = [d(pverts[sl]), d(joints[sl]), d(est[sl]), d(prot[sl]), d(tverts[sl]), d(tj2d[sl]), d(tj3d[sl]), d(tshape[sl]), d(trot[sl])]
        loss = torch.empty(12, device=dev)
        dv, dj, de, dr, dl = (torch.empty(n, 6890, 3, device=dev), torch.empty(n, 90, 3, device=dev), torch.empty(n, 160, device=dev),
                              torch.empty(n, 24, 3, 3, device=dev), torch.empty(5, device=dev))
        ws = torch.empty(L.straps_loss_workspace_bytes(n) // 4, device=dev)
        hipabi.check(L.straps_loss_fwd_bwd_gm(hipabi.ptr(t[0]), hipabi.ptr(t[1]), hipabi.ptr(t[2]), 160, hipabi.ptr(t[3]), hipabi.ptr(t[4]), hipabi.ptr(t[5]),
                                              hipabi.ptr(t[6]), hipabi.ptr(t[7]), hipabi.ptr(t[8]), hipabi.ptr(lvd), hipabi.ptr(loss), hipabi.ptr(dv), hipabi.ptr(dj),
                                              hipabi.ptr(de), hipabi.ptr(dr), hipabi.ptr(dl), hipabi.ptr(ws), n, 256, hipabi.ptr(count_dev), scale, None), 'loss_gm')
        return loss.cpu().double(), dl.cpu().double(), dj.cpu().double(), de.cpu().double()
    # every rank counts its own visible joints; the sum is what the all-reduce delivers
    counts = []
    for sl in (slice(0, Bh), slice(Bh, B)):
        c = torch.zeros(1, device=dev)
        hipabi.check(L.straps_count_visible(hipabi.ptr(d(tj2d[sl])), hipabi.ptr(c), Bh, 17, 256, None), 'count')
        counts.append(float(c))
    assert counts == [51.0, 12.0] and sum(counts) == float(lab['vis'].sum())
    glob = torch.tensor([sum(counts)], device=dev)
    r0, r1 = rank(slice(0, Bh), glob, 0.5), rank(slice(Bh, B), glob, 0.5)
    mean = [(a + b) / 2 for a, b in zip(r0, r1)]
    # joints2D: weighted task loss (slot 2), its log-variance gradient, the head gradients of the camera / the COCO joints
    assert float(mean[0][2]) == pytest.approx(float(parts['joints2D']), rel=2e-5)
    assert float(mean[1][1]) == pytest.approx(float(lv['joints2D'].grad), rel=2e-5)
    got_dj = torch.cat([r0[2], r1[2]]) / 2                      # each body's gradient lives on one rank; the exchange averages over ranks
    got_de = torch.cat([r0[3], r1[3]]) / 2
    # (the other tasks are plain per-rank means of equal-sized halves: their rank average is the global mean as well)
    assert _relerr(got_dj, J.grad) < 1e-5 and _relerr(got_de, E.grad) < 1e-5
    assert float(mean[0][0]) == pytest.approx(float(total), rel=2e-5)
    # without the global count the same average is NOT the global masked mean (rank 1's few joints weigh as much as rank 0's many)
    p0, p1 = rank(slice(0, Bh), None, 1.0), rank(slice(Bh, B), None, 1.0)
    assert abs(float((p0[0][2] + p1[0][2]) / 2) - float(parts['joints2D'])) > 1e-3 * float(parts['joints2D'])


def test_build_proxy_input_vs_reference_golden(dev):
    small = np.load(os.path.join(GOLD, 'small_golden.npz'))
    jh = torch.from_numpy(small['heat_in']).to(dev)
    hm = straps_amd.label_conversions.convert_2Djoints_to_gaussian_heatmaps_torch(jh, 256)
    flat = hm.reshape(-1).cpu()
    nz = flat.nonzero().squeeze(1).numpy()
    assert np.array_equal(nz, small['heat_nz_idx'])
    np.testing.assert_allclose(flat[nz].numpy(), small['heat_nz_val'], rtol=2e-6, atol=1e-7)
    seg = (torch.from_numpy(det_uniform((2, 256, 256), 38, 0.0, 1.0)) > 0.7).float() * torch.from_numpy(np.floor(det_uniform((2, 256, 256), 39, 1.0, 6.999)))
    x = straps_amd.label_conversions.build_proxy_input(seg.to(dev), jh)
    assert x.shape == (2, 18, 256, 256)
    assert float(x[:, 0].sum()) == float(small['binary_sum'])
    assert torch.equal(x[:, 1:], hm)


@pytest.mark.parametrize('B,NJ,WH,std', [(3, 17, 256, 4), (2, 5, 264, 4), (2, 17, 64, 2), (1, 3, 520, 8)])
def test_build_proxy_input_with_nonzero_map_equals_the_two_passes(dev, B, NJ, WH, std):
    """straps_build_proxy_input_nz (round 4: the training step's input and the stem's non-zero bit map in ONE pass, cells outside a joint's
    window written without evaluating the Gaussian) against straps_build_proxy_input_std followed by straps_stem_nzmask: the same planes and
    the same words, bit for bit.  Joints inside, on every border, in the corners, outside the image and negative (the truncation toward
    zero of .int()); sizes whose last mask word is partial (264, 520) and a small one (64)."""
    L = hipabi.lib()
    j = torch.from_numpy(det_uniform((B, NJ, 2), 41, -12.0, WH + 12.0))
    edge = [(0.0, 0.0), (WH - 1.0, WH - 1.0), (0.4, WH - 0.6), (WH - 1.0, 3.0), (-0.9, 17.2), (WH + 7.9, 40.0), (2 * std - 1.0, 2 * std + 0.0), (-2.0 * std, 50.0),
            (WH - 2.0 * std, WH / 2.0), (WH + 2.0 * std - 1.0, 9.0)]
    for k, (ex, ey) in enumerate(edge):
        j[k % B, k % NJ] = torch.tensor([ex, ey])
    seg = ((torch.from_numpy(det_uniform((B, WH, WH), 42, 0.0, 1.0)) > 0.9).float() * torch.from_numpy(np.floor(det_uniform((B, WH, WH), 43, 1.0, 6.999))))
    seg[:, : WH // 2, : WH // 3] = 0.0              # whole cells and words of the silhouette empty
    seg, j = seg.to(dev), j.to(dev)
    x0 = torch.full((B, NJ + 1, WH, WH), float('nan'), device=dev)
    x1 = torch.full((B, NJ + 1, WH, WH), float('nan'), device=dev)
    nw = L.straps_stem_nzmask_words(B, NJ + 1, WH, WH)
    m0 = torch.full((nw,), 0x5a5a5a5a, device=dev, dtype=torch.int32)
    m1 = torch.full((nw,), 0x5a5a5a5a, device=dev, dtype=torch.int32)
    hipabi.check(L.straps_build_proxy_input_std(hipabi.ptr(seg), hipabi.ptr(j), hipabi.ptr(x0), B, NJ, WH, std, None), 'build_proxy_input_std')
    hipabi.check(L.straps_stem_nzmask(hipabi.ptr(x0), hipabi.ptr(m0), B, NJ + 1, WH, WH, None), 'stem_nzmask')
    hipabi.check(L.straps_build_proxy_input_nz(hipabi.ptr(seg), hipabi.ptr(j), hipabi.ptr(x1), hipabi.ptr(m1), B, NJ, WH, std, None), 'build_proxy_input_nz')
    assert torch.equal(x0, x1)
    assert torch.equal(m0, m1)
    assert 0 < int((x0[:, 1:] != 0).sum()) and int((m0 != 0).sum()) < nw      # some heat-maps drawn, some words empty
    assert L.straps_build_proxy_input_nz(hipabi.ptr(seg), hipabi.ptr(j), hipabi.ptr(x1), hipabi.ptr(m1), B, NJ, WH + 4, std, None) == 1      # wh % 8


def test_adam_vs_reference_golden(dev):
    small = np.load(os.path.join(GOLD, 'small_golden.npz'))
    man = json.load(open(os.path.join(GOLD, 'state_dict_keys_r18.json')))
    sd = {k: torch.from_numpy(v) for k, v in det_state_dict(man['keys']).items()}
    ps = [sd[n].clone() for n in man['param_order']] + [torch.zeros(()) for _ in range(5)]
    grads = [torch.from_numpy(det_uniform(tuple(p.shape), 9000 + i, -1e-2, 1e-2)).reshape(p.shape) for i, p in enumerate(ps)]
    flat_p = torch.cat([p.reshape(-1) for p in ps]).to(dev)
    flat_g = torch.cat([g.reshape(-1) for g in grads]).to(dev)
    before = flat_p.clone()
    m, v = torch.zeros_like(flat_p), torch.zeros_like(flat_p)
    L = hipabi.lib()
    for step in (1, 2):
        hipabi.check(L.straps_adam_step(hipabi.ptr(flat_p), hipabi.ptr(flat_g), hipabi.ptr(m), hipabi.ptr(v), flat_p.numel(), step, 1e-4, 0.9, 0.999, 1e-8, 1.0, None, None), 'adam')
    delta = (flat_p - before).cpu().double()
    off = 0
    ds, da = [], []
    for p in ps:
        n = p.numel()
        ds.append(float(delta[off:off + n].sum()))
        da.append(float(delta[off:off + n].abs().sum()))
        off += n
    np.testing.assert_allclose(da, small['adam_delta_abs'], rtol=1e-4)
    np.testing.assert_allclose(ds, small['adam_delta_sum'], rtol=2e-3, atol=1e-6)


@pytest.mark.parametrize('layers,operand_bn', [(50, True), (50, False), (18, True)])
def test_fp32_operand_route_equals_the_plane_route(dev, layers, operand_bn):
    """round 6 (csrc/conv_x3f.hip, conv_wgrad_x3f.hip; encoder_exec.x3f_mode): the long 1x1 layers read the fp32 tensors -- forward with the producer's
    BatchNorm in the operand path, data gradient with the lean epilogue, weight gradient from fp32 operands -- instead of bf16 planes.  Same arithmetic
    (three bf16 parts per value, six products per term): the forward outputs agree to rounding of the batch statistics' partial sums (other block
    shapes), every parameter gradient to 2e-4 of its norm (bar of the whole-step float64 tests for resnet50: tests/test_gpu_train_step.py)."""
    from straps_amd import encoder_exec
    outs = []
    rows0, bn0 = encoder_exec.X3F_MIN_ROWS, encoder_exec.X3F_OPERAND_BN
    try:
        encoder_exec.X3F_OPERAND_BN = operand_bn
        for rows in (1024, 0):          # (every 1x1 layer from 1024 pixel rows on: layer1-3 of this batch; 0 = the plane route everywhere)
            encoder_exec.X3F_MIN_ROWS = rows
            reg, _ = _load_det(straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP), layers, dev)
            reg.train()
            x = torch.from_numpy(det_uniform((4, 18, 256, 256), 83, 0.0, 1.0)).to(dev)
            coef = torch.from_numpy(det_uniform((4, 157), 84)).to(dev)
            cam, pose, shp = reg(x)
            (torch.cat([cam, pose, shp], 1) * coef).sum().backward()
            outs.append((torch.cat([cam, pose, shp], 1).detach().clone(), {n: p.grad.clone() for n, p in reg.named_parameters()}))
    finally:
        encoder_exec.X3F_MIN_ROWS, encoder_exec.X3F_OPERAND_BN = rows0, bn0
    (ya, ga), (yb, gb) = outs
    assert torch.allclose(ya, yb, rtol=2e-5, atol=2e-5), (ya - yb).abs().max().item()
    # The two routes compute the same products, but their batch statistics are summed over other block shapes (1e-7 relative), so a pre-activation that
    # sits within rounding of zero may be decided the other way -- and one flipped ReLU decision moves the encoder gradients upstream of it by its whole
    # term (1e-3 ... 1e-2 per tensor between ANY two fp32 evaluations; the whole-step tests of tests/test_gpu_train_step.py compare both
    # routes with float64 ON the GPU's decisions, to 2e-4).  Here: the head's gradients (no decision between them and the loss differs) to 1e-4, every
    # encoder tensor in direction (cosine >= 0.999) and size (5e-2).
    for n in ga:
        a, b = ga[n].double().flatten(), gb[n].double().flatten()
        assert torch.isfinite(a).all(), n
        rel = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
        if n.startswith('ief_module'):
            assert rel <= 1e-4, '%s: %.3e' % (n, rel)
        else:
            cos = (torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30)).item()
            assert cos >= 0.999 and rel <= 5e-2, '%s: rel %.3e cos %.6f' % (n, rel, cos)
