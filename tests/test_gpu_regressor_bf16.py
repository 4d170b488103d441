"""GPU: the single-product bf16 route end to end -- ResNet(conv_precision='bf16') under .eval() / torch.no_grad() and the one-call composite
(straps_regressor_fwd_infer, precision 3) bit-identical to each other (also on a NaN-filled workspace and replayed from a captured graph); the
estimates' accuracy against the float64 oracle within the bound derived from the CPU model of the route; the refusals (train mode, grad mode,
TrainStep, CompositeTrainer) before any launch; and the default route untouched by a detour through 'bf16'."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import straps_amd
import straps_oracle as O
from bf16x3_emul import bf16_bits_to_f32, bf16_rn_bits
from detgen import det_state_dict, det_uniform
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
MP = straps_amd.synthetic_mean_params(0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _regressor(dev, layers, cin=18, precision='bf16', seed=0):
    torch.manual_seed(seed)
    reg = straps_amd.SingleInputRegressor(cin, layers, 3, mean_params=MP)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in reg.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.weight.shape[0]
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
    reg.image_encoder.conv_precision = precision
    return reg.to(dev).eval()


def _input(dev, B, cin, h=256, w=256, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(B, cin, h, w, generator=g)
    return torch.where(torch.rand(B, cin, h, w, generator=g) < 0.02, x, torch.zeros(())).to(dev)


def _module(reg, x):
    with torch.no_grad():
        cam, pose, shape = reg(x)
        return cam, pose, shape, straps_amd.rot6d_to_rotmat(pose)


def _same(a, b, what):
    for name, u, v in zip(('cam', 'pose', 'shape', 'rotmats'), a, b):
        assert torch.equal(u, v), '%s: %s differs (max |d| = %.3e)' % (what, name, float((u - v).abs().max()))


@pytest.mark.parametrize('cin', [18, 1])
@pytest.mark.parametrize('layers', [18, 50])
def test_module_and_composite_bit_identical(dev, layers, cin):
    reg = _regressor(dev, layers, cin, seed=layers + cin)
    ir = straps_amd.InferenceRegressor(reg)
    assert ir.precision == 'bf16' and ir.desc.precision == 3
    for i, (B, h, w) in enumerate([(1, 256, 256), (5, 256, 256), (64, 256, 256), (3, 224, 192)]):
        x = _input(dev, B, cin, h, w, seed=i)
        want = _module(reg, x)
        got = ir(x, rotmats=True)
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in got)
        _same(got, want, 'r%d cin=%d B=%d %dx%d' % (layers, cin, B, h, w))


@pytest.mark.parametrize('layers', [18, 50])
def test_poisoned_workspace_and_graph_replay(dev, layers):
    reg = _regressor(dev, layers, seed=3)
    ir = straps_amd.InferenceRegressor(reg, precision='bf16')
    x = _input(dev, 5, 18, seed=11)
    want = _module(reg, x)
    ir(x)
    ir.workspace.view(torch.float32).fill_(float('nan'))
    _same(ir(x, rotmats=True), want, 'NaN-filled workspace')
    # captured: the module and the composite, replayed on new input data
    static_x = x.clone()
    for name, fn in (('module', lambda: _module(reg, static_x)), ('composite', lambda: ir(static_x, rotmats=True))):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn()
        x2 = _input(dev, 5, 18, seed=12)
        static_x.copy_(x2)
        g.replay()
        torch.cuda.synchronize()
        _same(out, _module(reg, x2), '%s graph replay' % name)
        static_x.copy_(x)


class _Bf16Conv:
    """torch.nn.functional with conv2d on rn_bf16 operands for every 3x3 / 1x1 convolution (the stem, 7x7, stays exact): the CPU model of the route"""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def conv2d(x, w, b=None, stride=1, padding=0):
        if w.shape[-1] != 7:
            rn = lambda t: torch.from_numpy(bf16_bits_to_f32(bf16_rn_bits(t.float().numpy())).astype(np.float64))  # noqa: E731
            x, w = rn(x).to(x.dtype), rn(w).to(w.dtype)
        return F.conv2d(x, w, b, stride, padding)


def _oracle(x, sd, layers, emulate):
    sd64 = {k: v.double() for k, v in sd.items()}
    init = O.ief_init_estimate(MP['pose'], MP['shape']).double()
    keep = O.F
    try:
        if emulate:
            O.F = _Bf16Conv()
        cam, pose, shape, _ = O.regressor_forward(x.double(), sd64, init, layers, 3, False)
    finally:
        O.F = keep
    return torch.cat([cam, pose, shape], 1)


def _verts_mm(model, est):
    """SMPL vertices (mm, float64 oracle) of estimates [B, 157]"""
    R = O.rot6d_to_rotmat(est[:, 3:147].double().contiguous()).view(-1, 24, 3, 3)
    v, _ = O.smpl_forward(model, est[:, 147:157].double(), rotmats=R, dtype=torch.float64)
    return v * 1000.0


@pytest.mark.parametrize('weights', ['golden', 'random'])
@pytest.mark.parametrize('layers', [18, 50])
def test_accuracy_within_the_modelled_bound(dev, layers, weights):
    """Bound: the CPU model of the route (float64 network, every 3x3 / 1x1 convolution on rn_bf16 operands) has an error e_model against the
    float64 network on the same input; the GPU route differs from the model by fp32 accumulation and the bf16 rounding decisions it flips --
    a perturbation of the same size or smaller, so |bf16 - float64| <= 2 e_model + 2e-4 (2e-4: the fp32 route's own bar against the golden
    outputs, test_gpu_regressor_infer.py).  The SMPL vertices of the bf16 estimates against the fp32-class (bf16x3) route's in mm: the same
    rule on the vertices of the model's estimates (+ 0.1 mm)."""
    if weights == 'golden':
        man = json.load(open(os.path.join(GOLD, 'state_dict_keys_r%d.json' % layers)))['keys']
        reg = straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP)
        reg.load_state_dict({k: torch.from_numpy(v) for k, v in det_state_dict(man).items()}, strict=True)
        reg = reg.to(dev).eval()
        x = torch.from_numpy(det_uniform((2, 18, 256, 256), 4242, 0.0, 1.0)).to(dev)
    else:
        reg = _regressor(dev, layers, seed=40 + layers, precision='bf16x3')
        x = _input(dev, 2, 18, seed=41)
    sd = {k: v.detach().cpu() for k, v in reg.state_dict().items()}
    reg.image_encoder.conv_precision = 'bf16x3'
    ref_x3 = torch.cat(_module(reg, x)[:3], 1).cpu().double()
    reg.image_encoder.conv_precision = 'bf16'
    got = torch.cat(_module(reg, x)[:3], 1).cpu().double()
    exact = _oracle(x.cpu(), sd, layers, False)
    model = _oracle(x.cpu(), sd, layers, True)
    e_model = float((model - exact).abs().max())
    e_gpu = float((got - exact).abs().max())
    smpl = straps_amd.synthetic_smpl_model(0)
    dv = float((_verts_mm(smpl, got) - _verts_mm(smpl, ref_x3)).abs().max())
    dv_model = float((_verts_mm(smpl, model) - _verts_mm(smpl, exact)).abs().max())
    print('\nr%d %s: |bf16 - f64| max %.3e mean %.3e  model %.3e  bf16x3 %.3e;  vertices vs bf16x3 max %.3f mm (model %.3f mm)' % (
        layers, weights, e_gpu, float((got - exact).abs().mean()), e_model, float((ref_x3 - exact).abs().max()), dv, dv_model))
    assert torch.isfinite(got).all()
    assert e_gpu <= 2 * e_model + 2e-4, (e_gpu, e_model)
    assert dv <= 2 * dv_model + 0.1, (dv, dv_model)


def _launch_counter(monkeypatch):
    """counts calls into the library's convolution / stem entry points: a refusal must come before any of them"""
    L = hipabi.lib()
    calls = []
    for name in ('straps_stem_fwd', 'straps_stem_nzmask', 'straps_conv_fwd_bf16', 'straps_split_bf16_cm', 'straps_conv_fwd_x3', 'straps_conv_fwd'):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _n=name: (calls.append(_n), _fn(*a))[1])
    return calls


def test_refusals_before_any_launch(dev, monkeypatch):
    reg = _regressor(dev, 18, seed=5)
    x = _input(dev, 2, 18)
    calls = _launch_counter(monkeypatch)
    with pytest.raises(RuntimeError, match='no_grad'):
        reg(x)                                           # grad mode, parameters require grad
    with pytest.raises(RuntimeError, match='no_grad'):
        reg.image_encoder(x)
    with torch.no_grad():
        reg.train()
        with pytest.raises(RuntimeError, match='conv_precision'):
            reg(x)
        with pytest.raises(RuntimeError, match='conv_precision'):
            reg.image_encoder(x)
        reg.eval()
    for p in reg.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match='no_grad'):
        reg(x.clone().requires_grad_(True))              # an input that requires grad
    assert calls == []
    for p in reg.parameters():
        p.requires_grad_(True)
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=2).to(dev)
    crit = straps_amd.HomoscedasticUncertaintyWeightedMultiTaskLoss(['verts', 'shape_params', 'pose_params', 'joints2D', 'joints3D']).to(dev)
    from straps_amd.train_step import TrainStep
    with pytest.raises(RuntimeError, match='conv_precision'):
        TrainStep(reg, smpl, crit, 2, mean_shape=MP['shape'])
    from straps_amd.train_abi import CompositeTrainer
    with pytest.raises(RuntimeError, match='bf16'):
        CompositeTrainer(reg)
    assert calls == []
    with torch.no_grad():
        reg(x)
    assert 'straps_conv_fwd_bf16' in calls and 'straps_conv_fwd_x3' not in calls


@pytest.mark.parametrize('layers', [18, 50])
def test_default_route_unchanged_by_a_bf16_detour(dev, layers):
    """bf16x3 outputs are bit-identical before and after a bf16 forward of the same module, and equal to a twin that never left bf16x3:
    no cached pack or plane leaks between the routes"""
    a = _regressor(dev, layers, seed=8, precision='bf16x3')
    b = _regressor(dev, layers, seed=8, precision='bf16x3')
    x = _input(dev, 3, 18, seed=9)
    before = _module(a, x)
    a.image_encoder.conv_precision = 'bf16'
    low = _module(a, x)
    assert not torch.equal(low[1], before[1])            # (the detour did run the other route)
    a.image_encoder.conv_precision = 'bf16x3'
    _same(_module(a, x), before, 'after the detour')
    _same(_module(b, x), before, 'twin')
    ir = straps_amd.InferenceRegressor(a)
    assert ir.precision == 'bf16x3'
    _same(ir(x, rotmats=True), before, 'composite after the detour')
