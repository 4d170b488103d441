"""GPU: the one-call regressor inference (straps_regressor_fwd_infer / infer.InferenceRegressor) against SingleInputRegressor.eval():
bit-identical outputs over depths, precisions, batch sizes, channel counts, image sizes and inputs; the reference golden; a poisoned
workspace; one prepared buffer over many calls and refresh(); hipGraph capture; and the torch-free C++ example."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import straps_amd
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


def _regressor(dev, layers, cin=18, precision='bf16x3', seed=0):
    """a regressor with randomised BatchNorm (gamma, beta, running mean and var) in eval mode"""
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
        for fc in (reg.ief_module.fc1, reg.ief_module.fc2, reg.ief_module.fc3):
            fc.bias.copy_(torch.randn(fc.bias.shape, generator=g) * 0.01)
    reg.image_encoder.conv_precision = precision
    return reg.to(dev).eval()


def _input(dev, B, cin, h=256, w=256, sparse=True, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(B, cin, h, w, generator=g)
    if sparse:      # the proxy representation: ~98 % exact zeros (the stem's skip path)
        x = torch.where(torch.rand(B, cin, h, w, generator=g) < 0.02, x, torch.zeros(()))
    return x.to(dev)


def _module(reg, x):
    with torch.no_grad():
        cam, pose, shape = reg(x)
        rot = straps_amd.rot6d_to_rotmat(pose)
    return cam, pose, shape, rot


def _assert_same(a, b, what):
    for name, u, v in zip(('cam', 'pose', 'shape', 'rotmats'), a, b):
        assert u.shape == v.shape, (what, name, u.shape, v.shape)
        assert torch.equal(u, v), '%s: %s differs (max |d| = %.3e)' % (what, name, float((u - v).abs().max()))


@pytest.mark.parametrize('cin', [18, 1])
@pytest.mark.parametrize('precision', ['bf16x3', 'fp32'])
@pytest.mark.parametrize('layers', [18, 50])
def test_bit_identical_to_module(dev, layers, precision, cin):
    reg = _regressor(dev, layers, cin, precision, seed=layers + cin)
    ir = straps_amd.InferenceRegressor(reg)
    assert ir.precision == precision
    cases = [(B, 256, 256, sp) for B in (1, 5, 37, 64 if layers == 18 else 32) for sp in (True, False)] + [(3, 224, 224, True), (2, 224, 224, False)]
    for i, (B, h, w, sparse) in enumerate(cases):
        x = _input(dev, B, cin, h, w, sparse, seed=i)
        want = _module(reg, x)
        got = ir(x, rotmats=True)
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in got)
        _assert_same(got, want, 'r%d %s cin=%d B=%d %dx%d sparse=%s' % (layers, precision, cin, B, h, w, sparse))
        assert torch.equal(got[3], straps_amd.rot6d_to_rotmat(got[1]))


def test_precision_override(dev):
    """InferenceRegressor(reg, precision='fp32') follows the fp32 route of a module built for bf16x3"""
    reg = _regressor(dev, 18, precision='bf16x3')
    x = _input(dev, 4, 18)
    ir = straps_amd.InferenceRegressor(reg, precision='fp32')
    got = ir(x, rotmats=True)
    reg.image_encoder.conv_precision = 'fp32'
    _assert_same(got, _module(reg, x), 'fp32 override')


@pytest.mark.parametrize('layers', [18, 50])
def test_reference_golden(dev, layers):
    """the deterministic weights of test_regressor_eval_vs_reference_golden: the composite meets the reference golden at 2e-4"""
    gold = np.load(os.path.join(GOLD, 'encoder_golden.npz'))
    man = json.load(open(os.path.join(GOLD, 'state_dict_keys_r%d.json' % layers)))['keys']
    reg = straps_amd.SingleInputRegressor(18, layers, 3, mean_params=MP)
    reg.load_state_dict({k: torch.from_numpy(v) for k, v in det_state_dict(man).items()}, strict=True)
    reg = reg.to(dev).eval()
    x = torch.from_numpy(det_uniform((2, 18, 256, 256), 4242, 0.0, 1.0)).to(dev)
    cam, pose, shape = straps_amd.InferenceRegressor(reg)(x)
    out = torch.cat([cam, pose, shape], 1).cpu().double()
    ref = torch.from_numpy(gold['r%d_eval_out' % layers]).double()
    err = float(((out - ref).abs() / (2e-4 + 2e-4 * ref.abs())).max())
    assert err <= 1.0, 'composite vs golden: %.3e of the 2e-4 tolerance' % err
    _assert_same((cam, pose, shape), _module(reg, x)[:3], 'golden weights')


@pytest.mark.parametrize('precision', ['bf16x3', 'fp32'])
def test_poisoned_workspace(dev, precision):
    """NaN in every workspace byte before the call: no slot is read before it is written"""
    reg = _regressor(dev, 50, precision=precision)
    ir = straps_amd.InferenceRegressor(reg)
    x = _input(dev, 5, 18)
    want = ir(x, rotmats=True)
    want = tuple(t.clone() for t in want)
    ir.workspace.view(torch.float32).fill_(float('nan'))
    got = ir(x, rotmats=True)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in got)
    _assert_same(got, want, 'poisoned workspace')
    _assert_same(got, _module(reg, x), 'poisoned workspace vs module')


def test_one_prepared_buffer_many_calls_and_refresh(dev):
    reg = _regressor(dev, 18)
    ir = straps_amd.InferenceRegressor(reg)
    prepared = ir.prepared.data_ptr()
    xs = [_input(dev, B, 18, seed=B) for B in (64, 3, 64)]
    ws = None
    for x in xs:
        _assert_same(ir(x, rotmats=True), _module(reg, x), 'B=%d' % x.shape[0])
        ws = ws or ir.workspace.data_ptr()
    assert ir.workspace.data_ptr() == ws and ir.prepared.data_ptr() == prepared     # the B = 64 workspace served B = 3 and 64 again
    # an optimiser step changes the weights: without refresh() the composite keeps the old ones
    x = xs[1]
    old = _module(reg, x)
    opt = torch.optim.SGD(reg.parameters(), lr=0.05)
    g = torch.Generator(device=dev).manual_seed(5)
    for p in reg.parameters():
        p.grad = torch.randn(p.shape, device=dev, generator=g)
    opt.step()
    new = _module(reg, x)
    assert not torch.equal(new[0], old[0])
    stale = ir(x, rotmats=True)
    _assert_same(stale, old, 'without refresh()')
    assert not torch.equal(stale[1], new[1])
    ir.refresh()
    assert ir.prepared.data_ptr() == prepared
    _assert_same(ir(x, rotmats=True), new, 'after refresh()')


@pytest.mark.parametrize('layers', [18, 50])
def test_graph_capture(dev, layers):
    reg = _regressor(dev, layers)
    ir = straps_amd.InferenceRegressor(reg)
    B = 4
    static_x = _input(dev, B, 18, seed=1)
    ir(static_x, rotmats=True)          # warm-up: the workspace is sized outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ir(static_x, rotmats=True)
    for seed in (2, 3):
        xn = _input(dev, B, 18, sparse=seed == 2, seed=seed)
        static_x.copy_(xn)
        graph.replay()
        torch.cuda.synchronize()
        eager = ir(xn, rotmats=True)
        _assert_same(out, eager, 'graph replay %d vs eager' % seed)
        _assert_same(out, _module(reg, xn), 'graph replay %d vs module' % seed)


@pytest.mark.parametrize('layers,precision', [(18, 'bf16x3'), (50, 'fp32')])
def test_torch_free_example(dev, layers, precision, tmp_path):
    """examples/regressor_infer.cpp, built here and run as a child process, writes the module's outputs bit for bit"""
    exe = tmp_path / 'regressor_infer'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    libdir = os.path.dirname(hipabi.LIB_PATH)
    cmd = [hipcc, '--offload-arch=gfx950', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'regressor_infer.cpp'),
           '-o', str(exe), '-L', libdir, '-lstraps_hip', '-Wl,-rpath,' + libdir]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    reg = _regressor(dev, layers, precision=precision)
    B, cin, h, w = 3, 18, 256, 256
    x = _input(dev, B, cin, h, w)
    straps_amd.flat_inference_params(reg).cpu().numpy().astype(np.float32).tofile(str(tmp_path / 'params.bin'))
    x.cpu().numpy().astype(np.float32).tofile(str(tmp_path / 'input.bin'))
    args = [str(exe), str(layers), str(cin), '3', '0' if precision == 'bf16x3' else '1', str(B), str(h), str(w),
            str(tmp_path / 'params.bin'), str(tmp_path / 'input.bin'), str(tmp_path)]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    print(p.stdout.strip())
    cam, pose, shape, rot = _module(reg, x)
    est = torch.from_numpy(np.fromfile(str(tmp_path / 'est.bin'), dtype=np.float32).reshape(B, 157))
    rots = torch.from_numpy(np.fromfile(str(tmp_path / 'rotmats.bin'), dtype=np.float32).reshape(B * 24, 3, 3))
    assert torch.equal(est, torch.cat([cam, pose, shape], 1).cpu())
    assert torch.equal(rots, rot.cpu())
