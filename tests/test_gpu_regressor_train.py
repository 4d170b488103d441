"""GPU: the one-call train-mode regressor forward and backward (straps_regressor_fwd_train / _bwd, train_abi.CompositeTrainer) against
SingleInputRegressor's own autograd path (reg.train(); reg(x); torch.autograd.backward): bit-identical estimates, parameter gradients,
running statistics and input gradients over depths, precisions, batch sizes (both 1x1 routes of resnet50), channel counts, image sizes,
sparse and dense inputs and row strides; a poisoned workspace; three Adam steps; hipGraph capture; the export to the inference entry
points; and the torch-free C++ training example."""
import os
import re
import subprocess

import pytest
import torch

import straps_amd
from straps_amd import hipabi
from straps_amd.train_step import flatten_parameters

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP = straps_amd.synthetic_mean_params(0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _regressor(dev, layers, cin=18, precision='bf16x3', seed=0):
    """a regressor with randomised BatchNorm (gamma, beta, running statistics) and IEF biases, in train mode"""
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
    return reg.to(dev).train()


def _input(dev, B, cin, h=256, w=256, sparse=True, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(B, cin, h, w, generator=g)
    if sparse:      # the proxy representation: ~98 % exact zeros (the stem's skip path)
        x = torch.where(torch.rand(B, cin, h, w, generator=g) < 0.02, x, torch.zeros(()))
    return x.to(dev)


def _dest(dev, B, seed=0, ld=160):
    g = torch.Generator().manual_seed(2000 + seed)
    d = torch.zeros(B, ld)
    d[:, :157] = torch.randn(B, 157, generator=g) * 0.1
    return d.to(dev)


def _module(reg, x, dest, want_dx=False, param_grads=True):
    """the module's autograd path: (est [B,157], flat parameter gradients | None, x.grad | None)"""
    for p in reg.parameters():
        p.requires_grad_(param_grads)
        p.grad = None
    xx = x.clone().requires_grad_(want_dx)
    cam, pose, shape = reg(xx)
    est = torch.cat([cam, pose, shape], 1).detach()
    torch.autograd.backward([cam, pose, shape], [dest[:, :3], dest[:, 3:147], dest[:, 147:157]])
    grads = torch.cat([p.grad.reshape(-1) for p in reg.parameters()]) if param_grads else None
    for p in reg.parameters():
        p.requires_grad_(True)
    return est, grads, xx.grad


def _composite(tr, x, dest, want_dx=False, param_grads=True):
    cam, pose, shape = tr.forward(x)
    est = torch.cat([cam, pose, shape], 1)
    grads, dx = tr.backward(dest, want_dx=want_dx, param_grads=param_grads)
    return est, (grads.clone() if grads is not None else None), dx


def _check(reg, tr, got, want):
    for name, a, b in zip(('est', 'grads', 'dx'), got, want):
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a, b), '%s differs: max |diff| %g' % (name, float((a - b).abs().max()))
    assert torch.equal(tr.bn_state, straps_amd.flat_bn_state(reg)), 'running statistics differ'


CASES = [
    # layers, precision, batch, cin, h, w, sparse, want_dx
    (18, 'bf16x3', 2, 18, 256, 256, True, False),
    (18, 'bf16x3', 2, 18, 256, 256, True, True),
    (18, 'fp32', 2, 1, 256, 256, False, True),
    (18, 'fp32', 2, 18, 256, 256, True, False),
    (18, 'bf16x3', 3, 1, 224, 192, False, True),
    (50, 'bf16x3', 2, 18, 256, 256, True, True),       # the 1x1 layers on the plane route
    (50, 'bf16x3', 8, 18, 256, 256, True, False),      # layer1 / layer2's 1x1 layers on the fp32-operand route
    (50, 'bf16x3', 8, 1, 256, 256, False, True),
    (50, 'fp32', 2, 1, 256, 256, False, False),
]


@pytest.mark.parametrize('layers,precision,B,cin,h,w,sparse,want_dx', CASES)
def test_matches_module(dev, layers, precision, B, cin, h, w, sparse, want_dx):
    reg = _regressor(dev, layers, cin, precision)
    tr = straps_amd.CompositeTrainer(reg)
    x, dest = _input(dev, B, cin, h, w, sparse), _dest(dev, B)
    got = _composite(tr, x, dest, want_dx)
    want = _module(reg, x, dest, want_dx)
    _check(reg, tr, got, want)


@pytest.mark.parametrize('layers,precision', [(18, 'bf16x3'), (50, 'fp32')])
def test_input_gradient_without_parameter_gradients(dev, layers, precision):
    """grads == NULL: no weight-gradient kernel, the same dx (the module with every parameter frozen)"""
    reg = _regressor(dev, layers, 18, precision, seed=3)
    tr = straps_amd.CompositeTrainer(reg)
    x, dest = _input(dev, 2, 18, seed=3), _dest(dev, 2, seed=3)
    got = _composite(tr, x, dest, want_dx=True, param_grads=False)
    want = _module(reg, x, dest, want_dx=True, param_grads=False)
    _check(reg, tr, got, want)


def test_row_strides_other_than_160(dev):
    """est with ld_est 163 and dest with ld_dest 170 through the C ABI itself (columns 157.. of dest are not read)"""
    reg = _regressor(dev, 18, 18, 'bf16x3', seed=4)
    tr = straps_amd.CompositeTrainer(reg)
    B = 2
    x, dest = _input(dev, B, 18, seed=4), _dest(dev, B, seed=4)
    L = hipabi.lib()
    n = L.straps_regressor_train_workspace_bytes(tr.desc, B, 256, 256)
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    est = torch.zeros(B, 163, device=dev)
    d170 = torch.full((B, 170), float('nan'), device=dev)
    d170[:, :157] = dest[:, :157]
    grads = torch.empty_like(tr.params)
    dx = torch.empty_like(x)
    st = hipabi.stream_ptr()
    hipabi.check(L.straps_regressor_fwd_train(tr.desc, hipabi.ptr(tr.params), hipabi.ptr(tr.bn_state), hipabi.ptr(tr.init_est), hipabi.ptr(x), B, 256, 256,
                                              hipabi.ptr(est), 163, hipabi.ptr(ws), n, st), 'fwd_train')
    hipabi.check(L.straps_regressor_bwd(tr.desc, hipabi.ptr(tr.params), hipabi.ptr(x), B, 256, 256, hipabi.ptr(d170), 170, hipabi.ptr(grads), hipabi.ptr(dx),
                                        hipabi.ptr(ws), n, st), 'bwd')
    want = _module(reg, x, dest, want_dx=True)
    _check(reg, tr, (est[:, :157], grads, dx), want)
    assert torch.equal(est[:, 157:], torch.zeros(B, 6, device=dev))      # nothing past the 157 columns is written


@pytest.mark.parametrize('layers', [18, 50])
def test_poisoned_workspace(dev, layers):
    """a NaN-filled workspace before fwd_train changes nothing"""
    reg = _regressor(dev, layers, 18, 'bf16x3', seed=5)
    tr_a, tr_b = straps_amd.CompositeTrainer(reg), straps_amd.CompositeTrainer(reg)
    B = 8 if layers == 50 else 2
    x, dest = _input(dev, B, 18, seed=5), _dest(dev, B, seed=5)
    a = _composite(tr_a, x, dest, want_dx=True)
    tr_b.workspace = torch.empty(tr_b.workspace_bytes(B, 256, 256), device=dev, dtype=torch.uint8)
    tr_b.workspace.view(torch.float32).fill_(float('nan'))
    b = _composite(tr_b, x, dest, want_dx=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(tr_a.bn_state, tr_b.bn_state)


def _adam(L, flat_p, flat_g, m, v, step, lr=1e-3):
    hipabi.check(L.straps_adam_step(hipabi.ptr(flat_p), hipabi.ptr(flat_g), hipabi.ptr(m), hipabi.ptr(v), flat_p.numel(), step, lr, 0.9, 0.999, 1e-8, 1.0,
                                    None, hipabi.stream_ptr()), 'straps_adam_step')


@pytest.mark.parametrize('layers,precision,B', [(18, 'bf16x3', 2), (50, 'bf16x3', 8), (18, 'fp32', 2)])
def test_three_adam_steps(dev, layers, precision, B):
    """composite + straps_adam_step == module + the same Adam over flatten_parameters buffers, running statistics included"""
    L = hipabi.lib()
    reg = _regressor(dev, layers, 18, precision, seed=6)
    tr = straps_amd.CompositeTrainer(reg)
    params = list(reg.parameters())
    flat_p, flat_g, _ = flatten_parameters(params, dev)
    assert torch.equal(flat_p, tr.params)
    m1, v1, m2, v2 = (torch.zeros_like(flat_p) for _ in range(4))
    x = _input(dev, B, 18, seed=6)
    for step in range(1, 4):
        dest = _dest(dev, B, seed=6 + step)
        est_c, g_c, _ = _composite(tr, x, dest)
        est_m, g_m, _ = _module(reg, x, dest)
        assert torch.equal(est_c, est_m) and torch.equal(g_c, g_m), 'step %d' % step
        flat_g.copy_(g_m)
        _adam(L, flat_p, flat_g, m1, v1, step)
        _adam(L, tr.params, tr.grads, m2, v2, step)
        # the raw-pointer update bumps no tensor version: the module's packed-weight caches must be told
        reg.image_encoder._cache.clear()
        reg.ief_module._cache = {}
    assert torch.equal(flat_p, tr.params)
    assert torch.equal(tr.bn_state, straps_amd.flat_bn_state(reg))


def test_graph_capture(dev):
    """a captured fwd_train + bwd replayed twice == two eager pairs"""
    reg = _regressor(dev, 18, 18, 'bf16x3', seed=7)
    tr_e, tr_g = straps_amd.CompositeTrainer(reg), straps_amd.CompositeTrainer(reg)
    B = 2
    x, dest = _input(dev, B, 18, seed=7), _dest(dev, B, seed=7)
    bn0 = tr_g.bn_state.clone()
    eager = [_composite(tr_e, x, dest, want_dx=True) for _ in range(2)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _composite(tr_g, x, dest, want_dx=True)       # (sizes the workspace; its running-statistic update is undone below)
    torch.cuda.current_stream().wait_stream(s)
    tr_g.bn_state.copy_(bn0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cam, pose, shape = tr_g.forward(x)
        grads, dx = tr_g.backward(dest, want_dx=True)
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        est = torch.cat([cam, pose, shape], 1)
        assert torch.equal(est, eager[i][0]) and torch.equal(grads, eager[i][1]) and torch.equal(dx, eager[i][2]), 'replay %d' % i
    assert torch.equal(tr_g.bn_state, tr_e.bn_state)
    del g


@pytest.mark.parametrize('layers,precision', [(18, 'bf16x3'), (50, 'fp32')])
def test_export_to_inference(dev, layers, precision):
    """export_infer_params -> prepare -> fwd_infer == reg.eval() after write_back"""
    reg = _regressor(dev, layers, 18, precision, seed=8)
    tr = straps_amd.CompositeTrainer(reg)
    x = _input(dev, 2, 18, seed=8)
    L = hipabi.lib()
    tr.forward(x)
    grads, _ = tr.backward(_dest(dev, 2, seed=8))
    m, v = torch.zeros_like(tr.params), torch.zeros_like(tr.params)
    _adam(L, tr.params, grads, m, v, 1)
    flat = tr.export_infer_params()
    tr.write_back(reg)
    assert torch.equal(flat, straps_amd.flat_inference_params(reg))
    prepared = torch.empty(L.straps_regressor_prepared_bytes(tr.desc), device=dev, dtype=torch.uint8)
    hipabi.check(L.straps_regressor_prepare(tr.desc, hipabi.ptr(flat), hipabi.ptr(prepared), hipabi.stream_ptr()), 'prepare')
    n = L.straps_regressor_workspace_bytes(tr.desc, 2, 256, 256)
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    est = torch.empty(2, 160, device=dev)
    hipabi.check(L.straps_regressor_fwd_infer(tr.desc, hipabi.ptr(prepared), hipabi.ptr(x), 2, 256, 256, hipabi.ptr(est), 160, None, hipabi.ptr(ws), n,
                                              hipabi.stream_ptr()), 'fwd_infer')
    reg.image_encoder._cache.clear()
    reg.ief_module._cache = {}
    with torch.no_grad():
        cam, pose, shape = reg.eval()(x)
    assert torch.equal(est[:, :157], torch.cat([cam, pose, shape], 1))
    assert int(reg.image_encoder.bn1.num_batches_tracked) == 1


def test_torch_free_example(dev, tmp_path):
    """examples/regressor_train.cpp, built here and run as a child process: finite losses, the last below the first"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    exe = tmp_path / 'regressor_train'
    libdir = os.path.dirname(hipabi.LIB_PATH)
    cmd = [hipcc, '--offload-arch=gfx950', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'regressor_train.cpp'),
           '-o', str(exe), '-L', libdir, '-lstraps_hip', '-Wl,-rpath,' + libdir]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    reg = _regressor(dev, 18, 18, 'bf16x3', seed=9)
    files = {'params.bin': straps_amd.flat_training_params(reg), 'bn_state.bin': straps_amd.flat_bn_state(reg),
             'init_est.bin': reg.ief_module.initial_params_estimate}
    for name, t in files.items():
        t.detach().float().cpu().numpy().tofile(str(tmp_path / name))
    args = [str(exe), '18', '18', '3', '0', '4', '128', '128', '5'] + [str(tmp_path / k) for k in files]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    losses = [float(v) for v in re.findall(r'^step \d+ loss (\S+)$', p.stdout, re.M)]
    assert len(losses) == 5, p.stdout
    assert all(torch.isfinite(torch.tensor(losses))), losses
    assert losses[-1] < losses[0], losses
