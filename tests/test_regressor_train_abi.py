"""CPU: the train-mode regressor entry points (straps_regressor_fwd_train / _bwd / export_infer_params) -- parameter and running-
statistic layouts, argument validation and workspace sizing are host code, checkable without a GPU; the torch-free training example
compiles against the header."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import straps_amd
from straps_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
P = 8192        # a non-null, never dereferenced address


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _desc(layers=50, cin=18, iters=3, precision=0):
    return hipabi.RegressorDesc(layers, cin, iters, precision)


def _err(lib):
    return lib.straps_last_error().decode()


@pytest.mark.parametrize('layers', [18, 50])
@pytest.mark.parametrize('cin', [1, 18])
def test_sizes_match_module(lib, layers, cin):
    reg = straps_amd.SingleInputRegressor(cin, layers, 3, mean_params=straps_amd.synthetic_mean_params(0))
    bns = [m for m in reg.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for precision in (0, 1):
        d = _desc(layers, cin, 3, precision)
        assert lib.straps_regressor_train_param_floats(d) == sum(p.numel() for p in reg.parameters())
        assert lib.straps_regressor_bn_state_floats(d) == 2 * sum(m.num_features for m in bns)
    flat = straps_amd.flat_training_params(reg)
    assert flat.numel() == sum(p.numel() for p in reg.parameters())
    assert flat[:reg.image_encoder.conv1.weight.numel()].equal(reg.image_encoder.conv1.weight.detach().reshape(-1))
    assert flat[-157:].equal(reg.ief_module.fc3.bias.detach())
    bn = straps_amd.flat_bn_state(reg)
    assert bn[:64].equal(reg.image_encoder.bn1.running_mean) and bn[64:128].equal(reg.image_encoder.bn1.running_var)


def _fwd(lib, d, params=P, bn=P, init=P, x=P, batch=2, h=256, w=256, est=P, ld_est=157, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.straps_regressor_train_workspace_bytes(d, max(batch, 1), h, w)
    return lib.straps_regressor_fwd_train(d, C.c_void_p(params), C.c_void_p(bn), C.c_void_p(init), C.c_void_p(x), batch, h, w, C.c_void_p(est), ld_est,
                                          C.c_void_p(ws), ws_bytes, None)


def _bwd(lib, d, params=P, x=P, batch=2, h=256, w=256, dest=P, ld_dest=157, grads=P, dx=None, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.straps_regressor_train_workspace_bytes(d, max(batch, 1), h, w)
    return lib.straps_regressor_bwd(d, C.c_void_p(params), C.c_void_p(x), batch, h, w, C.c_void_p(dest), ld_dest, C.c_void_p(grads), C.c_void_p(dx),
                                    C.c_void_p(ws), ws_bytes, None)


def test_argument_validation_without_gpu(lib):
    """every failure below returns EINVAL before any HIP call (the pointers are never dereferenced) and names the argument"""
    d = _desc()
    for name in ('params', 'bn', 'init', 'x', 'est', 'ws'):
        field = {'bn': 'bn_state', 'init': 'init_est', 'ws': 'workspace'}.get(name, name)
        assert _fwd(lib, d, **{name: None}) == EINVAL and '`%s`' % field in _err(lib), name
    for name in ('params', 'x', 'dest', 'ws'):
        field = {'ws': 'workspace'}.get(name, name)
        assert _bwd(lib, d, **{name: None}) == EINVAL and '`%s`' % field in _err(lib), name
    assert _fwd(lib, d, batch=0) == EINVAL and '`batch`' in _err(lib)
    assert _bwd(lib, d, batch=0) == EINVAL and '`batch`' in _err(lib)
    assert _fwd(lib, d, ld_est=156) == EINVAL and '`ld_est`' in _err(lib)
    assert _bwd(lib, d, ld_dest=156) == EINVAL and '`ld_dest`' in _err(lib)
    need = lib.straps_regressor_train_workspace_bytes(d, 2, 256, 256)
    assert _fwd(lib, d, ws_bytes=need - 1) == EINVAL and '`workspace_bytes`' in _err(lib)
    assert _bwd(lib, d, ws_bytes=need - 1) == EINVAL and '`workspace_bytes`' in _err(lib)
    assert _fwd(lib, d, h=6) == EINVAL and '`h`' in _err(lib)
    # the input gradient's stem kernel covers at most 64 channels
    d65 = _desc(18, 65, 3, 0)
    assert _bwd(lib, d65, dx=P) == EINVAL and '`dx`' in _err(lib)
    for field, bad in (('layers', 34), ('precision', 2), ('in_channels', 0), ('ief_iters', 0)):
        db = _desc()
        setattr(db, field, bad)
        assert _fwd(lib, db) == EINVAL and '`%s`' % field in _err(lib), field
        assert _bwd(lib, db) == EINVAL and '`%s`' % field in _err(lib), field
        assert lib.straps_regressor_export_infer_params(db, C.c_void_p(P), C.c_void_p(P), C.c_void_p(P), C.c_void_p(P), None) == EINVAL
        assert '`%s`' % field in _err(lib)
        assert lib.straps_regressor_train_param_floats(db) == 0 and lib.straps_regressor_bn_state_floats(db) == 0
        assert lib.straps_regressor_train_workspace_bytes(db, 2, 256, 256) == 0
    for i, field in enumerate(('params', 'bn_state', 'init_est', 'infer_params')):
        ptrs = [C.c_void_p(P)] * 4
        ptrs[i] = None
        assert lib.straps_regressor_export_infer_params(d, *ptrs, None) == EINVAL and '`%s`' % field in _err(lib), field
    assert lib.straps_regressor_fwd_train(None, *[C.c_void_p(P)] * 4, 1, 256, 256, C.c_void_p(P), 157, C.c_void_p(P), 1 << 40, None) == EINVAL
    assert '`desc`' in _err(lib)
    assert lib.straps_regressor_train_param_floats(None) == 0
    # invalid geometry: no workspace size
    assert lib.straps_regressor_train_workspace_bytes(d, 0, 256, 256) == 0
    assert lib.straps_regressor_train_workspace_bytes(d, 1, 6, 256) == 0


@pytest.mark.parametrize('precision', [0, 1])
@pytest.mark.parametrize('layers', [18, 50])
def test_workspace_grows_with_batch(lib, layers, precision):
    d = _desc(layers, 18, 3, precision)
    sizes = [lib.straps_regressor_train_workspace_bytes(d, b, 256, 256) for b in (1, 2, 5, 16, 32)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.straps_regressor_train_workspace_bytes(d, 4, 224, 192) < lib.straps_regressor_train_workspace_bytes(d, 4, 256, 256)
    # the tape keeps every layer: more than the inference workspace's reused slots
    assert lib.straps_regressor_train_workspace_bytes(d, 8, 256, 256) > lib.straps_regressor_workspace_bytes(d, 8, 256, 256)


def test_example_compiles_against_header(lib, tmp_path):
    out = tmp_path / 'regressor_train'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'regressor_train.cpp'),
           '-o', str(out), '-L', os.path.dirname(hipabi.LIB_PATH), '-lstraps_hip']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert out.is_file()
