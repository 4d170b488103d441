"""CPU: the one-call regressor inference entry points (straps_regressor_*, ABI 11) -- parameter layout, argument validation and workspace
sizing are host code, checkable without a GPU; the torch-free example compiles against the header."""
import ctypes as C
import json
import math
import os
import subprocess

import pytest

import straps_amd
from straps_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
EINVAL = 1


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _desc(layers=50, cin=18, iters=3, precision=0):
    return hipabi.RegressorDesc(layers, cin, iters, precision)


def _manifest_floats(layers, cin):
    keys = json.load(open(os.path.join(GOLD, 'state_dict_keys_r%d.json' % layers)))['keys']
    n = 0
    for k, shape in keys.items():
        if k.endswith('num_batches_tracked') or '.ief_layers.' in k:
            continue
        if k == 'image_encoder.conv1.weight':
            shape = [shape[0], cin] + shape[2:]
        n += math.prod(shape)
    return n + 157


@pytest.mark.parametrize('layers', [18, 50])
@pytest.mark.parametrize('cin', [1, 18])
def test_param_floats_match_module_and_manifest(lib, layers, cin):
    reg = straps_amd.SingleInputRegressor(cin, layers, 3, mean_params=straps_amd.synthetic_mean_params(0))
    flat = straps_amd.flat_inference_params(reg)
    n = lib.straps_regressor_param_floats(_desc(layers, cin))
    assert n == flat.numel() == _manifest_floats(layers, cin)
    # the layout: conv1.weight first, the initial estimate last
    assert flat[:reg.image_encoder.conv1.weight.numel()].equal(reg.image_encoder.conv1.weight.detach().reshape(-1))
    assert flat[-157:].equal(reg.ief_module.initial_params_estimate)
    assert lib.straps_regressor_prepared_bytes(_desc(layers, cin)) > 0


def _err(lib):
    return lib.straps_last_error().decode()


def _fwd(lib, d, prepared=8192, x=8192, batch=2, h=256, w=256, est=8192, ld_est=157, rot=None, ws=8192, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.straps_regressor_workspace_bytes(d, max(batch, 1), h, w)
    return lib.straps_regressor_fwd_infer(d, C.c_void_p(prepared), C.c_void_p(x), batch, h, w, C.c_void_p(est), ld_est, C.c_void_p(rot),
                                          C.c_void_p(ws), ws_bytes, None)


def test_argument_validation_without_gpu(lib):
    """every failure below returns EINVAL before any HIP call (the pointers are never dereferenced) and names the argument"""
    d = _desc()
    assert lib.straps_regressor_prepare(d, None, C.c_void_p(8192), None) == EINVAL and '`params`' in _err(lib)
    assert lib.straps_regressor_prepare(d, C.c_void_p(8192), None, None) == EINVAL and '`prepared`' in _err(lib)
    assert _fwd(lib, d, prepared=None) == EINVAL and '`prepared`' in _err(lib)
    assert _fwd(lib, d, x=None) == EINVAL and '`x`' in _err(lib)
    assert _fwd(lib, d, est=None) == EINVAL and '`est`' in _err(lib)
    assert _fwd(lib, d, ws=None) == EINVAL and '`workspace`' in _err(lib)
    assert _fwd(lib, d, batch=0) == EINVAL and '`batch`' in _err(lib)
    assert _fwd(lib, d, ld_est=156) == EINVAL and '`ld_est`' in _err(lib)
    need = lib.straps_regressor_workspace_bytes(d, 2, 256, 256)
    assert _fwd(lib, d, ws_bytes=need - 1) == EINVAL and '`workspace_bytes`' in _err(lib)
    for field, bad in (('layers', 34), ('precision', 2), ('in_channels', 0), ('ief_iters', 0)):
        db = _desc()
        setattr(db, field, bad)
        assert _fwd(lib, db) == EINVAL and '`%s`' % field in _err(lib), field
        assert lib.straps_regressor_prepare(db, C.c_void_p(8192), C.c_void_p(8192), None) == EINVAL and '`%s`' % field in _err(lib)
        assert lib.straps_regressor_param_floats(db) == 0 and lib.straps_regressor_prepared_bytes(db) == 0
        assert lib.straps_regressor_workspace_bytes(db, 2, 256, 256) == 0
    assert lib.straps_regressor_fwd_infer(None, C.c_void_p(8192), C.c_void_p(8192), 1, 256, 256, C.c_void_p(8192), 157, None,
                                          C.c_void_p(8192), 1 << 40, None) == EINVAL
    assert lib.straps_regressor_param_floats(None) == 0
    # invalid geometry: no workspace size
    assert lib.straps_regressor_workspace_bytes(d, 0, 256, 256) == 0
    assert lib.straps_regressor_workspace_bytes(d, 1, 6, 256) == 0


@pytest.mark.parametrize('precision', [0, 1])
@pytest.mark.parametrize('layers', [18, 50])
def test_workspace_grows_with_batch_and_stays_bounded(lib, layers, precision):
    d = _desc(layers, 18, 3, precision)
    sizes = [lib.straps_regressor_workspace_bytes(d, b, 256, 256) for b in (1, 2, 3, 5, 16, 37, 64)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.straps_regressor_workspace_bytes(d, 4, 224, 224) < lib.straps_regressor_workspace_bytes(d, 4, 256, 256)
    # fixed slots, not a sum over layers: resnet50 at 64 bodies, 256 x 256, within 8x the stem output
    stem_out = 64 * 128 * 128 * 64 * 4
    assert lib.straps_regressor_workspace_bytes(d, 64, 256, 256) <= 8 * stem_out
    # the prepared buffer does not depend on the batch or the image
    assert lib.straps_regressor_prepared_bytes(d) == lib.straps_regressor_prepared_bytes(_desc(layers, 18, 3, precision))


def test_example_compiles_against_header(lib, tmp_path):
    out = tmp_path / 'regressor_infer'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'regressor_infer.cpp'),
           '-o', str(out), '-L', os.path.dirname(hipabi.LIB_PATH), '-lstraps_hip']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert out.is_file()
