"""CPU: the single-product bf16 route's host side -- precision 3 of the composite inference (size queries, refusals of every train entry point),
argument checks of the new entry points before any launch, the Python surface, and a numpy model of the route's error budget."""
import ctypes as C

import numpy as np
import pytest

import straps_amd
from bf16x3_emul import bf16_bits_to_f32, bf16_rn_bits
from straps_amd import hipabi

EINVAL = 1
P = 8192        # a non-null, never dereferenced address (16-byte aligned)


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _desc(layers=50, cin=18, iters=3, precision=3):
    return hipabi.RegressorDesc(layers, cin, iters, precision)


def _err(lib):
    return lib.straps_last_error().decode()


@pytest.mark.parametrize('layers', [18, 50])
def test_precision_3_size_queries(lib, layers):
    d3, d0 = _desc(layers, 18, 3, 3), _desc(layers, 18, 3, 0)
    assert lib.straps_regressor_param_floats(d3) == lib.straps_regressor_param_floats(d0) > 0
    p3, p0 = lib.straps_regressor_prepared_bytes(d3), lib.straps_regressor_prepared_bytes(d0)
    assert 0 < p3 < p0                         # one weight plane instead of three
    convs = sum(v.numel() for k, v in straps_amd.SingleInputRegressor(18, layers, 3, mean_params=straps_amd.synthetic_mean_params(0))
                .image_encoder.state_dict().items() if k.endswith('.weight') and v.dim() == 4 and not k.startswith('conv1'))
    assert p0 - p3 >= 2 * 2 * convs            # (two planes of 2 bytes per weight fewer)
    for B in (1, 64):
        w3, w0 = lib.straps_regressor_workspace_bytes(d3, B, 256, 256), lib.straps_regressor_workspace_bytes(d0, B, 256, 256)
        assert 0 < w3 < w0                     # one activation plane instead of three
    assert lib.straps_regressor_workspace_bytes(d3, 0, 256, 256) == 0


def test_precision_2_stays_invalid(lib):
    d = _desc(precision=2)
    assert lib.straps_regressor_prepared_bytes(d) == 0 and lib.straps_regressor_workspace_bytes(d, 1, 256, 256) == 0
    assert lib.straps_regressor_prepare(d, C.c_void_p(P), C.c_void_p(256 * 64), None) == EINVAL and '`precision`' in _err(lib)
    assert lib.straps_regressor_fwd_infer(d, C.c_void_p(256 * 64), C.c_void_p(P), 1, 256, 256, C.c_void_p(P), 157, None, C.c_void_p(256 * 64),
                                          1 << 40, None) == EINVAL and '`precision`' in _err(lib)


def test_every_train_entry_rejects_precision_3(lib):
    d = _desc(precision=3)
    assert lib.straps_regressor_train_param_floats(d) == 0
    assert lib.straps_regressor_bn_state_floats(d) == 0
    assert lib.straps_regressor_train_workspace_bytes(d, 2, 256, 256) == 0
    v = C.c_void_p(P)
    assert lib.straps_regressor_fwd_train(d, v, v, v, v, 2, 256, 256, v, 157, C.c_void_p(256 * 64), 1 << 40, None) == EINVAL
    assert '`precision`' in _err(lib)
    assert lib.straps_regressor_bwd(d, v, v, 2, 256, 256, v, 157, v, None, C.c_void_p(256 * 64), 1 << 40, None) == EINVAL
    assert '`precision`' in _err(lib)
    assert lib.straps_regressor_export_infer_params(d, v, v, v, v, None) == EINVAL and '`precision`' in _err(lib)


def test_new_entry_points_check_arguments_before_any_launch(lib):
    v = C.c_void_p(P)
    # (every call below would fault if it launched: the pointers are not device memory)
    assert lib.straps_split_bf16_cm(None, v, 16, 64, None) == EINVAL and 'null' in _err(lib)
    assert lib.straps_split_bf16_cm(v, v, 16, 48, None) == EINVAL and 'c % 32' in _err(lib)
    assert lib.straps_split_bf16_cm(v, v, 0, 64, None) == EINVAL
    assert lib.straps_split_bf16_cm(C.c_void_p(P + 4), v, 16, 64, None) == EINVAL and 'aligned' in _err(lib)
    assert lib.straps_pack_conv_weight_bf16(None, v, 64, 64, 3, 3, None) == EINVAL and 'null' in _err(lib)
    assert lib.straps_pack_conv_weight_bf16(v, v, 64, 48, 3, 3, None) == EINVAL and 'cin % 32' in _err(lib)
    assert lib.straps_pack_conv_weight_bf16(v, v, 64, 64, 5, 5, None) == EINVAL and 'geometry' in _err(lib)

    def fwd(x=v, w=v, scale=v, shift=v, y=v, yp=v, B=2, h=8, wd=8, cin=64, cout=64, k=3, s=1, p=1, cfg=0):
        return lib.straps_conv_fwd_bf16(x, w, scale, shift, None, 1, y, yp, B, h, wd, cin, cout, k, k, s, p, cfg, None)
    assert fwd(x=None) == EINVAL and 'null' in _err(lib)
    assert fwd(y=None, yp=None) == EINVAL and 'no output' in _err(lib)
    assert fwd(B=0) == EINVAL and 'empty' in _err(lib)
    assert fwd(cin=32) == EINVAL and 'cin%64' in _err(lib)
    assert fwd(cout=96) == EINVAL and 'cout%64' in _err(lib)
    assert fwd(k=4) == EINVAL and 'geometry' in _err(lib)
    assert fwd(scale=None) == EINVAL and 'together' in _err(lib)
    assert fwd(x=C.c_void_p(P + 8)) == EINVAL and 'aligned' in _err(lib)
    assert fwd(cfg=11) == EINVAL and 'tile_cfg' in _err(lib)
    assert fwd(cfg=-1) == EINVAL
    assert fwd(cfg=1) == EINVAL and 'N extent' in _err(lib)            # 128-wide tile on 64 output channels
    assert fwd(cin=64, cout=128, cfg=6) == EINVAL and 'cin % 128' in _err(lib)
    assert fwd(cout=128, s=2, cfg=9) == EINVAL and 'halo' in _err(lib)
    assert fwd(k=1, p=0, cfg=10) == EINVAL and 'halo' in _err(lib)


def test_tile_rule_covers_every_eval_shape(lib):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from sweep_conv_bf16 import eval_conv_shapes
    for layers in (18, 50):
        for (H, W, cin, cout, k, s, p, _) in eval_conv_shapes(layers):
            for B in (1, 5, 64, 256):
                assert 1 <= lib.straps_conv_bf16_tile_choice(B, H, W, cin, cout, k, k, s, p) <= 10
    assert lib.straps_conv_bf16_tile_choice(1, 8, 8, 32, 64, 3, 3, 1, 1) == -1


def test_python_surface():
    net = straps_amd.resnet18(18, conv_precision='bf16')
    assert net.conv_precision == 'bf16'
    net.conv_precision = 'bf16x3'
    net.conv_precision = 'bf16'
    with pytest.raises(ValueError):
        straps_amd.resnet18(18, conv_precision='bf16x2')
    from straps_amd import infer
    assert infer.PRECISIONS['bf16'] == 3 and 2 not in infer.PRECISIONS.values()
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=straps_amd.synthetic_mean_params(0))
    reg.image_encoder.conv_precision = 'bf16'
    d = infer.regressor_desc(reg)
    assert (d.layers, d.in_channels, d.ief_iters, d.precision) == (18, 18, 3, 3)
    assert infer.regressor_desc(reg, 'bf16x3').precision == 0
    # SMPL precisions are a different switch: 'bf16' is not one of them
    with pytest.raises(Exception):
        straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=1, precision='bf16')


def _rn(a):
    return bf16_bits_to_f32(bf16_rn_bits(a.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize('K', [64, 576, 2048, 4608])
def test_error_model_of_one_product_per_term(K):
    """numpy model of one output of the route: sum_k rn(a_k) rn(b_k), products exact, fp32 accumulation (modelled here in float64: its rounding
    is 2^-24-class, below what is checked).  Against the fp32-operand dot product the error is the operands' rounding: each rn() is within
    2^-9 relative, so |err| <= (2^-8 + 2^-18) sum |a_k b_k| holds for every output, and for random data the error is a random walk far inside it"""
    rng = np.random.default_rng(K)
    a = rng.uniform(-1, 1, (256, K)).astype(np.float32)
    b = (rng.standard_normal(K) * (2.0 / K) ** 0.5).astype(np.float32)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    route = _rn(a) @ _rn(b)
    l1 = np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))
    err = np.abs(route - exact)
    assert np.all(err <= (2.0 ** -8 + 2.0 ** -18) * l1)
    # random-walk size: rms of the error ~ 2^-9 / sqrt(3) * sqrt(2) * rms of the products * sqrt(K); 3x margin
    rms_prod = np.sqrt(np.mean((a.astype(np.float64) * b.astype(np.float64)) ** 2, axis=1))
    assert np.sqrt(np.mean(err ** 2)) <= 3 * 2.0 ** -9 * np.sqrt(2.0 / 3.0) * np.sqrt(K) * np.mean(rms_prod)
    # and the route is not the fp32 chain: the bf16x3 route's bar (2e-5 relative) is far below this error
    assert np.max(err / np.maximum(l1, 1e-30)) > 1e-4
