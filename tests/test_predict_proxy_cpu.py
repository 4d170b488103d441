"""CPU: the predict-side proxy input (straps_predict_proxy_input, straps_amd.predict) without a GPU -- the numpy restatement of the
header's semantics (tests/predict_cases.py) reproduces what the reference itself computed (tests/golden/predict_proxy_golden.npz,
written by tools/make_predict_proxy_golden.py); the caller-supplied Gaussian table is the reference's; the symbol is exported and
bound; every argument check answers before any HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

import predict_cases as PC
import straps_amd
from straps_amd import hipabi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'predict_proxy_golden.npz')
EINVAL = 1


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


@pytest.mark.parametrize('group', sorted(PC.GROUPS))
def test_case_table_is_the_golden_input_and_keeps_its_properties(gold, group):
    sil, joints = PC.inputs(group)
    H, W, nj, ld, outs, samples = PC.GROUPS[group]
    assert sil.shape == (len(samples), H, W) and sil.dtype == np.uint8 and joints.shape == (len(samples), nj, ld) and joints.dtype == np.float32
    assert np.array_equal(sil, gold['%s_sil' % group]) and np.array_equal(joints, gold['%s_joints' % group])
    PC.check_properties(group)


def test_case_table_covers_sizes_and_joint_layouts():
    shapes = {(g[0], g[1]) for g in PC.GROUPS.values()}
    assert shapes == {(64, 64), (80, 96), (96, 80)}
    assert {o for g in PC.GROUPS.values() for o in g[4]} == {32, 64}
    assert {(g[2], g[3]) for g in PC.GROUPS.values()} == {(17, 3), (1, 2)}          # 17 joints with a confidence column, and one bare joint
    assert max(len(g[5]) for g in PC.GROUPS.values()) == 5


@pytest.mark.parametrize('group', sorted(PC.GROUPS))
def test_restatement_reproduces_the_reference(gold, group):
    """silhouette and heat maps bit for bit, joints equal as float64"""
    sil, joints = PC.inputs(group)
    patch = straps_amd.heatmap_patch(PC.STD)
    for o in PC.GROUPS[group][4]:
        out, j64, boxes = PC.proxy_input(sil, joints, patch, o)
        assert boxes[:, 4].all()
        ref_sil, ref_j, ref_heat = gold['%s_o%d_sil' % (group, o)], gold['%s_o%d_joints' % (group, o)], gold['%s_o%d_heat' % (group, o)]
        assert out.dtype == np.float32 and np.array_equal(out[:, 0], ref_sil.astype(np.float32)), (group, o)
        assert ref_j.dtype == np.float64 and np.array_equal(j64, ref_j), (group, o)
        assert ref_heat.dtype == np.float32 and np.array_equal(out[:, 1:].view(np.uint32), ref_heat.view(np.uint32)), (group, o)


def test_golden_exercises_what_the_table_promises(gold):
    """the joints on the visibility bounds: the exact bound draws nothing, one pixel inside it draws a one-pixel-wide strip; a joint at
    -7.5 is drawn (truncation gives -7, floor would give the invisible -8); the last row / column never receives a value"""
    heat = gold['a_o32_heat'][3]                       # joints_on_bounds_32: targets PC.TARGETS_32 in order
    t = PC.TARGETS_32
    drawn = heat.reshape(17, -1).any(axis=1)
    for k in (2, 4, 6, 8, 15, 16):
        assert not drawn[k], t[k]
    for k in (0, 1, 3, 5, 7, 9, 10, 11, 12, 13, 14):
        assert drawn[k], t[k]
    assert np.nonzero(heat[3].any(axis=0))[0].tolist() == [0] and np.nonzero(heat[7].any(axis=0))[0].tolist() == [30]
    assert np.nonzero(heat[5].any(axis=1))[0].tolist() == [0] and np.nonzero(heat[9].any(axis=1))[0].tolist() == [30]
    assert np.nonzero(heat[10].any(axis=0))[0].tolist() == [0]
    assert not heat[:, 31, :].any() and not heat[:, :, 31].any()
    heat64 = gold['a_o64_heat'][4]                     # joints_on_bounds_64
    drawn64 = heat64.reshape(17, -1).any(axis=1)
    assert [bool(d) for d in drawn64] == [k not in (1, 3, 5, 7, 15, 16) for k in range(17)]
    # the windows leaving the frame really pad: zero rows / columns at the border of the resized silhouette
    assert not gold['b_o32_sil'][0][0].any() and not gold['b_o32_sil'][0][-1].any()
    assert not gold['c_o64_sil'][0][:, 0].any() and not gold['c_o64_sil'][0][:, -1].any()
    assert not gold['a_o64_sil'][0][0].any() and not gold['a_o64_sil'][0][:, 0].any()


def test_heatmap_patch_is_the_references_table(gold):
    """heatmap_patch(4) == the 16 x 16 patch of a golden heat map drawn whole (joint 0 of joints_on_bounds_32 sits at (16, 16))"""
    p = straps_amd.heatmap_patch(4)
    assert p.shape == (16, 16) and p.dtype == np.float32
    whole = gold['a_o32_heat'][3, 0, 8:24, 8:24]
    assert np.array_equal(p.view(np.uint32), whole.view(np.uint32))
    assert straps_amd.heatmap_patch(3).shape == (12, 12)
    with pytest.raises(ValueError):
        straps_amd.heatmap_patch(0)


def test_invalid_samples_in_the_restatement():
    inv = PC.invalid_silhouettes()
    sil = np.stack([inv['empty'], inv['one_pixel']])
    out, j64, boxes = PC.proxy_input(sil, np.full((2, 17, 3), 20.0, np.float32), straps_amd.heatmap_patch(4), 32)
    assert not out.any() and not j64.any()
    assert boxes.tolist() == [[0, 0, 0, 0, 0, 0], [20, 30, 20, 30, 0, 0]]


def test_symbol_exported_and_bound(lib):
    assert 'predict.hip' in hipabi.SOURCES
    assert hasattr(lib, 'straps_predict_proxy_input'), 'library does not export straps_predict_proxy_input'
    res, args = hipabi.SIGNATURES['straps_predict_proxy_input']
    assert res is C.c_int and len(args) == 15 and args[5] is C.c_double
    assert lib.straps_abi_version() == 12
    assert all(hasattr(straps_amd, n) for n in ('Predictor', 'create_proxy_representation_batch', 'heatmap_patch'))


def _call(lib, sil=8192, joints=8192, ld=3, patch=8192, std=4, scale=1.2, out=8192, jout=8192, boxes=8192, batch=2, h=512, w=512, nj=17, out_wh=256):
    p = lambda v: C.c_void_p(v)
    return lib.straps_predict_proxy_input(p(sil), p(joints), ld, p(patch), std, scale, p(out), p(jout), p(boxes), batch, h, w, nj, out_wh, None)


def test_argument_validation_without_gpu(lib):
    """every failure returns STRAPS_EINVAL before any HIP call (the pointers are never dereferenced) and names the argument"""
    err = lambda: lib.straps_last_error().decode()
    for name in ('sil', 'joints', 'patch', 'out', 'jout', 'boxes'):
        text = {'joints': 'joints2d', 'patch': 'gauss_patch', 'out': 'out_nchw', 'jout': 'out_joints2d'}.get(name, name)
        assert _call(lib, **{name: None}) == EINVAL and '`%s`' % text in err() and 'null pointer' in err(), name
    for out_wh in (30, 255, 0, -4):
        assert _call(lib, out_wh=out_wh) == EINVAL and '`out_wh`' in err(), out_wh
    for ld in (1, 0, -2):
        assert _call(lib, ld=ld) == EINVAL and '`ld_joint`' in err(), ld
    for std in (0, -1):
        assert _call(lib, std=std) == EINVAL and '`std`' in err(), std
    assert _call(lib, h=32768) == EINVAL and '`h`' in err()
    assert _call(lib, w=32768) == EINVAL and '`w`' in err()
    assert _call(lib, h=0) == EINVAL and '`h`' in err()
    assert _call(lib, batch=0) == EINVAL and '`batch`' in err()
    assert _call(lib, nj=0) == EINVAL and '`nj`' in err()
    for off in (4, 8, 12, 1):
        assert _call(lib, out=8192 + off) == EINVAL and '`out_nchw`' in err() and '16-byte' in err(), off
