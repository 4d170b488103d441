"""CPU: the model variants and input conditions of tests/test_gpu_smpl_fwd_edges.py, from the oracle and the packing alone -- what
pack_smpl_model makes of every variant, the packed tables read back into the forward they stand for (a packing error is then told from a
kernel error), and the distance of the float32 oracle from the float64 oracle on every case of the GPU matrix."""
import ctypes as C

import numpy as np
import pytest
import torch

import smpl_fwd_cases as FC
from straps_amd import hipabi
from straps_amd.smpl import MAX_TILES, pack_smpl_model

CONDITIONING_BAR = 5e-6          # a quarter of the 2e-5 m of every SMPL test: the bar then tests the kernel and not the case
PACKED_BODIES = 8                # bodies of a variant's case that go through numpy_forward_from_packed (body 0 the extreme one, 1 the identity)


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _virtual_bones(p, j):
    """the bones of the virtual vertices of regressed joint j (0..44)"""
    e0, e1 = int(p['vj_ptr'][j]), int(p['vj_ptr'][j + 1])
    return np.asarray(p['skin_j'])[FC.VPAD + e0:FC.VPAD + e1, 0]


@pytest.mark.parametrize('name', list(FC.FWD_VARIANTS))
def test_packed_figures_of_every_variant(lib, name):
    p = FC.packed(name)
    got = (p['n_tiles'], int(p['vj_ptr'][45]), p['skin_k'], p['max_depth'])
    print('%s: n_tiles %d, nvirt %d, skin_k %d, max_depth %d; joint kernel LDS %d bytes' % ((name,) + got + (4 * (p['n_tiles'] - 216) * 96 * 4,)))
    assert got == FC.PACKED_FIGURES[name]
    assert p['n_tiles'] % 8 == 0 and 216 + (got[1] + 31) // 32 <= p['n_tiles'] <= MAX_TILES
    assert p['skin_w'].shape == (32 * p['n_tiles'], p['skin_k']) and not p['skin_w'][FC.VPAD + got[1]:].any()      # padding rows: weight 0
    s = hipabi.SmplModelStruct()
    s.n_tiles = p['n_tiles']
    for B in (1, 67, 129, 65536):
        assert lib.straps_smpl_workspace_bytes(C.byref(s), B) == B * (224 + 288 + (p['n_tiles'] - 216) * 96) * 4 == FC.workspace_bytes_formula(B, p['n_tiles'])
    # the sign split of a cancelling (joint, bone) pair: taken for 'signed_regressor' and for no other variant -- from the model (the
    # condition restated) and from the packed tables (a joint with two virtual vertices on one bone)
    twice = [j for j in range(45) if len(set(_virtual_bones(p, j).tolist())) < len(_virtual_bones(p, j))]
    if name == 'signed_regressor':
        assert FC.sign_split_pairs(FC.model(name)) == 4 and twice == [28 + FC.SIGNED_ROW]
        assert len(_virtual_bones(p, 28 + FC.SIGNED_ROW)) == 9
        assert (np.asarray(p['skin_w'])[FC.VPAD:FC.VPAD + got[1], 0] < 0).any()                  # the negative halves carry negative weights
    else:
        assert FC.sign_split_pairs(FC.model(name)) == 0 and twice == []
    empty = [j for j in range(45) if p['vj_ptr'][j + 1] == p['vj_ptr'][j]]
    assert empty == ([FC.EMPTY_ROW] if name == 'empty_regressor_row' else [])
    if name == 'all_dense_regressors':
        assert all(len(_virtual_bones(p, j)) == 24 for j in range(45))                          # every (joint, bone) pair: the most non-negative rows can give
    # the K-packed skinning operand: [hi | hi | lo | 0 x 8]
    P = FC.unpack_skin_frag_p(p)
    assert np.array_equal(P[:, 24:48], P[:, :24]) and not P[:, 72:].any()


@pytest.mark.parametrize('name', list(FC.FWD_VARIANTS))
def test_packed_tables_restate_the_oracle(name):
    """numpy_forward_from_packed == O.smpl_forward in float64: <= 1e-6 m through the fp32 tables (blend_frag, skin_w / skin_j: fp32 roundings
    of the float64 virtual-vertex directions), and through the tables rebuilt from the two-term fp16 splits <= 1e-6 m AND <= the bound
    derived from the case (2^-22 relative per split entry, carried through the contraction and the skinning: smpl_fwd_cases)."""
    x = FC.inputs('var_' + name)
    b, R = x['betas'][:PACKED_BODIES], x['R'][:PACKED_BODIES]
    v64, j64 = FC.oracle_forward(FC.model(name), b, R, torch.float64)
    p = FC.packed(name)
    v, j = FC.numpy_forward_from_packed(p, b.numpy(), R.numpy(), 'fp32')
    r32 = FC.assert_close('%s, fp32 tables' % name, v, j, v64, j64, 1e-6)
    v, j, bound = FC.numpy_forward_from_packed(p, b.numpy(), R.numpy(), 'split', with_bound=True)
    vf, jf = FC.numpy_forward_from_packed(p, b.numpy(), R.numpy(), 'fp32')
    d = FC.error_report(v, j, torch.from_numpy(vf), torch.from_numpy(jf))
    rs = FC.assert_close('%s, fp16-split tables' % name, v, j, v64, j64, 1e-6)
    print('%s: fp32 tables %s | split tables %s | split tables against fp32 tables %.3e / %.3e, derived bound %.3e'
          % (name, FC.describe(r32), FC.describe(rs), d['verts'], d['joints'], bound))
    assert bound <= 2e-6                                             # (the bound itself: a tenth of the 2e-5 m bar at most)
    assert max(d['verts'], d['joints']) <= bound, '%s: the split tables differ from the fp32 tables by %s, derived bound %.3e' % (name, FC.describe(d), bound)
    if name == 'empty_regressor_row':
        assert not j[:, FC.EMPTY_JOINT].any() and not j64[:, FC.EMPTY_JOINT].any()


def test_float32_oracle_is_within_a_quarter_of_the_bar_on_every_case():
    """a condition on the INPUTS of the GPU matrix: the float32 oracle within 5e-6 m of the float64 oracle on vertices and joints.  A case
    that misses it gets another recipe or seed (smpl_fwd_cases.SEEDS), chosen by the oracle alone; the bar stays."""
    worst, where = 0.0, None
    for name in FC.CASES:
        v64, j64 = FC.oracle(name, torch.float64)
        v32, j32 = FC.oracle(name, torch.float32)
        rep = FC.assert_close('float32 oracle, case %s' % name, v32, j32, v64, j64, CONDITIONING_BAR)
        if max(rep['verts'], rep['joints']) > worst:
            worst, where = max(rep['verts'], rep['joints']), '%s: %s' % (name, FC.describe(rep))
    print('float32 oracle, worst distance from float64 over %d cases: %.3e m (%s)' % (len(FC.CASES), worst, where))
    assert 1e-8 < worst


def test_special_bodies_are_what_they_are_named_for():
    x = FC.inputs('input_edges')
    assert x['betas'][0].tolist() == list(FC.EXTREME_BETAS)
    assert not x['betas'][1].any() and torch.equal(x['R'][1], torch.eye(3).expand(24, 3, 3))
    eye = torch.eye(3).double()
    orth = lambda R: float((R.double().transpose(-1, -2) @ R.double() - eye).abs().max())
    assert orth(x['R'][2]) < 1e-6 and orth(x['R'][3]) > 0.02 and orth(x['R'][4]) < 1e-6
    angle = torch.acos(((x['R'][2].diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1))
    assert float(angle.max()) > 2.5                                                  # rotations near pi
    v64, j64 = FC.oracle('input_edges', torch.float64)
    m = FC.model('seed0')
    # (the fp32 skinning weights of a vertex sum to 1 within 4 x 2^-25: the identity body is v_template within 1.2e-7 x 0.85 m)
    assert float((v64[1] - torch.from_numpy(m['v_template']).double()).abs().max()) < 1.1e-7
    assert float((j64[1, :24] - torch.from_numpy(m['J_regressor']).double() @ torch.from_numpy(m['v_template']).double()).abs().max()) < 1e-12


def test_models_beyond_the_virtual_vertex_row_are_refused_at_packing():
    """45 dense rows with sign changes: every (joint, bone) pair cancels and is split in two -- 2160 virtual vertices, 288 tiles; the joint
    kernel would need 4 x 72 x 96 x 4 = 110 592 bytes of LDS.  (The C side of the same bound: tests/test_gpu_smpl_fwd_edges.py.)"""
    m = dict(FC.model('all_dense_regressors'))
    for key in ('J_regressor_extra', 'J_regressor_cocoplus', 'J_regressor_h36m'):
        a = m[key].astype(np.float64)
        for r in range(a.shape[0]):
            nz = np.nonzero(a[r])[0]
            a[r, nz[1::2]] *= -0.8
        m[key] = a.astype(np.float32)
    with pytest.raises(ValueError, match='at most 256'):
        pack_smpl_model(m)
    assert MAX_TILES == 256 and FC.packed('all_dense_regressors')['n_tiles'] == MAX_TILES      # the largest model non-negative rows give is accepted
