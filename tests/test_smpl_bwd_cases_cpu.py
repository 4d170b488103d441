"""CPU: the input conditions of tests/test_gpu_smpl_bwd_edges.py and tests/test_gpu_loss_head_edges.py, from the oracle alone, and the
host-side arithmetic / argument checks of the entry points they call (no compute calls -- there is no GPU here)."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_metrics as G
import smpl_cases as S
from straps_amd import hipabi
from straps_amd.smpl import pack_smpl_model

EINVAL = 1


@pytest.fixture(scope='module', autouse=True)
def _threads():
    before = torch.get_num_threads()
    torch.set_num_threads(S.cpu_threads())
    yield
    torch.set_num_threads(before)


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


@pytest.mark.parametrize('name', S.DENSE)
def test_no_scale_of_a_dense_case_is_below_1e_3_of_its_tensor_maximum(name):
    """the dense cases are compared per joint / component / body WITHOUT a floor: every such scale of the float64 oracle must be at
    least 1e-3 of its tensor's maximum.  If one is not, change the input, not the metric."""
    for kind in S.CASES[name]['kinds']:
        for k, ref in S.oracle(name, kind, torch.float64).items():
            if ref is None:
                continue
            tmax, sg, sb = G.slice_scales(ref)
            assert tmax > 0 and sg.min() >= 1e-3 * tmax and sb.min() >= 1e-3 * tmax, \
                '%s/%s %s: smallest group scale %.2e, body scale %.2e of the maximum' % (name, kind, k, sg.min() / tmax, sb.min() / tmax)


def test_float32_oracle_floor_is_fp32_class():
    """the floor of the measured bar is the float32 oracle's worst slice error over the whole matrix.  It must stay what fp32 arithmetic
    costs, well under the 1e-4 ceiling, or the measured bar means nothing.  The worst plain evaluation is a sequential sum: dbetas adds
    N = 20670 products of random sign, error <= N x 2^-24 of a term against a result of about sqrt(N) terms, i.e. 1e-5 (measured: 2.1e-6
    with a blocked BLAS, 1.07e-5 on another host); 2.5 x that is the bound.  An ill-conditioned input exceeds it at once (batch1 with its
    first seed: 1.2e-4 -- smpl_cases.py)."""
    floor = S.float32_floor()
    print('float32 oracle, worst slice error over the matrix: %.3e (%s)' % (floor, S.float32_floor_case()))
    assert 1e-7 < floor < 2.5e-5


def test_sparse_cases_have_the_structure_they_are_named_for():
    r = S.oracle('onehot0', 'joints', torch.float64)
    assert not r['drot'].any() and r['dbetas'].abs().max() > 0          # a gradient at the root's position moves no rotation
    r = S.oracle('onehot23', 'joints', torch.float64)
    assert int((G.slice_scales(r['drot'])[1] == 0).sum()) == 16          # 8 joints on the path root .. 23
    r = S.oracle('one_body', 'both', torch.float64)
    assert [bool(r['drot'][b].any()) for b in range(5)] == [False, False, False, True, False]
    x = S.inputs('verts_last_tile')
    assert not x['gv'][:, :6880].any() and bool(x['gv'][:, 6880:].all())


def test_model_variants_are_what_they_are_named_for():
    nnz = lambda n: (np.asarray(S.model(n)['weights']) != 0).sum(1)
    assert nnz('rigid').max() == 1 and pack_smpl_model(S.model('rigid'))['skin_k'] == 1
    w = nnz('wide')
    assert w.max() == 7 and all(w[v] == 7 for v in S.WIDE_FIXED) and 0.04 < (w == 7).mean() < 0.06
    np.testing.assert_allclose(np.asarray(S.model('wide')['weights'], np.float64).sum(1), 1.0, atol=1e-6)
    pw = pack_smpl_model(S.model('wide'))
    assert pw['skin_k'] == 7 and not pw['skin_w'][6890:6912].any()       # rows 6890..6911 of the last tile are padding: weight 0 at joint 0
    assert not np.asarray(S.model('unskinned_joint')['weights'])[:, 15].any()
    assert pack_smpl_model(S.model('chain_tree'))['max_depth'] == 23
    ps = pack_smpl_model(S.model('shallow_tree'))
    assert ps['max_depth'] == 3 and (ps['children'][0] >= 0).sum() == 3
    d = S.model('dense_regressors')
    assert (d['J_regressor'][7] != 0).sum() == 400 and (d['J_regressor_h36m'][S.DENSE_ROW_H36M] != 0).sum() == 400
    lens = np.diff(pack_smpl_model(d)['jrt_ptr'])
    assert lens[100:112].min() >= 2.5 * np.median(lens)                    # long joint-gradient lists in the tiles of vertices 3200..3599


def test_unsupported_trees_are_refused_at_construction():
    m = S.MODEL_VARIANTS['seed0']()
    m['parents'] = np.asarray([-1, 0, 0, 0, 0] + list(range(4, 23)), np.int32)          # the root with four children
    with pytest.raises(AssertionError, match='more than 3 children'):
        pack_smpl_model(m)
    m['parents'] = np.asarray([-1, 2, 0] + list(range(2, 23)), np.int32)                 # joint 1 hangs on joint 2
    with pytest.raises(AssertionError, match='topologically ordered'):
        pack_smpl_model(m)


def test_smpl_bwd_workspace_bytes_formula_and_monotone(lib):
    """straps_smpl_bwd_workspace_bytes == the formula of include/straps_hip.h for a spread of batches up to 2^21 (host arithmetic, nothing
    is allocated), and is monotone in the number of chunks"""
    for B in (1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025, 4096, 65536, 1 << 20, (1 << 21) - 1, 1 << 21):
        prev = 0
        for chunks in list(range(1, 56)) + [100, 1 << 20]:
            got = lib.straps_smpl_bwd_workspace_bytes(B, chunks)
            assert got == S.workspace_bytes_formula(B, chunks), (B, chunks)
            assert got >= prev, 'workspace shrinks from chunks=%d to %d at B=%d' % (chunks - 1, chunks, B)
            prev = got
        assert lib.straps_smpl_bwd_workspace_bytes(B, 0) == S.workspace_bytes_formula(B, 8 if B >= 1024 else 54)
        assert lib.straps_smpl_bwd_workspace_bytes(B, -3) == lib.straps_smpl_bwd_workspace_bytes(B, 0)
        assert lib.straps_smpl_bwd_workspace_bytes(B, 1) == B * 2 * 512 * 4 and lib.straps_smpl_bwd_workspace_bytes(B, 54) == B * 55 * 512 * 4


def test_loss_head_argument_checks(lib):
    """ld_est < 157 and a call that gives some gradient outputs and not others are refused before any launch"""
    f = C.c_void_p(16)           # never dereferenced: validation fails first
    def call(ld_est=160, outs=(f, f, f, f, f)):
        return lib.straps_loss_fwd_bwd(f, f, f, ld_est, f, f, f, f, f, f, f, f, *outs, f, 4, 256, None)
    assert call(ld_est=156) == EINVAL and b'ld_est=156' in lib.straps_last_error()
    for i in range(5):
        some = [f] * 5
        some[i] = None
        assert call(outs=some) == EINVAL, 'output %d missing' % i
        assert b'all gradient outputs or none' in lib.straps_last_error()
        one = [None] * 5
        one[i] = f
        assert call(outs=one) == EINVAL, 'output %d alone' % i
