"""CPU: the float64 reference of straps_fit_keypoints checks itself (tests/fit_cases.py), and pack_fit_model's tables are the model's rows.

The caps on the fits are conditions on the INPUTS of tests/test_gpu_fit_keypoints.py (the standard case must be one a fit solves), not on
the kernel."""
import numpy as np
import pytest
import torch

import fit_cases as FC
import straps_oracle as O
from smpl_cases import cpu_threads
from straps_amd import config
from straps_amd.fit import pack_fit_model
from straps_amd.smpl import pack_smpl_model


@pytest.fixture(scope='module', autouse=True)
def _threads():
    old = torch.get_num_threads()
    torch.set_num_threads(cpu_threads())
    yield
    torch.set_num_threads(old)


def test_autograd_gradient_vs_central_differences():
    case = FC.standard_case(B=3)
    est, tg, cf = case['est'].double(), case['targets'].double(), case['conf'].double()
    est0 = est + 0.01
    for sigma in (0.0, 0.1):
        _, g, _ = FC.energy_grad(est, est0, tg, cf, sigma=sigma)
        cols = [0, 1, 2, 3, 4, 8, 9 + 6 * 3, 3 + 6 * 9 + 5, 3 + 6 * 16, 3 + 6 * 17 + 1, 3 + 6 * 20 + 2, 3 + 6 * 23 + 5, 100, 120, 147, 148, 150, 153, 155, 156]
        assert len(cols) == 20
        h = 1e-6
        for c in cols:
            d = torch.zeros_like(est)
            d[:, c] = h
            with torch.no_grad():
                fd = (FC.energy(est + d, est0, tg, cf, sigma=sigma)[0] - FC.energy(est - d, est0, tg, cf, sigma=sigma)[0]) / (2 * h)
            err = float((fd - g[:, c]).abs().max() / g.abs().max())
            assert err < 1e-6, (sigma, c, err)


@pytest.mark.parametrize('name,cap', [('sigma0', 0.01), ('sigma01', 0.07)])
def test_standard_case_is_one_a_fit_solves(name, cap):
    case, traj, en, _ = FC.reference_fit(name)
    has_kp = (case['conf'] > 0).any(dim=1)
    assert int(has_kp.sum()) == 5 and not bool(has_kp[4])
    ratio = en[has_kp, -1] / en[has_kp, 0]
    print('E_100 / E_0 (%s):' % name, ratio.tolist())
    assert float(ratio.max()) <= cap
    assert float(en[4].abs().max()) == 0.0 and torch.equal(traj[-1, 4], traj[0, 4])      # the body without keypoints does not move
    px = case['targets']
    assert 0 < float(px.min()) and float(px.max()) < FC.IMG_WH


def test_nonmonotone_case_rises():
    case, _, en, _ = FC.reference_fit('nonmonotone')
    has_kp = (case['conf'] > 0).any(dim=1)
    rises = (en[has_kp, 1:] > en[has_kp, :-1]).sum(dim=1)
    print('rises per body:', rises.tolist())
    assert int(rises.min()) >= 5


def test_pack_fit_model_rows_are_the_models():
    M = FC.MODEL
    p = pack_fit_model(M)
    assert p['n_kp'] == 17 and p['n_verts'] == 5
    ev = [int(v) for v in M['extra_vertex_ids']]
    assert list(config.ALL_JOINTS_TO_COCO_MAP) == FC.COCO
    assert p['kp_src'].tolist() == [24, 25, 26, 27, 28, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8]      # output rows 24, 26, 25, 28, 27: vertices numbered by first appearance
    assert p['vertex_ids'].tolist() == [ev[0], ev[2], ev[1], ev[4], ev[3]]
    vt, sd, pd, W = (np.asarray(M[k], np.float32) for k in ('v_template', 'shapedirs', 'posedirs', 'weights'))
    for i, v in enumerate(p['vertex_ids'].tolist()):
        assert np.array_equal(p['vert_dirs'][i, :, 0], vt[v])
        assert np.array_equal(p['vert_dirs'][i, :, 1:11], sd[v])
        assert np.array_equal(p['vert_dirs'][i, :, 11:218], pd.reshape(207, -1, 3)[:, v, :].T)
        assert not p['vert_dirs'][i, :, 218:].any()
        assert np.array_equal(p['vert_w'][i], W[v])
    assert p['vert_dirs'].shape == (5, 3, 224) and p['vert_dirs'].dtype == np.float32
    assert np.array_equal(p['parents'], np.asarray(M['parents'], np.int32))
    ps = pack_smpl_model(M)                 # the forward kernel's rest joints
    assert np.array_equal(p['j_template'], ps['j_template']) and np.array_equal(p['j_shapedirs'], ps['j_shapedirs'])
    # the blend of a tracked vertex is a row of the oracle's mesh
    case = FC.standard_case(B=2)
    est = case['est'].double()
    R = O.rot6d_to_rotmat(est[:, 3:147].reshape(-1, 6)).view(2, 24, 3, 3)
    F = torch.cat([torch.ones(2, 1, dtype=FC.F64), est[:, 147:], (R[:, 1:] - torch.eye(3, dtype=FC.F64)).reshape(2, 207)], dim=1)
    vposed = torch.einsum('bk,ick->bic', F, torch.from_numpy(p['vert_dirs'][:, :, :218]).double())
    vshaped = torch.from_numpy(vt).double()[None] + torch.einsum('bl,mkl->bmk', est[:, 147:], torch.from_numpy(sd).double())
    want = vshaped + (F[:, 11:] @ torch.from_numpy(pd).double()).view(2, -1, 3)
    assert float((vposed - want[:, p['vertex_ids'].tolist()]).abs().max()) < 1e-12


def test_pack_fit_model_keypoint_sets_and_errors():
    M = FC.MODEL
    p = pack_fit_model(M, [0, 23, ('vertex', 0), ('vertex', 6889), 24, ('vertex', 0)])
    ev0 = int(M['extra_vertex_ids'][0])
    assert p['vertex_ids'].tolist() == [0, 6889] + ([ev0] if ev0 not in (0, 6889) else [])
    assert p['kp_src'].tolist()[:4] == [0, 23, 24, 25] and p['kp_src'][5] == 24
    p0 = pack_fit_model(M, list(range(24)) + list(range(8)))
    assert p0['n_verts'] == 0 and p0['n_kp'] == 32 and p0['vert_dirs'].shape == (0, 3, 224)
    with pytest.raises(ValueError):
        pack_fit_model(M, [0, 45])                                       # a regressed joint needs the mesh
    with pytest.raises(ValueError):
        pack_fit_model(M, [89])
    with pytest.raises(ValueError):
        pack_fit_model(M, list(range(24)) + list(range(9)))              # 33 keypoints
    with pytest.raises(ValueError):
        pack_fit_model(M, [('vertex', i) for i in range(17)])            # 17 distinct vertices
    assert pack_fit_model(M, [('vertex', i % 16) for i in range(32)])['n_verts'] == 16
