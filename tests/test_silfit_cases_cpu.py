"""CPU: the float64 reference of the silhouette fit (tests/silfit_cases.py) is itself checked -- the brute-force distance transform against
a row-blocked two-pass restatement (all masks up to 257 pixels; sparse masks at 1000 and 1024, which licenses the two-pass as the GPU tests'
reference above 257), the autograd gradient against central differences, the input conditions of every energy case, the paths of
csrc/silfit.hip that the energy cases reach, and the float64 composed fit of the standard trajectory case, whose outcome is the condition of
the GPU test's bound."""
import numpy as np
import pytest
import torch

import silfit_cases as SC
from smpl_cases import cpu_threads


@pytest.fixture(scope='module', autouse=True)
def _threads():
    torch.set_num_threads(cpu_threads())


def _check_transform(wh, name, m, got):
    want = SC.reference_d2(wh, name)
    assert want.dtype == np.int32 and got.dtype == np.int32 and np.array_equal(want, got), (wh, name)
    assert (want[m != 0] == 0).all()
    if not m.any():
        assert (want == 2 * wh * wh).all()
    else:
        assert want.max() <= 2 * (wh - 1) ** 2 < 2 * wh * wh


@pytest.mark.parametrize('wh', [1, 2, 3, 16, 17, 64, 65, 256, 257])
def test_brute_force_transform_equals_two_pass(wh):
    assert wh <= SC.BRUTE_MAX_WH
    for name, m in SC.mask_cases(wh).items():
        _check_transform(wh, name, m, SC.two_pass_d2(m))


@pytest.mark.parametrize('wh', [1000, 1024])
def test_brute_force_transform_equals_two_pass_on_sparse_masks_at_the_largest_sizes(wh):
    """what licenses the row-blocked two-pass as the GPU tests' reference above 257 pixels: on masks sparse enough for brute force (about 1e8
    integer operations each) the two agree exactly, at a size that is no multiple of 64 and at the limit"""
    cases = SC.sparse_mask_cases(wh)
    assert tuple(cases) == SC.SPARSE and 50 <= int((cases['rand1e4'] != 0).sum()) <= 200
    for name, m in cases.items():
        _check_transform(wh, name, m, SC.reference_d2_two_pass(wh, name))


def test_row_blocking_changes_nothing():
    """the blocked row pass against all rows at once, and against a block size that does not divide wh"""
    m = SC.mask_cases(65)
    whole = {k: SC.two_pass_d2(v) for k, v in m.items()}
    keep = SC.ROW_BLOCK
    try:
        for block in (1, 7, 65, 1000):
            SC.ROW_BLOCK = block
            for k, v in m.items():
                assert np.array_equal(SC.two_pass_d2(v), whole[k]), (block, k)
    finally:
        SC.ROW_BLOCK = keep


def test_autograd_gradient_matches_central_differences():
    case = SC.energy_case(12, 8, 2, 0.5, 2, 6900)
    assert SC.conditions_hold(SC.input_conditions(case))
    v, c = case['verts'].double(), case['cam'].double()
    args = (case['masks'], case['d2'], case['lattice'], case['tau'])
    e2, gv, gc, near = SC.energies_grad(v, c, *args, 3.0, 2.0)
    assert float(e2[:, 0].min()) > 0 and float(e2[:, 1].max()) > 0

    def total(v_, c_):
        ei, eo, _ = SC.energies(v_, c_, *args, nearest=near)
        return 3.0 * ei + 2.0 * eo
    h = 1e-6
    worst = 0.0
    for b in range(2):
        for i in range(12):
            for k in range(2):
                d = torch.zeros_like(v)
                d[b, i, k] = h
                fd = float((total(v + d, c) - total(v - d, c))[b]) / (2 * h)
                worst = max(worst, abs(fd - float(gv[b, i, k])))
        for k in range(3):
            d = torch.zeros_like(c)
            d[b, k] = h
            fd = float((total(v, c + d) - total(v, c - d))[b]) / (2 * h)
            worst = max(worst, abs(fd - float(gc[b, k])) / max(1.0, float(gc[b].abs().max())))
    assert not bool(gv[:, :, 2].any())
    assert worst < 1e-6 * max(1.0, float(gv.abs().max())), worst


@pytest.mark.parametrize('name', sorted(SC.ENERGY_SPECS))
def test_energy_cases_meet_the_input_conditions(name):
    nv, wh, lat, tau, B, seed, kw = SC.ENERGY_SPECS[name]
    case = SC.get_energy_case(name)
    cond = case['conditions']
    print(name, 'seed', case['seed'], cond)
    assert cond['cell'] > 1e-3 and cond['tau'] > 1e-3 and cond['gap'] > 1e-4
    # nothing was dropped: every vertex and every lattice point of the stated sizes takes part
    assert tuple(case['verts'].shape) == (B, nv, 3) and cond['verts'] == B * nv
    nl = -(-wh // min(lat, wh))
    want_pts = sum(int(SC.lattice_points(case['masks'][b], lat)[1].sum()) for b in range(B) if case['masks'][b].any())
    assert cond['points'] == want_pts and SC.lattice_points(case['masks'][0], lat)[0].shape[0] == nl * nl
    if kw.get('empty_body') is not None:
        assert not case['masks'][kw['empty_body']].any()
    if kw.get('odd_only_body') is not None:
        b = kw['odd_only_body']
        assert case['masks'][b].any() and not bool(SC.lattice_points(case['masks'][b], lat)[1].any())
    if kw.get('tie'):
        i, j = case['tie']
        assert torch.equal(case['verts'][0, i], case['verts'][0, j])
        near = SC.energies(case['verts'].double(), case['cam'].double(), case['masks'], case['d2'], lat, tau)[2]
        assert bool((near[0] == i).any()) and not bool((near[0] == j).any())      # the pair is somebody's nearest, and the lower index is reported
    if nv > 8:      # vertices beyond every side and corner
        g = SC.grid_coords(case['verts'].double(), case['cam'].double(), wh)[:, :8]
        out = ((g < 0) | (g > wh - 1)).sum(dim=2)
        assert bool((out[:, :4] == 1).all()) and bool((out[:, 4:] == 2).all())


PATHS = {
    'one vertex tile': lambda f: f['vertex_tiles'] == 1,
    'more than one vertex tile': lambda f: f['vertex_tiles'] > 1,
    'one gather tile': lambda f: f['gather_tiles'] == 1,
    'more than one gather tile': lambda f: f['gather_tiles'] > 1,
    'no more chunks than workgroups': lambda f: f['chunks'] <= SC.MAX_WORKGROUPS,
    'more chunks than workgroups, ragged trips': lambda f: f['chunks'] > SC.MAX_WORKGROUPS and f['trips'][0] < f['trips'][1],
    'more chunks than workgroups, equal trips': lambda f: f['chunks'] > SC.MAX_WORKGROUPS and f['trips'][0] == f['trips'][1],
    'more chunks than workgroups with more than one vertex tile': lambda f: f['chunks'] > SC.MAX_WORKGROUPS and f['vertex_tiles'] > 1,
    'more than 256 partial sums in the finish': lambda f: f['finish_trips'] > 1,
    'wh above 256': lambda f: f['wh'] > 256,
    'wh = 1024': lambda f: f['wh'] == 1024,
}


def test_path_facts():
    assert (SC.LANES, SC.VERTEX_TILE, SC.GATHER_TILE, SC.MAX_WORKGROUPS) == (256, 6912, 2048, 32)
    f = SC.path_facts((6912, 256, 2))                   # 16384 points: 64 chunks, two whole trips
    assert f == {'vertex_tiles': 1, 'gather_tiles': 8, 'chunks': 64, 'trips': (2, 2), 'finish_trips': 1, 'wh': 256}
    f = SC.path_facts((6913, 91, 1))                    # 8281 points: 33 chunks, workgroup 0 takes two
    assert f == {'vertex_tiles': 2, 'gather_tiles': 5, 'chunks': 33, 'trips': (1, 2), 'finish_trips': 1, 'wh': 91}
    f = SC.path_facts((65537, 16, 17))                  # a lattice above wh - 1: the single point
    assert f == {'vertex_tiles': 10, 'gather_tiles': 1, 'chunks': 1, 'trips': (1, 1), 'finish_trips': 2, 'wh': 16}
    assert SC.path_facts((65536, 16, 4))['finish_trips'] == 1


@pytest.mark.parametrize('path', sorted(PATHS))
def test_energy_cases_reach_every_path(path):
    """every path of csrc/silfit.hip's energy kernels that depends on the sizes is taken by at least one case of ENERGY_SPECS"""
    reached = [name for name, spec in SC.ENERGY_SPECS.items() if PATHS[path](SC.path_facts(spec))]
    print(path, '<-', reached)
    assert reached, 'no case of ENERGY_SPECS reaches: ' + path


def test_float64_fit_of_the_standard_trajectory_case_reaches_a_quarter():
    case = SC.trajectory_case()
    assert all(m.any() for m in case['masks'])
    _, terms = SC.trajectory_reference()
    sil = terms[:, :, 1] + terms[:, :, 2]
    ratio = sil[-1] / sil[0]
    print('silhouette energy, start -> end:', sil[0].tolist(), sil[-1].tolist(), 'ratio', ratio.tolist())
    assert bool((ratio < 0.25).all()), ratio
