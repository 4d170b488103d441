"""CPU: the float64 reference of the silhouette fit (tests/silfit_cases.py) is itself checked -- the brute-force distance transform against
a two-pass restatement, the autograd gradient against central differences, the input conditions of every energy case, and the float64
composed fit of the standard trajectory case, whose outcome is the condition of the GPU test's bound."""
import numpy as np
import pytest
import torch

import silfit_cases as SC
from smpl_cases import cpu_threads


@pytest.fixture(scope='module', autouse=True)
def _threads():
    torch.set_num_threads(cpu_threads())


@pytest.mark.parametrize('wh', [1, 2, 3, 16, 17, 64, 65, 256])
def test_brute_force_transform_equals_two_pass(wh):
    for name, m in SC.mask_cases(wh).items():
        want = SC.reference_d2(wh, name)
        assert want.dtype == np.int32 and np.array_equal(want, SC.two_pass_d2(m)), (wh, name)
        assert (want[m != 0] == 0).all()
        if not m.any():
            assert (want == 2 * wh * wh).all()
        else:
            assert want.max() <= 2 * (wh - 1) ** 2 < 2 * wh * wh


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


def test_float64_fit_of_the_standard_trajectory_case_reaches_a_quarter():
    case = SC.trajectory_case()
    assert all(m.any() for m in case['masks'])
    _, terms = SC.trajectory_reference()
    sil = terms[:, :, 1] + terms[:, :, 2]
    ratio = sil[-1] / sil[0]
    print('silhouette energy, start -> end:', sil[0].tolist(), sil[-1].tolist(), 'ratio', ratio.tolist())
    assert bool((ratio < 0.25).all()), ratio
