"""CPU: the float64 restatement of the tape-girth gradient (tests/tape_grad_cases.py) checked against itself -- the values against
tests/tape_cases.py, the closed-form scatter against autograd, Euler homogeneity, translation invariance, central finite differences -- and
the input conditions that the GPU tests rely on."""
import numpy as np
import pytest
import torch

import measure_cases as MC
import tape_cases as TC
import tape_grad_cases as TG
from straps_amd import measure
from tape_cases import HULL

CASES = TC.gpu_cases()


def _one_hot(m, M):
    d = np.zeros(M)
    d[m] = 1.0
    return d


@pytest.mark.parametrize('name', sorted(CASES))
def test_values_scatter_homogeneity_and_translation(name):
    verts, points, f, p, meas = CASES[name]
    TG.assert_conditions(verts, points, f, p, meas)
    want, _, _ = TC.oracle(verts, points, f, p, meas)
    M = len(meas)
    hull_grads = 0
    for b in range(3):
        V, P = verts[b].astype(np.float64), points[b].astype(np.float64)
        for m in range(M):
            vals, gv, gp = TG.oracle_grad_body(verts[b], points[b], f, p, meas, _one_hot(m, M))
            assert abs(vals[m] - want[b, m]) <= 1e-12 * abs(want[b, m]), (b, m, vals[m], want[b, m])
            # the closed forms against autograd: the module's margin, 1e-10 S
            sv, sp, Sv, Sp = TG.scatter(verts[b], points[b], f, p, meas, _one_hot(m, M))
            assert (np.abs(sv - gv) <= 1e-10 * Sv).all() and (np.abs(sp - gp) <= 1e-10 * Sp).all(), (b, m)
            # Euler: the value is homogeneous of degree 1 when vertices and points scale together
            euler = (gv * V).sum() + (gp * P).sum()
            assert abs(euler - vals[m]) <= 1e-12 * max(abs(vals[m]), (np.abs(gv * V)).sum() + (np.abs(gp * P)).sum()), (b, m, euler, vals[m])
            # translation of vertices and points together changes nothing
            total = gv.sum(0) + gp.sum(0)
            assert (np.abs(total) <= 1e-12 * max(1.0, np.abs(gv).sum() + np.abs(gp).sum())).all(), (b, m, total)
            hull_grads += meas[m]['kind'] == HULL and bool(gv.any())
    assert hull_grads >= 3


@pytest.mark.parametrize('name', sorted(CASES))
def test_finite_differences(name):
    """central differences, h = 1e-6, on float64 inputs; the bar is 1e-5 of the largest entry (the O(h) term comes from the jump of the second
    derivative at collinear points)"""
    verts, points, f, p, meas = CASES[name]
    h, M = 1e-6, len(meas)
    worst = 0.0
    for b in range(3):
        V0, P0 = verts[b].astype(np.float64), points[b].astype(np.float64)

        def values(V, P):
            with torch.no_grad():
                return np.array([float(x) for x in TG.values_torch(torch.from_numpy(V), torch.from_numpy(P), f, p, meas)])
        fd_v, fd_p = np.zeros((M,) + V0.shape), np.zeros((M,) + P0.shape)
        for arr, fd, which in ((V0, fd_v, 0), (P0, fd_p, 1)):
            for i in range(arr.shape[0]):
                for c in range(3):
                    hi, lo = arr.copy(), arr.copy()
                    hi[i, c] += h
                    lo[i, c] -= h
                    fd[:, i, c] = (values(*((hi, P0) if which == 0 else (V0, hi))) - values(*((lo, P0) if which == 0 else (V0, lo)))) / (2 * h)
        for m in range(M):
            _, gv, gp = TG.oracle_grad_body(V0, P0, f, p, meas, _one_hot(m, M), inputs=np.float64)
            top = max(np.abs(gv).max(), np.abs(gp).max())
            err = max(np.abs(fd_v[m] - gv).max(), np.abs(fd_p[m] - gp).max())
            if top > 0:
                worst = max(worst, err / top)
            assert err <= 1e-5 * top, (b, m, err, top)
    print('%s: worst finite-difference error %.3g of the largest entry' % (name, worst))


def test_special_rows():
    """dout == 0 adds nothing even where the row is NaN; a NaN HULL row puts NaN into its anchor[0] alone; a SECTION propagates"""
    verts, points, f, p, meas = CASES['prism 7']
    v = verts[0].copy()
    v[3, 1] = np.inf
    M = len(meas)
    vals, gv, gp = TG.oracle_grad_body(v, points[0], f, p, meas, _one_hot(0, M))
    assert np.isnan(vals[0]) and np.isnan(gp[0]).all() and not np.isnan(gv).any() and not np.isnan(gp[1:]).any() and not gv.any()
    sv, sp, _, _ = TG.scatter(v, points[0], f, p, meas, _one_hot(0, M))
    assert np.isnan(sp[0]).all() and not sv.any()
    _, gv, gp = TG.oracle_grad_body(v, points[0], f, p, meas, np.zeros(M))
    assert not gv.any() and not gp.any()


@pytest.mark.parametrize('k', (1, 2, 63, 64, 65, 255, 256, 257, 513))
def test_conditions_of_the_compaction_cases(k):
    TG.assert_conditions(*TC.compaction_case(k))


@pytest.mark.parametrize('seed', (0, 1))
def test_conditions_of_the_full_size_bodies(seed):
    """MC.bodies(betas_seed=0 / 1) pass the plane condition at 1e-6 m for tape_measurements() and posed_measurements()"""
    b = MC.bodies(betas_seed=seed)
    for specs in (measure.tape_measurements(), measure.posed_measurements()):
        arr, _ = measure.tape_structs(list(specs.values()), 6890)
        meas = [{'kind': q.kind, 'anchor': list(q.anchor), 'dir': list(q.dir), 'part_mask': q.part_mask} for q in arr]
        plane, corner = TG.worst_distances(b['verts'], b['joints'], b['faces'], b['face_parts'], meas)
        print('betas_seed %d, %d measurements: worst plane distance %.3g m, closest corners of different edges %.3g m' % (seed, len(meas), plane, corner))
        assert plane >= TG.MIN_PLANE_DISTANCE
