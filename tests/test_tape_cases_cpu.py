"""CPU: the float64 restatement of tests/tape_cases.py against closed forms (on float64 inputs, to 1e-12), against scipy's convex hull on
random point sets, the Lipschitz property the bar of the GPU tests rests on, and the input condition those tests rely on."""
import numpy as np
import pytest

import tape_cases as TC
from tape_cases import HULL, SECTION, tape

Y = (0.0, 1.0, 0.0)
F64 = dict(inputs=np.float64)


def _one(v, f, p, meas, points=None):
    return TC.oracle_body(v, points, f, p, meas, **F64)


@pytest.mark.parametrize('n', (3, 4, 5, 7, 64))
def test_regular_prism(n):
    """both girths of a convex section are the n-gon's perimeter 2 n r sin(pi / n), on a tilted plane included (then against each other)"""
    r = 0.37
    v, f, p = TC.prism(n, r, 1.0)
    o = np.array([[0.01, 0.05, -0.02]])
    val, S, cnt = _one(v, f, p, [tape(HULL, len(v), Y), tape(SECTION, len(v), Y), tape(HULL, len(v), (0.2, 1.0, 0.1)), tape(SECTION, len(v), (0.2, 1.0, 0.1))], o)
    want = 2 * n * r * np.sin(np.pi / n)
    assert abs(val[0] - want) <= 1e-12 * want and abs(val[1] - want) <= 1e-12 * want
    assert abs(val[2] - val[3]) <= 1e-12 * val[3] and val[2] > want
    assert cnt.tolist() == [4 * n] * 4 and S[1] == val[1] and S[0] > val[0]


def test_star_prism():
    """hull = the outer pentagon, section = 2n sqrt(R^2 + r^2 - 2 R r cos(pi / n))"""
    n, R, r = 5, 1.0, 0.4
    v, f, p = TC.star_prism(n, R, r, 1.0)
    val, _, cnt = _one(v, f, p, [tape(HULL, 4 * n, Y), tape(SECTION, 4 * n, Y)])      # anchored at the bottom centre (vertex 4n): d >= 0 everywhere, nothing is cut
    assert cnt.tolist() == [0, 0] and val.tolist() == [0.0, 0.0]
    o = np.zeros((1, 3))
    val, _, cnt = _one(v, f, p, [tape(HULL, len(v), Y), tape(SECTION, len(v), Y)], o)
    hull, section = 2 * n * R * np.sin(np.pi / n), 2 * n * np.sqrt(R * R + r * r - 2 * R * r * np.cos(np.pi / n))
    assert abs(val[0] - hull) <= 1e-12 * hull and abs(val[1] - section) <= 1e-12 * section and val[0] < val[1]
    assert abs(hull - 5.8779) < 1e-4 and abs(section - 7.1609) < 1e-4 and cnt.tolist() == [8 * n, 8 * n]


def test_two_prisms():
    """one tape round both: perimeter + 2 x the centre distance (the n-gons are translates, n odd or even); the section is two loops"""
    for n in (7, 4):
        r, dist = 0.3, 1.0
        v, f, p = TC.two_prisms(n, r, 1.0, dist)
        o = np.zeros((1, 3))
        val, _, cnt = _one(v, f, p, [tape(HULL, len(v), Y), tape(SECTION, len(v), Y), tape(HULL, len(v), Y, part_mask=1 << 1), tape(HULL, len(v), Y, part_mask=1 << 4)], o)
        per = 2 * n * r * np.sin(np.pi / n)
        assert abs(val[0] - (per + 2 * dist)) <= 1e-12 * (per + 2 * dist) and abs(val[1] - 2 * per) <= 1e-12 * per
        assert abs(val[2] - per) <= 1e-12 * per and abs(val[3] - per) <= 1e-12 * per and cnt.tolist() == [8 * n, 8 * n, 4 * n, 4 * n]
    assert abs((2 * 7 * 0.3 * np.sin(np.pi / 7) + 2.0) - 3.8223) < 1e-4


def test_collinear_single_and_empty():
    v, f, p = TC.sheet(5, 3, 2.0, 1.0)
    o = np.array([[0.3, 0.1, 0.0]])
    val, S, cnt = _one(v, f, p, [tape(HULL, len(v), Y), tape(SECTION, len(v), Y)], o)
    assert abs(val[0] - 4.0) <= 1e-12 and abs(val[1] - 2.0) <= 1e-12 and cnt[0] == cnt[1] == 20      # there and back; ten cut faces in the row of cells
    v, f, p = TC.one_face()
    val, S, cnt = _one(v, f, p, [tape(HULL, 3, Y), tape(SECTION, 3, Y), tape(HULL, 3, (0.0, 0.0, 0.0)), tape(HULL, 3, Y, toward=3), tape(HULL, 4, Y)],
                       np.array([[0.0, 0.0, 0.0], [0.0, 5.0, 0.0]]))
    seg = np.linalg.norm(np.array([1.0, 0.0, 0.25]) - np.array([-0.5, 0.0, 0.125]))
    assert abs(val[0] - 2 * seg) <= 1e-12 and abs(val[1] - seg) <= 1e-12 and cnt.tolist() == [2, 2, 0, 0, 0]
    assert val[2:].tolist() == [0.0, 0.0, 0.0] and S[2:].tolist() == [0.0, 0.0, 0.0]            # a zero normal (given, or A1 == A0) and a plane that misses
    # all points coincide: the hull of one point
    assert TC.hull_perimeter(np.array([[0.5, 0.25]] * 6)) == 0.0 and TC.hull_perimeter(np.zeros((0, 2))) == 0.0


def test_box_section_with_lexicographic_ties():
    v, f, p = TC.box_prism(5, 0.5, 1.0)
    val, _, cnt = _one(v, f, p, [tape(HULL, len(v), Y), tape(SECTION, len(v), Y)], np.zeros((1, 3)))
    assert abs(val[0] - 4.0) <= 1e-12 and abs(val[1] - 4.0) <= 1e-12 and cnt.tolist() == [80, 80]


def test_non_finite_points_make_a_hull_nan():
    v, f, p = TC.prism(5, 0.5, 1.0)
    v = v.copy()
    v[2, 0] = np.inf
    val, S, cnt = _one(v, f, p, [tape(HULL, len(v), Y), tape(SECTION, len(v), Y)], np.zeros((1, 3)))
    assert np.isnan(val).all() and cnt[0] == 20


def test_per_body_normal_equals_the_given_one():
    v, f, p = TC.prism(7, 0.5, 1.0)
    R = TC.rotation((1.0, 2.0, -0.5), 0.9)
    pts = np.array([[0.02, 0.1, 0.01], [0.02, 0.6, 0.01]])
    a = _one(v, f, p, [tape(HULL, len(v), Y), tape(HULL, len(v), toward=len(v) + 1)], pts)[0]
    b = _one(v @ R.T, f, p, [tape(HULL, len(v), toward=len(v) + 1), tape(HULL, len(v), R @ np.array(Y))], pts @ R.T)[0]
    want = 14 * 0.5 * np.sin(np.pi / 7)
    assert np.allclose([a[0], a[1], b[0], b[1]], want, rtol=1e-12, atol=0)


def test_basis_is_orthonormal_and_the_perimeter_does_not_depend_on_it():
    rng = np.random.RandomState(5)
    for n in ([0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -2.0], [1.0, 1.0, 1.0], [0.3, -0.2, 0.3], rng.randn(3), 1e-20 * rng.randn(3), 1e20 * rng.randn(3)):
        n = np.asarray(n)
        u, v = TC.basis(n)
        G = np.array([[u @ u, u @ v, u @ n], [v @ u, v @ v, v @ n]]) / np.array([1, 1, np.linalg.norm(n)])
        assert np.allclose(G, [[1, 0, 0], [0, 1, 0]], atol=1e-15)
    Q = rng.randn(40, 2)
    c, s = np.cos(0.7), np.sin(0.7)
    assert abs(TC.hull_perimeter(Q) - TC.hull_perimeter(Q @ np.array([[c, -s], [s, c]]))) <= 1e-13 * TC.hull_perimeter(Q)


def test_against_scipy_on_random_sets():
    from scipy.spatial import ConvexHull
    rng = np.random.RandomState(11)
    for trial in range(40):
        n = int(rng.randint(3, 200))
        Q = rng.randn(n, 2) * [1.0, rng.uniform(0.01, 3.0)]
        if trial % 4 == 0:
            Q = np.round(Q * 4) / 4                          # a lattice: many duplicates, equal u, collinear triples
        if trial % 5 == 0:
            Q = np.concatenate([Q, Q[::2]])
        if np.linalg.matrix_rank(Q - Q[0]) < 2:
            continue
        H = ConvexHull(Q)
        assert abs(TC.hull_perimeter(Q) - H.area) <= 1e-12 * H.area, trial            # (in two dimensions scipy's `area` is the perimeter)


def test_hull_perimeter_is_two_pi_lipschitz():
    """|perimeter(Q + E) - perimeter(Q)| <= 2 pi max |E_i|: the bar of the GPU tests rests on it"""
    rng = np.random.RandomState(3)
    worst = 0.0
    for trial in range(60):
        Q = rng.randn(int(rng.randint(1, 80)), 2) * [1.0, rng.uniform(0.0, 2.0)]
        if trial % 3 == 0:
            Q = np.round(Q * 2) / 2
        for eps in (1e-9, 1e-3, 0.5):
            E = rng.randn(*Q.shape)
            E *= eps * rng.uniform(0, 1, (Q.shape[0], 1)) / np.maximum(np.linalg.norm(E, axis=1, keepdims=True), 1e-300)
            dmax = np.linalg.norm(E, axis=1).max()
            diff = abs(TC.hull_perimeter(Q + E) - TC.hull_perimeter(Q))
            assert diff <= 2 * np.pi * dmax + 1e-13 * (1 + TC.hull_perimeter(Q)), (trial, eps)
            worst = max(worst, diff / (2 * np.pi * dmax))
    print('worst |difference| / (2 pi max displacement): %.3f' % worst)


def test_input_condition_of_the_gpu_cases():
    """in every case no vertex is closer to a plane than 1e-9 of the mesh size unless it lies on it exactly (d == 0): the sides, and with
    them `counts`, are then the same in any double evaluation of d"""
    cases = dict(TC.gpu_cases())
    for k in (63, 64, 65, 255, 256, 257, 513):
        cases['%d cut faces' % k] = TC.compaction_case(k)
        assert TC.oracle(*cases['%d cut faces' % k])[2].tolist() == [[2 * k, 2 * k]] * 3
    for name, (verts, points, f, p, meas) in cases.items():
        for b in range(verts.shape[0]):
            allp = np.concatenate([verts[b], points[b]]).astype(np.float64)
            size = np.abs(allp[:verts.shape[1]]).max()
            for q in meas:
                o = allp[q['anchor'][0]]
                n = allp[q['anchor'][1]] - o if q['anchor'][1] >= 0 else np.asarray(q['dir'], np.float64)
                if not n.any():
                    continue
                d = (allp[:verts.shape[1]] - o) @ n / np.linalg.norm(n)
                assert ((d == 0) | (np.abs(d) >= 1e-9 * size)).all(), (name, b, q)
