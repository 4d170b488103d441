"""CPU: the float64 restatement of the measurements (tests/measure_cases.py) against closed forms on a regular prism, and the properties the
definitions promise: rigid-motion invariance, additivity of girths over a partition of the faces, no tie case at d == 0, 0 for a plane that
misses, faces with an out-of-range index ignored."""
import numpy as np
import pytest

import measure_cases as MC
from measure_cases import AREA, EXTENT, GIRTH, PATH, VOLUME, measurement

PRISMS = ((3, 0.7, 1.1), (4, 0.5, 2.0), (7, 0.31, 0.9), (32, 0.45, 1.7))


def _one(verts, faces, parts, q, points=None):
    v, s = MC.oracle_body(np.asarray(verts, np.float32), points, faces, parts, [q])
    return float(v[0])


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize('n,r,h', PRISMS)
def test_prism_closed_forms(n, r, h):
    # float64 vertices here: the closed forms are held to 1e-12, below the fp32 rounding of the coordinates
    v, f, parts = MC.prism(n, r, h, centre=(0.2, -0.1, 0.3))
    V = v.astype(np.float64)

    def one(q, points=None):
        return float(_oracle64(V, points, f, parts, [q])[0][0])
    assert _rel(one(measurement(VOLUME)), 0.5 * n * r * r * np.sin(2 * np.pi / n) * h) < 1e-12
    assert _rel(one(measurement(VOLUME, (5,))), 0.5 * n * r * r * np.sin(2 * np.pi / n) * h) < 1e-12            # about a vertex: the same, the surface is closed
    assert _rel(one(measurement(AREA)), n * 2 * r * np.sin(np.pi / n) * h + n * r * r * np.sin(2 * np.pi / n)) < 1e-12
    assert _rel(one(measurement(AREA, part_mask=1 << 1)), n * 2 * r * np.sin(np.pi / n) * h) < 1e-12             # the sides alone
    assert _rel(one(measurement(AREA, part_mask=(1 << 2) | (1 << 3))), n * r * r * np.sin(2 * np.pi / n)) < 1e-12      # the caps
    girth = 2 * n * r * np.sin(np.pi / n)
    for frac in (0.03, 0.25, 0.5, 0.77, 0.99):
        pts = np.array([[5.0, -0.1 - h / 2 + frac * h, -3.0]])                                                     # a point on the plane, anywhere
        for normal in ((0, 1, 0), (0, -2.5, 0)):
            assert _rel(one(measurement(GIRTH, (V.shape[0],), normal), pts), girth) < 1e-12, (frac, normal)
    assert _rel(one(measurement(EXTENT, direction=(0, 1, 0))), h) < 1e-12
    assert _rel(one(measurement(EXTENT, direction=(0, -3, 0))), 3 * h) < 1e-12
    if n % 2 == 0:
        assert _rel(one(measurement(EXTENT, direction=(1, 0, 0))), 2 * r) < 1e-12
    side = 2 * r * np.sin(np.pi / n)
    assert _rel(one(measurement(PATH, (0, 1))), side) < 1e-12
    assert _rel(one(measurement(PATH, (0, 1, n + 1))), side + h) < 1e-12
    assert _rel(one(measurement(PATH, (0, 1, n + 1, n))), 2 * side + h) < 1e-12
    assert _rel(one(measurement(PATH, (2 * n, 2 * n + 1, 0, -1))), h + np.sqrt(r * r + h * h)) < 1e-12          # centres, then a rim vertex; -1 ends it
    flipped = f[:, ::-1]
    assert _rel(float(_oracle64(V, None, flipped, parts, [measurement(VOLUME)])[0][0]), -0.5 * n * r * r * np.sin(2 * np.pi / n) * h) < 1e-12


def _oracle64(V, points, faces, parts, meas):
    return MC.oracle_body(V, points, faces, parts, meas, inputs=np.float64)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


@pytest.mark.parametrize('seed', (0, 1, 2))
def test_rigid_motion_invariance(seed):
    rng = np.random.RandomState(seed)
    v, f = MC.sphere(9, 11, 0.4, centre=(0.1, 0.2, -0.3))
    parts = (np.arange(f.shape[0]) % 3 + 1).astype(np.uint8)
    pts = rng.uniform(-0.2, 0.2, (2, 3)) + (0.1, 0.2, -0.3)
    normal = rng.normal(size=3)
    N = v.shape[0]
    meas = lambda nrm: [measurement(VOLUME), measurement(VOLUME, (N,), part_mask=0b0110), measurement(AREA, part_mask=0b1010),
                        measurement(GIRTH, (N,), nrm), measurement(GIRTH, (N + 1,), nrm, 0b0100), measurement(GIRTH, (7,), nrm),
                        measurement(PATH, (3, N, 20, N + 1))]
    R, t = _rotation(rng), rng.uniform(-1, 1, 3)
    a, Sa = _oracle64(v, pts, f, parts, meas(normal))
    b, _ = _oracle64(v.dot(R.T) + t, pts.dot(R.T) + t, f, parts, [dict(q, dir=list(R.dot(q['dir']))) for q in meas(normal)])
    # (measurement() rounds the normal to float32; its rotated image is handed over in float64, so both sides see the same plane)
    assert (a[2:] > 0).all() and a[0] > 0
    assert (np.abs(a - b) <= 1e-10 * np.maximum(np.abs(a), Sa)).all()


def test_girths_over_a_partition_add_up():
    b = MC.bodies()
    verts, joints, faces, parts = b['verts'][1], b['joints'][1], b['faces'], b['face_parts']
    N = verts.shape[0]
    labels = sorted(set(parts.tolist()))
    assert labels == [1, 2, 3, 4, 5, 6]
    for j, normal in ((0, (0, 1, 0)), (9, (0.2, 1, -0.1)), (18, (1, 0, 0))):
        whole = _one(verts, faces, parts, measurement(GIRTH, (N + j,), normal), joints)
        each = [_one(verts, faces, parts, measurement(GIRTH, (N + j,), normal, 1 << l), joints) for l in labels]
        assert whole > 0 and sum(e > 0 for e in each) >= 2
        assert abs(sum(each) - whole) <= 1e-12 * whole
        pair = _one(verts, faces, parts, measurement(GIRTH, (N + j,), normal, (1 << 1) | (1 << 6)), joints)
        assert abs(pair - each[0] - each[5]) <= 1e-12 * whole


def test_plane_through_a_vertex_is_no_tie_case():
    """d == 0 at mesh vertices (the ring of a sphere, and the anchor vertex itself): the girth equals the limit from either side"""
    v, f = MC.sphere(8, 12, 0.5)
    V = v.astype(np.float64)
    ring_vertex = 1 + 3 * 12 + 5                    # on the equator ring: y == 0 for the whole ring up to rounding; made exact below
    V[1 + 3 * 12:1 + 4 * 12, 1] = 0.0
    at = float(_oracle64(V, None, f, None, [measurement(GIRTH, (ring_vertex,), (0, 1, 0))])[0][0])
    assert at > 0
    for eps in (1e-11, -1e-11):
        near = float(_oracle64(V, np.array([[0.0, eps, 0.0]]), f, None, [measurement(GIRTH, (V.shape[0],), (0, 1, 0))])[0][0])
        assert abs(near - at) <= 1e-9 * at, eps
    assert _rel(at, 12 * 2 * 0.5 * np.sin(np.pi / 12)) < 1e-12          # the equator polygon
    # a tilted plane through one vertex only
    tilt = (0.3, 1.0, -0.2)
    at = float(_oracle64(V, None, f, None, [measurement(GIRTH, (ring_vertex,), tilt)])[0][0])
    for eps in (1e-11, -1e-11):
        p = V[ring_vertex] + eps * np.asarray(tilt)
        near = float(_oracle64(V, p[None], f, None, [measurement(GIRTH, (V.shape[0],), tilt)])[0][0])
        assert at > 0 and abs(near - at) <= 1e-9 * at, eps


def test_missed_plane_gives_zero_and_bad_faces_are_ignored():
    v, f, parts = MC.prism(6, 0.5, 1.0)
    v32 = v.astype(np.float32)
    above = np.array([[0.0, 0.75, 0.0]], np.float32)
    vals, S = MC.oracle_body(v32, above, f, parts, [measurement(GIRTH, (v.shape[0],), (0, 1, 0)), measurement(GIRTH, (0,), (0, 1, 0), 1 << 3),
                                                   measurement(AREA, part_mask=1 << 9), measurement(VOLUME, part_mask=1 << 31)])
    assert vals.tolist() == [0.0, 0.0, 0.0, 0.0] and S.tolist() == [0.0, 0.0, 0.0, 0.0] and not np.isnan(vals).any()
    meas = [measurement(VOLUME), measurement(AREA), measurement(GIRTH, (0,), (0.1, 1, 0)), measurement(EXTENT, direction=(0, 1, 0))]
    good, _ = MC.oracle_body(v32, None, f, parts, meas)
    bad_faces = np.concatenate([f, [[0, 1, v.shape[0]], [-1, 2, 3], [4, 1 << 30, 5]]]).astype(np.int32)
    bad, _ = MC.oracle_body(v32, None, bad_faces, np.concatenate([parts, [1, 1, 1]]).astype(np.uint8), meas)
    assert np.array_equal(good, bad)
    # a label >= 32 is never selected by a non-zero mask, and always by mask 0
    odd = parts.copy()
    odd[:4] = (32, 33, 64, 255)
    a = MC.oracle_body(v32, None, f, odd, [measurement(AREA, part_mask=0xffffffff), measurement(AREA)])[0]
    assert a[0] < a[1] and a[1] == good[1]
    assert np.array_equal(MC.selected_faces(f, odd, v.shape[0], 0xffffffff)[:4], [False] * 4) and MC.selected_faces(f, odd, v.shape[0], 0xffffffff)[4:].all()


def test_sphere_and_synthetic_bodies_are_well_formed():
    v, f = MC.sphere(24, 32, 0.5, centre=(0.1, 0.2, -0.3))
    pts = np.array([[0.1, 0.2 + 0.11, -0.3]], np.float32)
    vals, _ = MC.oracle_body(v.astype(np.float32), pts, f, None, [measurement(VOLUME), measurement(AREA), measurement(GIRTH, (v.shape[0],), (0, 1, 0)),
                                                                   measurement(EXTENT, direction=(0, 1, 0))])
    ball, circle = 4 / 3 * np.pi * 0.125, 2 * np.pi * np.sqrt(0.25 - 0.0121)
    assert 0.985 * ball < vals[0] < ball and 0.98 * np.pi < vals[1] < np.pi and 0.99 * circle < vals[2] < circle and abs(vals[3] - 1.0) < 1e-6
    import straps_amd
    from straps_amd import measure
    b = MC.bodies()
    N = b['verts'].shape[1]
    specs = list(measure.default_measurements().values())
    vals, S = MC.oracle(b['verts'], b['joints'], b['faces'], b['face_parts'], MC.from_specs(specs, N))
    assert vals.shape == (3, 15) and np.isfinite(vals).all() and np.isfinite(S).all()
    names = list(measure.default_measurements())
    assert (vals[:, names.index('height')] > 1.5).all() and (vals[:, names.index('surface_area')] > 0).all()
    assert (vals[:, [names.index(n) for n in names if n.endswith('_girth') or '_girth_' in n]] > 0).all()
    assert (vals[:, [names.index(n) for n in names if 'length' in n or 'breadth' in n]] > 0).all()
    assert not np.array_equal(vals[0], vals[1])
