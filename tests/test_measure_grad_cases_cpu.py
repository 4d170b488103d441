"""CPU: the float64 restatement of the measurement gradients (tests/measure_grad_cases.py) checked against itself -- it is the oracle of
tests/test_gpu_measure_bwd.py, so it is held to things that do not depend on it: central finite differences of measure_cases.oracle_body,
Euler's identity for homogeneous functions, closed forms on a prism and a sphere, and the two formulations (scatter, CSR gather) against the
autograd gradient."""
import numpy as np
import pytest

import measure_cases as MC
import measure_grad_cases as GC
import straps_amd
from measure_cases import AREA, EXTENT, GIRTH, PATH, VOLUME, measurement
from straps_amd.nmr_renderer import vertex_face_table

SOUPS = {'a': (300, 1025, 5, 0), 'b': (2049, 513, 3, 1)}      # (nverts, nfaces, n_points, seed): the 32-measurement soup cases


def _soup(key):
    nverts, nfaces, n_points, seed = SOUPS[key]
    verts, points, faces, parts = MC.soup(1, nverts, nfaces, n_points, seed)
    meas = MC.mixed_measurements(32, nverts, n_points, seed=seed)
    GC.assert_conditions(verts, points, faces, parts, meas)
    return verts, points, faces, parts, meas


@pytest.mark.parametrize('key', sorted(SOUPS))
def test_forward_agrees_with_the_value_oracle(key):
    verts, points, faces, parts, meas = _soup(key)
    want, S = MC.oracle(verts, points, faces, parts, meas)
    got, _, _ = GC.oracle_jacobian(verts[0], points[0], faces, parts, meas)
    assert (np.abs(got - want[0]) <= 1e-13 * S[0] + 1e-300).all()
    assert (want[0][[m for m, q in enumerate(meas) if q['kind'] == GIRTH and q['part_mask'] == 0]] > 0).any()


def test_oracle_vs_central_finite_differences():
    """every coordinate of a small soup, every kind; step 1e-6 m, below the 1e-5 m that assert_conditions keeps free round every plane"""
    nverts, n_points = 40, 3
    verts, points, faces, parts = MC.soup(1, nverts, 90, n_points, seed=7)
    meas = MC.mixed_measurements(15, nverts, n_points, seed=7)
    GC.assert_conditions(verts, points, faces, parts, meas)
    v64, p64 = verts[0].astype(np.float64), points[0].astype(np.float64)
    dirs = [dict(q, dir=[float(x) for x in q['dir']]) for q in meas]
    _, JV, JP = GC.oracle_jacobian(v64, p64, faces, parts, dirs, inputs=np.float64)
    h = 1e-6
    fd_v, fd_p = np.zeros_like(JV), np.zeros_like(JP)
    for arr, fd in ((v64, fd_v), (p64, fd_p)):
        for i in range(arr.shape[0]):
            for c in range(3):
                keep = arr[i, c]
                arr[i, c] = keep + h
                up = MC.oracle_body(v64, p64, faces, parts, dirs, inputs=np.float64)[0]
                arr[i, c] = keep - h
                dn = MC.oracle_body(v64, p64, faces, parts, dirs, inputs=np.float64)[0]
                arr[i, c] = keep
                fd[:, i, c] = (up - dn) / (2 * h)
    for m, q in enumerate(meas):
        scale = max(np.abs(JV[m]).max(), np.abs(JP[m]).max())
        assert scale > 0, 'measurement %d has no gradient' % m
        err = max(np.abs(fd_v[m] - JV[m]).max(), np.abs(fd_p[m] - JP[m]).max())
        assert err <= 1e-6 * scale, 'measurement %d (kind %d): finite differences differ by %.3g of the largest entry' % (m, q['kind'], err / scale)


@pytest.mark.parametrize('key', sorted(SOUPS))
def test_eulers_identity(key):
    """a measurement is homogeneous in (vertices, anchor points) of degree 3 (VOLUME), 2 (AREA) or 1: sum p . dvalue/dp = degree x value"""
    verts, points, faces, parts, meas = _soup(key)
    vals, JV, JP = GC.oracle_jacobian(verts[0], points[0], faces, parts, meas)
    _, S = MC.oracle(verts, points, faces, parts, meas)
    v64, p64 = verts[0].astype(np.float64), points[0].astype(np.float64)
    for m, q in enumerate(meas):
        deg = {VOLUME: 3, AREA: 2}.get(q['kind'], 1)
        lhs = (v64 * JV[m]).sum() + (p64 * JP[m]).sum()
        mag = np.abs(v64 * JV[m]).sum() + np.abs(p64 * JP[m]).sum()
        assert abs(lhs - deg * vals[m]) <= 1e-13 * (mag + S[0, m]) + 1e-300, (m, q['kind'], lhs, deg * vals[m])


def test_closed_forms_on_a_prism_and_a_sphere():
    n, r, hgt = 12, 0.4, 1.3
    v, f, parts = MC.prism(n, r, hgt, centre=(0.1, -0.2, 0.05))
    point = np.array([[0.3, 0.1, -0.2]])
    meas = [measurement(VOLUME), measurement(VOLUME, (v.shape[0],)), measurement(GIRTH, (v.shape[0],), (0, 1, 0)), measurement(AREA, part_mask=1 << 1)]
    vals, JV, JP = GC.oracle_jacobian(v, point, f, parts, meas, inputs=np.float64)
    volume = 0.5 * n * r * r * np.sin(2 * np.pi / n) * hgt
    assert abs(vals[0] - volume) <= 1e-13 and abs(vals[1] - volume) <= 1e-13
    # uniform scale about the prism's centre: d volume / d s at s = 1 is 3 V
    c = np.array([0.1, -0.2, 0.05])
    assert abs(((v - c) * JV[0]).sum() - 3 * volume) <= 1e-13
    # the centre `about` of a closed mesh does not matter
    assert np.abs(JP[1]).max() <= 1e-14
    # girth = the perimeter 2 n r sin(pi / n): d / dr moves every ring vertex radially
    radial = np.zeros_like(v)
    phi = 2 * np.pi * np.arange(n) / n
    radial[:n] = radial[n:2 * n] = np.stack([np.cos(phi), np.zeros(n), np.sin(phi)], 1)
    assert abs(vals[2] - 2 * n * r * np.sin(np.pi / n)) <= 1e-13
    assert abs((radial * JV[2]).sum() - 2 * n * np.sin(np.pi / n)) <= 1e-13
    # side area n * (2 r sin(pi / n)) * h: d / dr
    assert abs((radial * JV[3]).sum() - 2 * n * np.sin(np.pi / n) * hgt) <= 1e-13
    # a sphere: volume w.r.t. a uniform scale, and the centre again
    sv, sf = MC.sphere(9, 14, r=0.7, centre=(0.2, 0.1, -0.3))
    svals, sJV, sJP = GC.oracle_jacobian(sv, point, sf, None, [measurement(VOLUME), measurement(VOLUME, (sv.shape[0],))], inputs=np.float64)
    assert abs(((sv - [0.2, 0.1, -0.3]) * sJV[0]).sum() - 3 * svals[0]) <= 1e-13 and svals[0] > 0.9 * 4 / 3 * np.pi * 0.7 ** 3 * 0.9
    assert np.abs(sJP[1]).max() <= 1e-14


@pytest.mark.parametrize('key', sorted(SOUPS))
def test_scatter_and_csr_gather_equal_the_autograd_gradient(key):
    verts, points, faces, parts, meas = _soup(key)
    # repeated and out-of-range indices take part: the table lists a face once per vertex and not at all when an index is out of range
    faces = np.concatenate([faces, [[5, 5, 9], [7, 7, 7], [1, 2, verts.shape[1]], [-1, 3, 4]]]).astype(np.int32)
    parts = np.concatenate([parts, [1, 2, 1, 1]]).astype(np.uint8)
    GC.assert_conditions(verts, points, faces, parts, meas)
    dout = GC.random_dout(1, len(meas), seed=3)
    assert (dout == 0).any() and (dout < 0).any()
    want_v, want_p = GC.oracle_grad_body(verts[0], points[0], faces, parts, meas, dout[0])
    sv, sp, S_v, S_p = GC.scatter(verts[0], points[0], faces, parts, meas, dout[0])
    off, vf = vertex_face_table(faces, verts.shape[1])
    gv, gp, G_v, G_p = GC.gather(verts[0], points[0], faces, parts, meas, dout[0], off, vf)
    # 1e-15: coordinates are below 1 m, so a product rounds by at most 2^-53, and a term that is exactly zero in exact arithmetic (the corner of
    # [5, 5, 9] that faces the repeated pair: q x q) comes out of autograd as a difference of two such products, not as 0
    for got_v, got_p in ((sv, sp), (gv, gp)):
        assert (np.abs(got_v - want_v) <= 1e-12 * S_v + 1e-15).all() and (np.abs(got_p - want_p) <= 1e-12 * S_p + 1e-15).all()
    assert np.allclose(G_v, S_v, rtol=1e-12, atol=0) and np.allclose(G_p, S_p, rtol=1e-12, atol=0)
    assert (S_v > 0).any() and (S_p > 0).any() and (np.abs(want_v) <= S_v * (1 + 1e-12) + 1e-15).all()


def test_extent_tie_goes_to_the_lowest_index_and_degenerate_terms_add_nothing():
    verts = np.array([[[0, 1, 0], [1, 1, 0], [0, -1, 0], [2, -1, 0], [0, 0, 0], [0, 0, 0]]], np.float32)
    faces = np.array([[4, 5, 4], [0, 1, 2]], np.int32)                       # a face of zero area, and a real one
    meas = [measurement(EXTENT, direction=(0, 1, 0)), measurement(AREA), measurement(PATH, (4, 5, 0))]
    GC.assert_conditions(verts, None, faces, None, meas, allow_extent_ties=True)
    gv, _ = GC.oracle_grad_body(verts[0], None, faces, None, meas, [1.0, 0.0, 0.0])
    assert gv[0].tolist() == [0, 1, 0] and gv[2].tolist() == [0, -1, 0] and not gv[[1, 3, 4, 5]].any()
    gv, _ = GC.oracle_grad_body(verts[0], None, faces, None, meas, [0.0, 1.0, 1.0])
    sv, _, _, _ = GC.scatter(verts[0], None, faces, None, meas, [0.0, 1.0, 1.0])
    assert np.isfinite(gv).all() and np.allclose(gv, sv, rtol=0, atol=1e-15) and gv[4].tolist() == [0, 0, 0] and gv[5].tolist() == [0, -1, 0]


def test_synthetic_bodies_meet_the_conditions():
    b = MC.bodies(betas_seed=1)      # (the bodies of the GPU test; seed 0 puts a vertex of body 2 at 1.7e-6 m from the upper-arm plane)
    meas = MC.from_specs(list(straps_amd.default_measurements().values()), b['verts'].shape[1])
    GC.assert_conditions(b['verts'], b['joints'], b['faces'], b['face_parts'], meas)
