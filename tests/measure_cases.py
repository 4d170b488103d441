"""Float64 restatement of the measurements of csrc/measure.hip (include/straps_hip.h states the definitions) and the meshes its tests use.

A measurement is a dict {'kind', 'anchor' (four ints, -1 = none), 'dir' (three floats), 'part_mask'}; `measurement()` builds one.  The oracle
reads the fp32 vertices as they are, computes in numpy float64 and returns, per measurement, the value and S: the sum of the absolute values
of the terms it added (per face for VOLUME / AREA / GIRTH -- scaled as the value is --, |max| + |min| for EXTENT, per segment for PATH).  A
GPU result is held to 2^-23 |value| + 1e-10 S: both sides compute every term in double from the same fp32 inputs, so they differ by the
summation order and fused multiply-adds (at most about nfaces * 2^-52 * S) and by the one rounding to float.
"""
import numpy as np

VOLUME, AREA, EXTENT, GIRTH, PATH = range(5)
FACE_KINDS = (VOLUME, AREA, GIRTH)


def measurement(kind, anchor=(), direction=(0.0, 0.0, 0.0), part_mask=0):
    a = [int(x) for x in anchor] + [-1] * (4 - len(anchor))
    return {'kind': int(kind), 'anchor': a, 'dir': [float(np.float32(x)) for x in direction], 'part_mask': int(part_mask)}


def _anchor_point(verts, points, a):
    n = verts.shape[0]
    return (verts[a] if a < n else points[a - n]).astype(np.float64)


def selected_faces(faces, face_parts, nverts, part_mask):
    """-> bool [F]: all three indices in [0, nverts), and part_mask == 0 or (label < 32 and its bit is set)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    sel = ((faces >= 0) & (faces < nverts)).all(1)
    if part_mask:
        lab = np.asarray(face_parts, np.int64)
        sel &= (lab < 32) & (((np.int64(part_mask) >> np.minimum(lab, 31)) & 1) == 1)
    return sel


def girth_terms(P, o, n):
    """P [F,3,3] float64 corners, plane through o with normal n -> [F] section lengths (0 where the three sides agree).  The vertex alone on
    its side is `a` of both crossing edges: x = p_a + t (p_b - p_a), t = d_a / (d_a - d_b)."""
    d = (n[0] * (P[..., 0] - o[0]) + n[1] * (P[..., 1] - o[1])) + n[2] * (P[..., 2] - o[2])
    s = d >= 0
    cut = ~((s[:, 0] == s[:, 1]) & (s[:, 1] == s[:, 2]))
    lone = np.where(s[:, 1] == s[:, 2], 0, np.where(s[:, 0] == s[:, 2], 1, 2))
    out = np.zeros(P.shape[0])
    idx = np.nonzero(cut)[0]
    if idx.size:
        a = lone[idx]
        A, B, C = P[idx, a], P[idx, (a + 1) % 3], P[idx, (a + 2) % 3]
        da, db, dc = d[idx, a], d[idx, (a + 1) % 3], d[idx, (a + 2) % 3]
        with np.errstate(invalid='ignore', divide='ignore'):
            xb = A + (da / (da - db))[:, None] * (B - A)
            xc = A + (da / (da - dc))[:, None] * (C - A)
            out[idx] = np.sqrt(((xb - xc) ** 2).sum(1))
    return out


def oracle_body(verts, points, faces, face_parts, meas, inputs=np.float32):
    """one body: verts [N,3] float32, points [P,3] float32 or None -> (values [M] float64, S [M] float64).  inputs=np.float64 skips the
    rounding of coordinates and directions to fp32 (checks of the definitions against closed forms below fp32 resolution)."""
    verts = np.asarray(verts, inputs)
    points = None if points is None else np.asarray(points, inputs)
    N = verts.shape[0]
    V = verts.astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    vals, S = np.zeros(len(meas)), np.zeros(len(meas))
    with np.errstate(invalid='ignore'):
        for m, q in enumerate(meas):
            kind, anc, n = q['kind'], q['anchor'], np.asarray(q['dir'], inputs).astype(np.float64)
            if kind in FACE_KINDS:
                sel = selected_faces(faces, face_parts, N, q['part_mask'])
                P = V[faces[sel]]                                         # [f,3,3]
                if kind == VOLUME:
                    c = _anchor_point(verts, points, anc[0]) if anc[0] >= 0 else np.zeros(3)
                    r = P - c
                    t = (r[:, 0] * np.cross(r[:, 1], r[:, 2])).sum(1) / 6.0
                elif kind == AREA:
                    t = 0.5 * np.sqrt((np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) ** 2).sum(1))
                else:
                    t = girth_terms(P, _anchor_point(verts, points, anc[0]), n)
                vals[m], S[m] = t.sum(), np.abs(t).sum()
            elif kind == EXTENT:
                h = (n[0] * V[:, 0] + n[1] * V[:, 1]) + n[2] * V[:, 2]
                hi, lo = (np.nan, np.nan) if np.isnan(h).any() else (h.max(), h.min())
                vals[m], S[m] = hi - lo, abs(hi) + abs(lo)
            else:
                k = 0
                while k < 4 and anc[k] >= 0:
                    k += 1
                pts = [_anchor_point(verts, points, a) for a in anc[:k]]
                t = np.array([np.sqrt(((pts[i + 1] - pts[i]) ** 2).sum()) for i in range(k - 1)])
                vals[m], S[m] = t.sum(), np.abs(t).sum()
    return vals, S


def oracle(verts, points, faces, face_parts, meas):
    """a batch: verts [B,N,3], points [B,P,3] or None -> (values [B,M], S [B,M])"""
    res = [oracle_body(verts[b], None if points is None else points[b], faces, face_parts, meas) for b in range(verts.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def prism(n, r, h, centre=(0.0, 0.0, 0.0)):
    """closed regular n-gon prism, axis y, outward winding: vertices [bottom ring n | top ring n | bottom centre | top centre],
    faces [2n sides | n bottom cap | n top cap]; face_parts 1 for sides, 2 bottom, 3 top"""
    phi = 2 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(phi), np.zeros(n), r * np.sin(phi)], 1)
    lo, hi = np.array([0.0, -h / 2, 0.0]), np.array([0.0, h / 2, 0.0])
    v = np.concatenate([ring + lo, ring + hi, lo[None], hi[None]]) + np.asarray(centre, np.float64)
    f = []
    for j in range(n):
        k = (j + 1) % n
        f += [(j, n + j, k), (k, n + j, n + k)]
    f += [(2 * n, j, (j + 1) % n) for j in range(n)]
    f += [(2 * n + 1, n + (j + 1) % n, n + j) for j in range(n)]
    return v, np.array(f, np.int32), np.array([1] * (2 * n) + [2] * n + [3] * n, np.uint8)


def sphere(nlat, nlon, r=1.0, centre=(0.0, 0.0, 0.0)):
    """closed latitude / longitude sphere, poles on y, outward winding -> (verts float64 [2 + (nlat - 1) nlon, 3], faces int32)"""
    v = [(0.0, r, 0.0)]
    for i in range(1, nlat):
        th = np.pi * i / nlat
        v += [(r * np.sin(th) * np.cos(ph), r * np.cos(th), r * np.sin(th) * np.sin(ph)) for ph in 2 * np.pi * np.arange(nlon) / nlon]
    v.append((0.0, -r, 0.0))
    v = np.array(v) + np.asarray(centre, np.float64)
    ring = lambda i, j: 1 + (i - 1) * nlon + (j % nlon)
    f = [(0, ring(1, j + 1), ring(1, j)) for j in range(nlon)]
    for i in range(1, nlat - 1):
        for j in range(nlon):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            f += [(a, b, d), (a, d, c)]
    last = len(v) - 1
    f += [(last, ring(nlat - 1, j), ring(nlat - 1, j + 1)) for j in range(nlon)]
    return v, np.array(f, np.int32)


def soup(batch, nverts, nfaces, n_points=0, seed=0):
    """random triangle soup: verts [B,nverts,3] in a body-sized box, points [B,n_points,3] or None, faces with indices in [0, nverts)
    (repeated indices allowed), face_parts 0..7 with a few labels >= 32"""
    rng = np.random.RandomState(1000 + seed)
    verts = (rng.uniform(-1, 1, (batch, nverts, 3)) * [0.45, 0.85, 0.15]).astype(np.float32)
    points = (rng.uniform(-1, 1, (batch, n_points, 3)) * [0.4, 0.8, 0.1]).astype(np.float32) if n_points else None
    faces = rng.randint(0, nverts, (nfaces, 3)).astype(np.int32)
    parts = rng.randint(0, 8, nfaces)
    parts[rng.rand(nfaces) < 0.1] = rng.choice([32, 33, 200, 255])
    return verts, points, faces, parts.astype(np.uint8)


def mixed_measurements(n_meas, nverts, n_points, seed=0, with_parts=True):
    """n_meas measurements, the five kinds interleaved (m % 5), anchors on vertices and -- when there are any -- on points, PATHs with 2, 3
    and 4 anchors in turn, part masks on every other face-based one"""
    rng = np.random.RandomState(2000 + seed)
    n_anchor = nverts + n_points

    def anchor(i):
        if n_points and i % 2:
            return nverts + int(rng.randint(n_points)) if i % 4 == 1 else n_anchor - 1
        return int(rng.randint(nverts)) if i % 3 else (0 if i % 2 else nverts - 1)
    out = []
    for m in range(n_meas):
        kind, rnd = m % 5, m // 5
        mask = int(rng.randint(1, 256)) | (int(rng.randint(2)) << 31) if (with_parts and rnd % 2) else 0
        d = rng.uniform(-1, 1, 3) if rnd % 3 else np.eye(3)[rnd % 3 if rnd < 3 else (rnd // 3) % 3] * (2.0 if rnd % 2 else 1.0)
        if kind == VOLUME:
            out.append(measurement(VOLUME, () if rnd % 3 == 0 else (anchor(rnd),), part_mask=mask))
        elif kind == AREA:
            out.append(measurement(AREA, part_mask=mask))
        elif kind == EXTENT:
            out.append(measurement(EXTENT, direction=d))
        elif kind == GIRTH:
            out.append(measurement(GIRTH, (anchor(rnd + 1),), d, mask))
        else:
            out.append(measurement(PATH, [anchor(rnd + i) for i in range(2 + rnd % 3)]))
    return out


def single_measurements(nverts, n_points):
    """one measurement of each kind, for n_meas == 1 calls"""
    p = nverts + n_points - 1
    return [measurement(VOLUME), measurement(AREA), measurement(EXTENT, direction=(0.3, -1.0, 0.2)), measurement(GIRTH, (p,), (0.1, 1.0, -0.2)),
            measurement(PATH, (0, p))]


_BODIES = {}


def bodies(betas_seed=0, batch=3):
    """T-pose bodies of synthetic_smpl_model(0): template + shape directions at a few betas, and their 24 joints
    -> {'verts' [B,6890,3] float32, 'joints' [B,24,3] float32, 'faces', 'face_parts', 'betas'}"""
    key = (betas_seed, batch)
    if key not in _BODIES:
        import straps_amd
        model = straps_amd.synthetic_smpl_model(0)
        rng = np.random.RandomState(3000 + betas_seed)
        betas = np.concatenate([np.zeros((1, 10)), rng.uniform(-2, 2, (batch - 1, 10))])[:batch]
        v = model['v_template'].astype(np.float64)[None] + np.einsum('vcl,bl->bvc', model['shapedirs'].astype(np.float64), betas)
        verts = v.astype(np.float32)
        joints = np.einsum('jv,bvc->bjc', model['J_regressor'].astype(np.float64), verts.astype(np.float64)).astype(np.float32)
        _BODIES[key] = {'verts': verts, 'joints': joints, 'faces': model['faces'], 'face_parts': model['face_parts'], 'betas': betas.astype(np.float32)}
    return _BODIES[key]


def from_specs(specs, nverts):
    """measure.py specs -> the dicts of this module (('joint', j) -> nverts + j)"""
    out = []
    for s in specs:
        anc = [nverts + a[1] if isinstance(a, tuple) else a for a in s.anchors]
        out.append(measurement(s.kind, anc, s.direction, sum(1 << p for p in s.parts) if s.parts else 0))
    return out
