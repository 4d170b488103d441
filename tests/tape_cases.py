"""Float64 restatement of the tape-measure girths of csrc/measure_tape.hip (include/straps_hip.h states the definitions) and the meshes its
tests use.

A measurement is a dict {'kind' (HULL / SECTION), 'anchor' (two ints; anchor[1] == -1: the normal is 'dir'), 'dir', 'part_mask'}; `tape()`
builds one.  The oracle reads the fp32 vertices as they are and computes in numpy float64: the section points of measure_cases.girth_terms'
definition, the basis (u, v) the header prescribes, Andrew's monotone chain on the DISTINCT points, the perimeter.  Per measurement it returns
(value, S, count).  A GPU result is held to the module's bar 2^-23 |value| + 1e-10 S; for SECTION S is the sum of the terms, for HULL
S = perimeter + 2 pi max_q |q - o|: the perimeter of a convex hull is 2 pi-Lipschitz in the largest displacement of a point (it is the integral
of the support function over the directions), and the two computations displace points by a few double ulps.
"""
import numpy as np

import measure_cases as MC

HULL, SECTION = 0, 1


def tape(kind, anchor, direction=None, toward=-1, part_mask=0):
    d = (0.0, 0.0, 0.0) if direction is None else direction
    return {'kind': int(kind), 'anchor': [int(anchor), int(toward)], 'dir': [float(np.float32(x)) for x in d], 'part_mask': int(part_mask)}


def basis(n):
    """the header's construction: k = argmin |n_k| (first on a tie), a = e_k x n, u = a / |a|, w = n x u, v = w / |w|"""
    k = int(np.argmin(np.abs(n)))
    a = [np.array([0.0, -n[2], n[1]]), np.array([n[2], 0.0, -n[0]]), np.array([-n[1], n[0], 0.0])][k]
    u = a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    w = np.array([n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]])
    return u, w / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])


def section_points(P, o, n):
    """P [F,3,3] float64 corners -> X [c,2,3]: the two section points of every cut face, in face order"""
    d = (n[0] * (P[..., 0] - o[0]) + n[1] * (P[..., 1] - o[1])) + n[2] * (P[..., 2] - o[2])
    s = d >= 0
    cut = ~((s[:, 0] == s[:, 1]) & (s[:, 1] == s[:, 2]))
    idx = np.nonzero(cut)[0]
    if not idx.size:
        return np.zeros((0, 2, 3))
    a = np.where(s[:, 1] == s[:, 2], 0, np.where(s[:, 0] == s[:, 2], 1, 2))[idx]
    A, B, C = P[idx, a], P[idx, (a + 1) % 3], P[idx, (a + 2) % 3]
    da, db, dc = d[idx, a], d[idx, (a + 1) % 3], d[idx, (a + 2) % 3]
    with np.errstate(invalid='ignore', divide='ignore'):
        xb = A + (da / (da - db))[:, None] * (B - A)
        xc = A + (da / (da - dc))[:, None] * (C - A)
    return np.stack([xb, xc], 1)


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_perimeter(Q):
    """Q [n,2] finite -> perimeter of the convex hull: Andrew's monotone chain on the distinct points, collinear points dropped.  0 for none
    or one distinct point, twice the length for a collinear set."""
    pts = sorted(set((float(x), float(y)) for x, y in np.asarray(Q, np.float64).reshape(-1, 2)))
    if len(pts) < 2:
        return 0.0
    chains = []
    for seq in (pts, pts[::-1]):
        ch = []
        for p in seq:
            while len(ch) >= 2 and cross(ch[-2], ch[-1], p) <= 0:
                ch.pop()
            ch.append(p)
        chains.append(ch)
    poly = chains[0][:-1] + chains[1][:-1]
    return float(sum(np.hypot(poly[i][0] - poly[i - 1][0], poly[i][1] - poly[i - 1][1]) for i in range(len(poly))))


def oracle_body(verts, points, faces, face_parts, meas, inputs=np.float32):
    """one body -> (values [M], S [M], counts [M] int).  inputs=np.float64 skips the rounding of coordinates and directions to fp32."""
    verts = np.asarray(verts, inputs)
    points = None if points is None else np.asarray(points, inputs)
    N = verts.shape[0]
    V = verts.astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    anchor = lambda a: (verts[a] if a < N else points[a - N]).astype(np.float64)
    vals, S, counts = np.zeros(len(meas)), np.zeros(len(meas)), np.zeros(len(meas), np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for m, q in enumerate(meas):
            o = anchor(q['anchor'][0])
            n = anchor(q['anchor'][1]) - o if q['anchor'][1] >= 0 else np.asarray(q['dir'], inputs).astype(np.float64)
            if not np.isfinite(n).all() or not n.any():
                continue
            sel = MC.selected_faces(faces, face_parts, N, q['part_mask'])
            X = section_points(V[faces[sel]], o, n)
            counts[m] = 2 * X.shape[0]
            t = np.sqrt(((X[:, 0] - X[:, 1]) ** 2).sum(1))
            if q['kind'] == SECTION:
                vals[m], S[m] = t.sum(), np.abs(t).sum()
                continue
            if not X.shape[0]:
                continue
            u, v = basis(n)
            D = X.reshape(-1, 3) - o
            Q = np.stack([(u[0] * D[:, 0] + u[1] * D[:, 1]) + u[2] * D[:, 2], (v[0] * D[:, 0] + v[1] * D[:, 1]) + v[2] * D[:, 2]], 1)
            if not np.isfinite(Q).all():
                vals[m], S[m] = np.nan, np.nan
                continue
            vals[m] = hull_perimeter(Q)
            S[m] = vals[m] + 2 * np.pi * np.sqrt((Q ** 2).sum(1)).max()
    return vals, S, counts


def oracle(verts, points, faces, face_parts, meas):
    """a batch: verts [B,N,3], points [B,P,3] or None -> (values [B,M], S [B,M], counts [B,M])"""
    res = [oracle_body(verts[b], None if points is None else points[b], faces, face_parts, meas) for b in range(verts.shape[0])]
    return tuple(np.stack([r[i] for r in res]) for i in range(3))


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
prism = MC.prism      # the regular n-gon prism, axis y: [2n side faces | n bottom cap | n top cap], parts 1 / 2 / 3


def ring_prism(ring, h, centre=(0.0, 0.0, 0.0)):
    """closed prism, axis y, over the polygon `ring` [m,2] of (x, z), star-shaped about the origin: the layout of measure_cases.prism"""
    ring = np.asarray(ring, np.float64)
    n = ring.shape[0]
    r3 = np.stack([ring[:, 0], np.zeros(n), ring[:, 1]], 1)
    lo, hi = np.array([0.0, -h / 2, 0.0]), np.array([0.0, h / 2, 0.0])
    v = np.concatenate([r3 + lo, r3 + hi, lo[None], hi[None]]) + np.asarray(centre, np.float64)
    f = []
    for j in range(n):
        k = (j + 1) % n
        f += [(j, n + j, k), (k, n + j, n + k)]
    f += [(2 * n, j, (j + 1) % n) for j in range(n)]
    f += [(2 * n + 1, n + (j + 1) % n, n + j) for j in range(n)]
    return v, np.array(f, np.int32), np.array([1] * (2 * n) + [2] * n + [3] * n, np.uint8)


def star_prism(n, R, r, h):
    """prism over the 2n-gon star: outer radius R at the even corners, inner radius r between them"""
    phi = np.pi * np.arange(2 * n) / n
    rad = np.where(np.arange(2 * n) % 2 == 0, R, r)
    return ring_prism(np.stack([rad * np.cos(phi), rad * np.sin(phi)], 1), h)


def box_prism(k, a, h):
    """prism over the axis-aligned square [-a, a]^2, every side cut into k segments: a section with many equal u and many equal v"""
    t = -a + 2 * a * np.arange(k) / k
    ring = np.concatenate([np.stack([t, np.full(k, -a)], 1), np.stack([np.full(k, a), t], 1), np.stack([-t, np.full(k, a)], 1), np.stack([np.full(k, -a), -t], 1)])
    return ring_prism(ring, h)


def two_prisms(n, r, h, dist):
    """two n-gon prisms in one mesh, centres dist apart along x: the second one's parts are 4 / 5 / 6"""
    v0, f0, p0 = MC.prism(n, r, h, (-dist / 2, 0.0, 0.0))
    v1, f1, p1 = MC.prism(n, r, h, (dist / 2, 0.0, 0.0))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + v0.shape[0]]).astype(np.int32), np.concatenate([p0, p1 + 3]).astype(np.uint8)


def sheet(nx, ny, w, h):
    """a flat open sheet in the plane z = 0, (nx x ny) cells of two triangles, x in [-w/2, w/2], y in [-h/2, h/2]: a plane with normal y
    cuts it in a collinear set"""
    xs, ys = -w / 2 + w * np.arange(nx + 1) / nx, -h / 2 + h * np.arange(ny + 1) / ny
    v = np.array([(x, y, 0.0) for y in ys for x in xs])
    idx = lambda i, j: j * (nx + 1) + i
    f = []
    for j in range(ny):
        for i in range(nx):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v, np.array(f, np.int32), np.ones(len(f), np.uint8)


def one_face():
    return np.array([(0.0, -1.0, 0.0), (2.0, 1.0, 0.5), (-1.0, 1.0, 0.25)]), np.array([(0, 1, 2)], np.int32), np.array([1], np.uint8)


def first_side_faces(k):
    """the first k side faces of the ceil(k / 2)-gon prism (every one is cut by the plane y = 0), cap faces strewn between them in the face
    order so that cut and uncut lanes alternate -> (verts, faces, parts)"""
    n = max(3, (k + 1) // 2)
    v, f, p = MC.prism(n, 0.5, 1.0)
    side, caps = list(range(k)), list(range(2 * n, 4 * n))
    order = []
    for i in range(max(len(side), len(caps))):
        order += side[i:i + 1] + caps[i:i + 1]
    return v, f[order], p[order]


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def three_bodies(v):
    """the body, a copy scaled by 1.5 and a copy moved by 0.25 along every axis, as fp32 [3,N,3]"""
    return np.stack([v, v * 1.5, v + 0.25]).astype(np.float32)


def gpu_cases():
    """name -> (verts float32 [3,N,3], points float32 [3,P,3], faces, parts, [measurements]): the mesh / plane families of the oracle-parity,
    degenerate-section and compaction tests on the GPU.  test_tape_cases_cpu.py checks the input condition on them: no vertex is closer to
    a plane than 1e-9 of the mesh size unless it lies exactly on it."""
    Y, T = (0.0, 1.0, 0.0), (0.3, 1.0, -0.2)
    pt = np.tile(np.array([[[0.0, 0.0, 0.0], [0.0, 0.1, 0.0], [0.05, 0.02, -0.03], [0.0, 9.0, 0.0]]], np.float32), (3, 1, 1))
    cases = {}

    def add(name, mesh, meas):
        v, f, p = mesh
        cases[name] = (three_bodies(v), pt, f, p, meas(len(v)))
    for n in (3, 4, 7):      # a point and a vertex as anchors, a tilted plane through either, a plane that misses (count 0)
        add('prism %d' % n, MC.prism(n, 0.5, 1.0), lambda N: [tape(HULL, N, Y), tape(SECTION, N + 1, Y), tape(HULL, N + 2, T), tape(SECTION, N + 2, T), tape(HULL, 0, T),
                                                              tape(SECTION, 0, T), tape(HULL, N + 3, Y), tape(SECTION, N + 3, Y)])
    add('star', star_prism(5, 1.0, 0.4, 1.0), lambda N: [tape(HULL, N, Y), tape(SECTION, N, Y), tape(HULL, N + 2, T), tape(SECTION, N + 2, T)])
    add('two prisms', two_prisms(7, 0.3, 1.0, 1.0), lambda N: [tape(HULL, N, Y), tape(SECTION, N, Y), tape(HULL, N, Y, part_mask=1 << 1), tape(HULL, N, Y, part_mask=1 << 4),
                                                                tape(SECTION, N, Y, part_mask=(1 << 4) | (1 << 9)), tape(HULL, N, Y, part_mask=1 << 9)])
    add('sheet', sheet(5, 3, 2.0, 1.0), lambda N: [tape(HULL, N + 1, Y), tape(SECTION, N + 1, Y), tape(HULL, N + 2, T)])
    add('box', box_prism(5, 0.5, 1.0), lambda N: [tape(HULL, N, Y), tape(SECTION, N, Y), tape(HULL, N + 2, T)])
    add('one face', one_face(), lambda N: [tape(HULL, N, Y), tape(SECTION, N, Y), tape(HULL, N, toward=N + 1), tape(HULL, N, toward=N), tape(HULL, N + 3, Y),
                                                   tape(HULL, 0, (0.0, -1.0, 0.0)), tape(SECTION, 0, (0.0, -1.0, 0.0))])      # through the lowest corner, alone on its side at d == 0: t = 0, both points ARE that corner
    return cases


def compaction_case(k):
    """k cut faces (first_side_faces), HULL and SECTION through the centre -> the tuple of gpu_cases()"""
    v, f, p = first_side_faces(k)
    pt = np.zeros((3, 1, 3), np.float32)
    return three_bodies(v), pt, f, p, [tape(HULL, len(v), (0.0, 1.0, 0.0)), tape(SECTION, len(v), (0.0, 1.0, 0.0))]
