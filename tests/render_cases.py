"""Shaded weak-perspective mesh pictures (straps_render_mesh, nmr_renderer.WeakPerspectiveMeshRenderer): deterministic mesh cases and the
numpy restatements the CPU and GPU tests compare against.

  * csr_table        : the vertex-to-face table the host builder must produce, by plain loops.
  * render32         : float32 restatement of csrc/render.hip's vertex, normal, face and resolve kernels, unfused, in the kernels' order, with a
                       per-face Python loop: face ids, depth, mask and the per-face flip decision, all meant to agree with the GPU bit for bit.
  * shade64          : float64 shading oracle.  It takes WHICH face a pixel shows and whether that face's normal is flipped from render32 (both
                       are decisions, reproduced exactly there) and computes everything continuous -- rotation, projection, vertex normals,
                       barycentric weights, interpolation, Lambert sum -- in float64 from the float32 inputs.
  * mesh cases       : eval_cases' hand-counted, border, blob and three-camera meshes, plus depth-ordering pairs, a UV sphere, closed grids at the
                       vertex kernels' block edge, unreferenced vertices, out-of-range faces, rotations and the synthetic SMPL mesh.
                       `shaded` marks the cases whose colours are compared: consistently wound meshes, on which the interpolated normal is
                       nowhere short (tests/test_render_cases_cpu.py asserts it); mixed-winding meshes are compared for geometry only.
No GPU, no torch."""
import functools

import numpy as np

import eval_cases as EC

F32 = np.float32
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

# the renderer's defaults: colour, ambient, background, two lights (unit directions from the surface to the light, float32 as the library gets them)
_D = np.array([[0.0, 1.0, -1.0], [0.0, -1.0, -1.0]]) / np.sqrt(2.0)
DEFAULT_OPTS = {'colour': (0.8, 0.3, 0.3), 'ambient': 0.3, 'background': (0.0, 0.0, 0.0), 'light_dir': _D.astype(F32), 'light_intensity': np.array([1.0, 1.0], F32)}
# a second set with every number off its default: three lights, one from the side, a coloured background, a sum that never saturates
# (the defaults saturate wherever a normal faces the viewer: 0.3 + 2 cos 45 > 1)
OTHER_OPTS = {'colour': (0.25, 0.9, 0.55), 'ambient': 0.12, 'background': (0.1, 0.45, 0.8),
              'light_dir': (np.array([[0.6, 0.0, -0.8], [-0.48, 0.6, -0.64], [0.0, 0.0, -1.0]])).astype(F32), 'light_intensity': np.array([0.35, 0.25, 0.2], F32)}


def quantise(c):
    """floor(255 * clamp(c, 0, 1) + 0.5) of float64 values -> uint8"""
    return np.floor(255.0 * np.clip(np.asarray(c, np.float64), 0.0, 1.0) + 0.5).astype(np.uint8)


def quantise32(c):
    """the kernel's quantisation in float32, step by step"""
    c = np.asarray(c, F32)
    return np.floor(F32(255.0) * np.minimum(np.maximum(c, F32(0.0)), F32(1.0)) + F32(0.5)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------------------
# vertex-to-face table
# --------------------------------------------------------------------------------------------------------------------------------
def csr_table(faces, num_vertices):
    """-> (offsets [N+1] int32, table int32): per vertex the ascending ids of the faces that hold it; a face with an index outside [0, N) is
    listed nowhere; a face that names a vertex twice is listed once for it.  Plain loops."""
    per = [[] for _ in range(num_vertices)]
    for f, tri in enumerate(np.asarray(faces, np.int64).tolist()):
        if all(0 <= i < num_vertices for i in tri):
            for i in sorted(set(tri)):
                per[i].append(f)
    offsets = np.zeros(num_vertices + 1, np.int32)
    offsets[1:] = np.cumsum([len(p) for p in per])
    return offsets, np.array([f for p in per for f in p], np.int32)


# --------------------------------------------------------------------------------------------------------------------------------
# float32 restatement
# --------------------------------------------------------------------------------------------------------------------------------
def _valid_faces(faces, N):
    faces = np.asarray(faces, np.int64)
    return ((faces >= 0) & (faces < N)).all(1)


def transform32(verts, cam_wp, rotation=None):
    """render_vertex_kernel: -> (pt [B,N,3], uv [B,N,2]) float32"""
    verts, cam = np.asarray(verts, F32), np.asarray(cam_wp, F32)
    B = verts.shape[0]
    pt, uv = np.empty_like(verts), np.empty(verts.shape[:2] + (2,), F32)
    for b in range(B):
        x, y, z = verts[b, :, 0], verts[b, :, 1], verts[b, :, 2]
        if rotation is not None:
            R = np.asarray(rotation, F32)
            R = R if R.ndim == 2 else R[b]
            x, y, z = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z, (R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z, (R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z)
        pt[b, :, 0], pt[b, :, 1], pt[b, :, 2] = x, y, z
        uv[b, :, 0] = cam[b, 0] * (x + cam[b, 1])
        uv[b, :, 1] = cam[b, 0] * (y + cam[b, 2])
    assert pt.dtype == F32 and uv.dtype == F32
    return pt, uv


def normals32(pt, faces, offsets, table):
    """render_normal_kernel: per vertex the face normals of its table entries, added one by one in the table's order -> [B,N,3] float32"""
    B, N = pt.shape[0], pt.shape[1]
    faces = np.asarray(faces, np.int64)
    safe = np.clip(faces, 0, N - 1)                       # (out-of-range faces are never gathered: they are in no table)
    out = np.zeros((B, N, 3), F32)
    deg = np.diff(offsets)
    for b in range(B):
        p0, p1, p2 = pt[b][safe[:, 0]], pt[b][safe[:, 1]], pt[b][safe[:, 2]]
        a1, a2 = p1 - p0, p2 - p0
        fn = np.stack([a1[:, 1] * a2[:, 2] - a1[:, 2] * a2[:, 1], a1[:, 2] * a2[:, 0] - a1[:, 0] * a2[:, 2], a1[:, 0] * a2[:, 1] - a1[:, 1] * a2[:, 0]], 1)
        assert fn.dtype == F32
        for k in range(int(deg.max()) if deg.size else 0):      # the k-th entry of every vertex that has one: each vertex's own order is kept
            v = np.nonzero(deg > k)[0]
            out[b, v] = out[b, v] + fn[table[offsets[v] + k]]
    return out


def depth_key32(z):
    u = np.asarray(z, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_depth32(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def zbuffer32(pt, uv, faces, wh):
    """render_face_kernel: -> uint64 keys [B,wh,wh] (depth key << 32 | face id; all ones where nothing covers)"""
    B, N = pt.shape[0], pt.shape[1]
    faces = np.asarray(faces, np.int64)
    fw = F32(wh)
    keys = np.full((B, wh, wh), EMPTY_KEY, np.uint64)
    sample = ((2 * np.arange(wh) + 1 - wh).astype(F32)) / fw
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for b in range(B):
            U, V, Z = uv[b, :, 0], uv[b, :, 1], pt[b, :, 2]
            for f in range(faces.shape[0]):
                i0, i1, i2 = faces[f]
                if not (0 <= i0 < N and 0 <= i1 < N and 0 <= i2 < N):
                    continue
                x0, y0, x1, y1, x2, y2 = U[i0], V[i0], U[i1], V[i1], U[i2], V[i2]
                area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
                if not (abs(area) > F32(1e-12)):
                    continue
                xmin, xmax, ymin, ymax = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)
                if not (xmax >= -1 and xmin <= 1 and ymax >= -1 and ymin <= 1):
                    continue
                xa = max(int(np.floor((max(xmin, F32(-1)) * fw + fw - F32(1)) * F32(0.5))), 0)
                xb = min(int(np.ceil((min(xmax, F32(1)) * fw + fw - F32(1)) * F32(0.5))), wh - 1)
                ya = max(int(np.floor((max(ymin, F32(-1)) * fw + fw - F32(1)) * F32(0.5))), 0)
                yb = min(int(np.ceil((min(ymax, F32(1)) * fw + fw - F32(1)) * F32(0.5))), wh - 1)
                if xb < xa or yb < ya:
                    continue
                xp = sample[None, xa:xb + 1]
                yp = sample[ya:yb + 1, None]
                e0 = (xp - x1) * (y2 - y1) - (yp - y1) * (x2 - x1)
                e1 = (xp - x2) * (y0 - y2) - (yp - y2) * (x0 - x2)
                e2 = (xp - x0) * (y1 - y0) - (yp - y0) * (x1 - x0)
                inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                w0, w1, w2 = e0 / area, e1 / area, e2 / area
                z = (w0 * Z[i0] + w1 * Z[i1]) + w2 * Z[i2]
                assert z.dtype == F32
                key = (depth_key32(z).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
                sub = keys[b, ya:yb + 1, xa:xb + 1]
                sub[inside] = np.minimum(sub[inside], key[inside])
    return keys


def render32(verts, faces, cam_wp, wh, rotation=None, num_vertices=None):
    """-> dict: 'face_ids' int32 [B,wh,wh] (-1 empty), 'depth' float32 (+inf empty), 'mask' uint8, 'flip' bool [B,wh,wh] (the winning face's
    decision; False where empty), and the intermediates 'pt', 'uv', 'normals', 'keys'"""
    verts = np.asarray(verts, F32)
    N = verts.shape[1]
    assert num_vertices is None or num_vertices == N
    offsets, table = csr_table(faces, N)
    pt, uv = transform32(verts, cam_wp, rotation)
    nrm = normals32(pt, faces, offsets, table)
    keys = zbuffer32(pt, uv, faces, wh)
    hit = keys != EMPTY_KEY
    fid = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, key_depth32((keys >> np.uint64(32)).astype(np.uint32)), F32(np.inf)).astype(F32)
    safe = np.clip(np.asarray(faces, np.int64), 0, N - 1)
    flip = np.zeros(hit.shape, bool)
    for b in range(verts.shape[0]):
        p0, p1, p2 = pt[b][safe[:, 0]], pt[b][safe[:, 1]], pt[b][safe[:, 2]]
        gz = (p1[:, 0] - p0[:, 0]) * (p2[:, 1] - p0[:, 1]) - (p1[:, 1] - p0[:, 1]) * (p2[:, 0] - p0[:, 0])
        assert gz.dtype == F32
        flip[b][hit[b]] = (gz > 0)[fid[b][hit[b]]]
    return {'face_ids': fid, 'depth': depth, 'mask': hit.astype(np.uint8), 'flip': flip, 'pt': pt, 'uv': uv, 'normals': nrm, 'keys': keys}


# --------------------------------------------------------------------------------------------------------------------------------
# float64 shading oracle
# --------------------------------------------------------------------------------------------------------------------------------
def shade64(verts, faces, cam_wp, wh, face_ids, flip, opts=DEFAULT_OPTS, rotation=None, background=None):
    """-> dict: 'rgb' uint8 [B,wh,wh,3] (the quantised float64 colours; background pixels from `background` uint8 [B,wh,wh,3] or the
    constant colour), 'normal_len' [B,wh,wh] float64 (length of the interpolated, un-normalised normal; nan where empty), 'incident_len'
    [B,wh,wh] (the largest of the winning face's three vertex-normal lengths), 'fallback' bool [B,wh,wh]"""
    v = np.asarray(verts, F32).astype(np.float64)
    cam = np.asarray(cam_wp, F32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    B, N = v.shape[0], v.shape[1]
    ok = _valid_faces(faces, N)
    colour, ambient = np.asarray(opts['colour'], F32).astype(np.float64), float(F32(opts['ambient']))
    dirs, inten = np.asarray(opts['light_dir'], F32).astype(np.float64).reshape(-1, 3), np.asarray(opts['light_intensity'], F32).astype(np.float64)
    rgb = np.empty((B, wh, wh, 3), np.uint8)
    nlen, ilen, fb = np.full((B, wh, wh), np.nan), np.full((B, wh, wh), np.nan), np.zeros((B, wh, wh), bool)
    centre = (2.0 * np.arange(wh) + 1.0 - wh) / wh
    for b in range(B):
        p = v[b]
        if rotation is not None:
            R = np.asarray(rotation, F32).astype(np.float64)
            p = p.dot((R if R.ndim == 2 else R[b]).T)
        uv = cam[b, 0] * (p[:, :2] + cam[b, 1:3])
        nrm = np.zeros((N, 3))
        fv = faces[ok]
        fn = np.cross(p[fv[:, 1]] - p[fv[:, 0]], p[fv[:, 2]] - p[fv[:, 0]])
        for k in range(3):
            np.add.at(nrm, fv[:, k], fn)
        rgb[b] = background[b] if background is not None else quantise(np.asarray(opts['background'], F32).astype(np.float64))
        rr, cc = np.nonzero(face_ids[b] >= 0)
        if rr.size == 0:
            continue
        tri = faces[face_ids[b][rr, cc]]
        a, bb, c = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
        px, py = centre[cc], centre[rr]
        edge = lambda s, t: (px - s[:, 0]) * (t[:, 1] - s[:, 1]) - (py - s[:, 1]) * (t[:, 0] - s[:, 0])
        area = (c[:, 0] - a[:, 0]) * (bb[:, 1] - a[:, 1]) - (c[:, 1] - a[:, 1]) * (bb[:, 0] - a[:, 0])
        w0, w1, w2 = edge(bb, c) / area, edge(c, a) / area, edge(a, bb) / area
        n = w0[:, None] * nrm[tri[:, 0]] + w1[:, None] * nrm[tri[:, 1]] + w2[:, None] * nrm[tri[:, 2]]
        len2 = (n * n).sum(1)
        short = ~(len2 >= 1e-24)
        with np.errstate(invalid='ignore', divide='ignore'):
            n = n / np.sqrt(len2)[:, None]
        n[short] = (0.0, 0.0, -1.0)
        n[flip[b][rr, cc]] *= -1.0
        lam = np.minimum(ambient + (inten[None] * np.maximum(n.dot(dirs.T), 0.0)).sum(1), 1.0)
        rgb[b][rr, cc] = quantise(colour[None] * lam[:, None])
        nlen[b][rr, cc] = np.sqrt(len2)
        ilen[b][rr, cc] = np.sqrt((nrm[tri] ** 2).sum(2)).max(1)
        fb[b][rr, cc] = short
    return {'rgb': rgb, 'normal_len': nlen, 'incident_len': ilen, 'fallback': fb}


# --------------------------------------------------------------------------------------------------------------------------------
# mesh cases
# --------------------------------------------------------------------------------------------------------------------------------
def _tri(wh, pix, z):
    """three (col, row) pixel centres at depth z (a number or three) -> [3,3] float32 rows"""
    z = np.broadcast_to(np.asarray(z, np.float64), (3,))
    return np.array([[EC.centre(c, wh), EC.centre(r, wh), zz] for (c, r), zz in zip(pix, z)], F32)


TRI_A, TRI_B = [(2, 2), (10, 2), (2, 10)], [(4, 4), (12, 4), (4, 12)]      # two right triangles; B is A moved by (2, 2): they overlap in 15 samples


def pair_expected_ids(front, wh=16):
    """hand count at wh = 16.  A holds row r in 2..10, columns 2 .. 12 - r (45 samples, edges included: eval_cases.right_triangle_mask); B
    holds row r in 4..12, columns 4 .. 16 - r (45).  Both: rows 4..8, columns 4 .. 12 - r: 5 + 4 + 3 + 2 + 1 = 15.  The overlap goes to
    `front` (face 0 = A, 1 = B)."""
    ids = np.full((wh, wh), -1, np.int32)
    a, b = np.zeros((wh, wh), bool), np.zeros((wh, wh), bool)
    for r in range(2, 11):
        a[r, 2:12 - r + 1] = True
    for r in range(4, 13):
        b[r, 4:16 - r + 1] = True
    assert a.sum() == 45 and b.sum() == 45 and (a & b).sum() == 15
    ids[a], ids[b & ~a] = 0, 1
    ids[a & b] = front
    assert (ids >= 0).sum() == 75
    return ids[None]


def uv_sphere(rings=9, segs=12, radius=0.7, centre=(0.05, -0.03, 0.1)):
    """a closed sphere, outward winding throughout: 2 + rings * segs = 110 vertices, 2 * segs * rings = 216 faces.  The rings sit at equal steps
    of cos(theta) -- bands of equal area -- with 3 / segs of a step for the two polar caps, so that the un-normalised vertex normals (sums
    of face areas, more or less) have similar lengths everywhere: a pole's `segs` faces together weigh what a ring vertex's six do"""
    cap = 3.0 / segs
    step = 2.0 / (rings - 1 + 2 * cap)
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, rings + 1):
        ct = 1.0 - step * (cap + i - 1)
        st = np.sqrt(1.0 - ct * ct)
        v += [(st * np.cos(2 * np.pi * (j + 0.31) / segs), st * np.sin(2 * np.pi * (j + 0.31) / segs), ct) for j in range(segs)]
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * segs + j % segs
    f = [[0, ring(1, j), ring(1, j + 1)] for j in range(segs)]
    for i in range(1, rings):
        for j in range(segs):
            f += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    last = len(v) - 1
    f += [[last, ring(rings, j + 1), ring(rings, j)] for j in range(segs)]
    verts = (radius * np.array(v) + np.array(centre)).astype(F32)[None]
    faces = np.array(f, np.int32)
    c = verts[0].astype(np.float64).mean(0)                 # outward: every face normal points away from the centre
    p = verts[0].astype(np.float64)
    fn = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    assert (np.einsum('ij,ij->i', fn, p[faces].mean(1) - c) > 0).all()
    return verts, faces


def torus_grid(nu, nv, major=0.55, minor=0.22, centre=(-0.03, 0.04, 0.05), seed=91):
    """an nu x nv grid closed in both directions -- a torus, tilted so that its far half is partly hidden behind its near half -- with every
    face wound outwards: exactly nu * nv vertices, 2 * nu * nv faces, six faces at every vertex.  (An open grid's border vertices hold one to
    three faces and its inner ones six: un-normalised vertex normals of very different lengths side by side, which is what the colour
    comparison's condition rules out.)  The grid lines are jittered a little, so that no two faces are alike."""
    ju, jv = 0.15 * EC.det_uniform((nu,), seed, -1.0, 1.0).astype(np.float64), 0.15 * EC.det_uniform((nv,), seed + 1, -1.0, 1.0).astype(np.float64)
    u, w = 2 * np.pi * (np.arange(nu) + ju) / nu, 2 * np.pi * (np.arange(nv) + jv) / nv
    U, W = np.meshgrid(u, w, indexing='ij')
    ring = major + minor * np.cos(W)
    p = np.stack([ring * np.cos(U), ring * np.sin(U), minor * np.sin(W)], -1).reshape(-1, 3)
    outward = np.stack([np.cos(W) * np.cos(U), np.cos(W) * np.sin(U), np.sin(W)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + j % nv
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, d, e = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
            f += [[a, b, e], [a, e, d]]
    faces = np.array(f, np.int32)
    fn = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    assert (np.einsum('ij,ij->i', fn, outward[faces].sum(1)) > 0).all()
    tilt = EC._rot([1.0, 0.3, 0.0], 1.0)
    return (p.dot(tilt.T) + np.array(centre)).astype(F32)[None], faces


def _case(verts, faces, cam, wh, shaded, rotation=None, expected_ids=None):
    verts = np.ascontiguousarray(verts, F32)
    return {'verts': verts, 'faces': np.ascontiguousarray(faces, np.int32), 'cam': np.ascontiguousarray(cam, F32), 'wh': wh, 'shaded': shaded,
            'rotation': None if rotation is None else np.ascontiguousarray(rotation, F32), 'expected_ids': expected_ids, 'num_vertices': verts.shape[1]}


def _build(name):
    ident = EC.IDENTITY_CAM
    hand = EC.hand_mesh_cases(16)
    if name.startswith('hand_'):
        base, wh = name[5:].rsplit('_wh', 1)
        v, f, c, m = hand[base]
        exp = None
        if int(wh) == 16:
            exp = np.where(m != 0, 0, -1).astype(np.int32)          # (each of these has at most one face that draws: id 0)
        return _case(v, f, c, int(wh), shaded=True, expected_ids=exp)
    if name.startswith('border_wh'):
        v, f = EC.border_mesh()
        return _case(v, f, ident, int(name[9:]), shaded=True)
    if name.startswith('blob_wh'):
        v, f = EC.blob_mesh()
        return _case(v, f, ident, int(name[7:]), shaded=False)
    if name.startswith('cameras_wh'):
        v, f, c = EC.camera_batch_case()
        return _case(v, f, c, int(name[10:]), shaded=False)
    two = np.arange(6, dtype=np.int32).reshape(2, 3)
    if name == 'pair_b_in_front':
        return _case(np.concatenate([_tri(16, TRI_A, 0.5), _tri(16, TRI_B, 0.2)])[None], two, ident, 16, True, expected_ids=pair_expected_ids(1))
    if name == 'pair_negative_a_in_front':
        return _case(np.concatenate([_tri(16, TRI_A, -0.3), _tri(16, TRI_B, 0.2)])[None], two, ident, 16, True, expected_ids=pair_expected_ids(0))
    if name.startswith('interpenetrating_wh'):
        # A tilts from z = -0.5 at its left to +0.5 at its right and passes through the level B (z = 0.02) inside their overlap
        return _case(np.concatenate([_tri(16, TRI_A, (-0.5, 0.5, -0.5)), _tri(16, TRI_B, 0.02)])[None], two, ident, int(name[19:]), True)
    if name == 'coincident':
        t = _tri(16, TRI_A, 0.37)
        return _case(np.concatenate([t, t])[None], two, ident, 16, True, expected_ids=np.where(EC.right_triangle_mask(16) != 0, 0, -1).astype(np.int32)[None])
    if name.startswith('sphere_wh'):
        v, f = uv_sphere()
        return _case(v, f, np.array([[0.9, 0.1, -0.05]], F32), int(name[9:]), True)
    if name == 'sphere_inward_wh20':                                  # every face turned round: the same picture through the flip
        v, f = uv_sphere()
        return _case(v, f[:, ::-1], np.array([[0.9, 0.1, -0.05]], F32), 20, True)
    if name.startswith('grid'):
        n, wh = name[4:].split('_wh')
        # 255 = 15 x 17 and 256 = 16 x 16 closed grids; 257 is prime: the 15 x 17 latitude-longitude grid of a sphere plus its two poles
        v, f = {'255': lambda: torus_grid(15, 17), '256': lambda: torus_grid(16, 16), '257': lambda: uv_sphere(15, 17, 0.8, (0.0, 0.02, 0.0))}[n]()
        assert v.shape[1] == int(n)
        return _case(v, f, np.array([[1.1, 0.02, -0.03]], F32), int(wh), True)
    if name == 'unreferenced_vertex':
        v, f = torus_grid(5, 6)
        lone = np.array([[[0.3, 0.3, -5.0]]], F32)                   # in front of everything, drawn by nothing: index 5, and one more at the end
        v = np.concatenate([v[:, :5], lone, v[:, 5:], lone], 1)
        f = np.where(f >= 5, f + 1, f).astype(np.int32)
        assert 5 not in f and v.shape[1] - 1 not in f
        return _case(v, f, ident, 20, True)
    if name == 'out_of_range_face':
        v, f = torus_grid(5, 6)
        N = v.shape[1]
        f = np.concatenate([f[:7], [[0, 1, N]], f[7:15], [[-1, 2, 3], [4, 2 ** 31 - 1, 5]], f[15:]]).astype(np.int32)
        return _case(v, f, ident, 20, True)
    if name == 'rotation_shared':
        v, f = uv_sphere()
        v = v * np.array([1.0, 0.6, 0.8], F32)                      # an ellipsoid about (almost) the origin: a rotation changes the picture
        return _case(v, f, np.array([[0.95, 0.0, 0.05]], F32), 20, True, rotation=EC._rot([0.3, 1.0, 0.2], 0.8))
    if name == 'rotation_per_body':
        v, f = torus_grid(15, 17)
        v = np.concatenate([v, v * F32(0.9), v + F32(0.02)], 0)
        R = np.stack([EC._rot([1.0, 0.0, 0.0], np.pi), EC._rot([0.2, 1.0, -0.3], 0.5), EC._rot([1.0, 1.0, 0.0], -0.4)])
        return _case(v, f, np.array([[0.8, 0.1, -0.05], [1.0, -0.05, 0.03], [1.3, 0.2, 0.2]], F32), 20, True, rotation=R)
    if name == 'no_normal':
        # the same three vertices wound both ways: every vertex normal is n + (-n) = 0 exactly, so every covered pixel takes the fallback normal
        return _case(_tri(16, TRI_A, (0.1, 0.3, -0.2))[None], np.array([[0, 1, 2], [0, 2, 1]], np.int32), ident, 16, True)
    if name == 'smpl_wh64':
        import straps_amd
        model = straps_amd.synthetic_smpl_model(0)
        return _case(model['v_template'][None].astype(F32), model['faces'], np.array([[0.9, 0.05, -0.1]], F32), 64, False)
    raise KeyError(name)


CASES = tuple(['hand_%s_wh%d' % (n, wh) for n in sorted(EC.hand_mesh_cases(16)) for wh in (16, 20)]
              + ['border_wh16', 'border_wh20', 'border_wh256', 'blob_wh16', 'blob_wh20', 'blob_wh256', 'cameras_wh16', 'cameras_wh20',
                 'pair_b_in_front', 'pair_negative_a_in_front', 'interpenetrating_wh16', 'interpenetrating_wh20', 'coincident', 'sphere_wh16', 'sphere_wh20', 'sphere_inward_wh20',
                 'grid255_wh16', 'grid256_wh20', 'grid257_wh16', 'grid257_wh20', 'unreferenced_vertex', 'out_of_range_face', 'rotation_shared',
                 'rotation_per_body', 'no_normal', 'smpl_wh64'])
HAND_COUNTED = tuple(n for n in CASES if n.endswith('_wh16') and n.startswith('hand_')) + ('pair_b_in_front', 'pair_negative_a_in_front', 'coincident')


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the case dict with its float32 restatement under 'ref' (computed once per process; treat as read-only)"""
    c = _build(name)
    c['ref'] = render32(c['verts'], c['faces'], c['cam'], c['wh'], c['rotation'])
    return c


@functools.lru_cache(maxsize=None)
def oracle(name, which='default', with_background=False):
    """-> shade64 of case `name` under DEFAULT_OPTS / OTHER_OPTS, over background_image(...) or the constant colour (read-only)"""
    c = case(name)
    bg = background_image(c['verts'].shape[0], c['wh']) if with_background else None
    return shade64(c['verts'], c['faces'], c['cam'], c['wh'], c['ref']['face_ids'], c['ref']['flip'], {'default': DEFAULT_OPTS, 'other': OTHER_OPTS}[which],
                   c['rotation'], bg)


def background_image(B, wh, seed=4242):
    """uint8 [B,wh,wh,3] of bytes that no shaded pixel is likely to repeat by accident"""
    return (EC.det_uniform((B, wh, wh, 3), seed, 0.0, 1.0) * 256.0).astype(np.int64).clip(0, 255).astype(np.uint8)


SHADED_CASES = tuple(n for n in CASES if n != 'smpl_wh64' and not n.startswith(('blob_', 'cameras_')))
