"""Float64 restatement of the GRADIENT of the tape-measure girths of csrc/measure_tape.hip (straps_measure_tape_bwd, csrc/measure_tape_bwd.hip;
include/straps_hip.h states the definition), on the meshes and measurement dicts of tests/tape_cases.py.

Two independent statements of the same derivative:
  * `values_torch`: float64 torch on the branch the forward takes.  The section points are those of tape_cases.section_points (side tests and
    the lone vertex decided on detached numbers).  SECTION: the sum of |x - x'| over the cut faces, faces of length exactly 0 left out.
    HULL: the chain of corners is chosen on the DETACHED (u, v) coordinates by Andrew's monotone chain on the distinct points (of equal
    points the lowest index stands for all); the perimeter is then the sum of the edge lengths between the chosen points, in the plane's
    basis, which is a constant.  Its autograd gradient w.r.t. vertices and points is THE ORACLE (`oracle_grad`).
  * `scatter`: the closed forms of the header, term by term in numpy.  With x = p_a + t (p_b - p_a), e = p_b - p_a, D = n . e, upstream g and
    s = (g . e) / D:  dp_a += (1 - t)(g - s n), dp_b += t (g - s n), do += s n, dn += -s (x - o);  per-body normal: dA1 += dn, dA0 += do - dn.
    It also gives, per output element, S: the sum of |dout| x |term| over the terms added into it.  A HULL corner adds, to all three
    components, |dout| x 2 x the Frobenius norm of the 3x3 block that carries g to that row (|g| <= 2: two unit vectors): entry-wise, S
    would be exactly 0 on axis-aligned prisms, where the two unit vectors of a corner cancel in exact arithmetic and not in double.  A
    SECTION point adds |dout| x 1 x that norm (|g| = 1) for the same reason: on a vertical edge under a normal with n_y = 1 the y
    component of g - s n is g_y - g_y in exact arithmetic, the closed form may give exactly 0 there, and autograd leaves 1e-18 ('prism 4',
    the tilted plane through vertex 0).  A section point that is no corner but lies ON the hull's boundary (within BOUNDARY = 1e-9 of the
    section's size: the collinear points a closed mesh puts on every quad diagonal, the sides of the box) adds the same block term with a
    zero vector: whether such a point is a corner is decided by the last bit of an orientation test, the kernel's coordinates differ from
    these by a few ulps (fused multiply-adds), and the derivative is continuous there -- as a corner the point receives the difference of
    two unit vectors that agree to rounding.
A GPU result is held to |got - want| <= 2^-23 |want| + 1e-10 S, the module's bar (tests/measure_grad_cases.py has the margin argument).

Special rows, as the header states them: dout == +-0 adds nothing; a HULL row that is NaN in the forward (a non-finite section point) puts
dout x NaN into the row of its anchor[0] and adds nothing else; a normal that cuts nothing adds nothing.

`assert_conditions` states what a case must satisfy so that the last bit of a double cannot decide a branch: no vertex of a cut face other
than an anchor itself within MIN_PLANE_DISTANCE = 1e-6 m of a plane (the full-size bodies would not all pass measure_grad_cases' 1e-5; 1e-6
is still ten orders above the double rounding of d), and no two hull corners from DIFFERENT mesh edges within 1e-7 m of each other
(near-coincident points of the same mesh edge, computed in two faces, are expected: either carries the same gradient to the same vertices).
"""
import numpy as np
import torch

import measure_cases as MC
import tape_cases as TC
from tape_cases import HULL, SECTION

MIN_PLANE_DISTANCE = 1e-6
MIN_CORNER_DISTANCE = 1e-7
BOUNDARY = 1e-9


def on_boundary(Q, chain):
    """Q [n,2], chain: hull_chain(Q) -> bool [n]: the points within BOUNDARY x the largest |q| of the hull's boundary"""
    if not chain:
        return np.zeros(Q.shape[0], bool)
    A, B = Q[chain], Q[np.roll(chain, -1)]
    E = B - A
    L2 = (E ** 2).sum(1)
    t = np.clip(((Q[:, None] - A[None]) * E[None]).sum(2) / L2[None], 0.0, 1.0)
    dist = np.sqrt((((A[None] + t[..., None] * E[None]) - Q[:, None]) ** 2).sum(2)).min(1)
    return dist <= BOUNDARY * np.sqrt((Q ** 2).sum(1)).max()


def hull_chain(Q):
    """Q [n,2] finite -> indices of the hull's corners in chain order (the lower chain from the lexicographic minimum, then the upper chain):
    Andrew's monotone chain on the distinct points, collinear points dropped; of equal points the lowest index.  [] for none or one distinct point."""
    first = {}
    for i, (x, y) in enumerate(np.asarray(Q, np.float64).reshape(-1, 2)):
        first.setdefault((float(x), float(y)), i)
    pts = sorted(first)
    if len(pts) < 2:
        return []
    chains = []
    for seq in (pts, pts[::-1]):
        ch = []
        for p in seq:
            while len(ch) >= 2 and TC.cross(ch[-2], ch[-1], p) <= 0:
                ch.pop()
            ch.append(p)
        chains.append(ch)
    return [first[p] for p in chains[0][:-1] + chains[1][:-1]]


def _plane(q, V, Pts):
    """-> (o, n) of measurement q on the leaves (torch) or arrays (numpy) V, Pts"""
    N = V.shape[0]
    anchor = lambda a: V[a] if a < N else Pts[a - N]
    o = anchor(q['anchor'][0])
    if q['anchor'][1] >= 0:
        return o, anchor(q['anchor'][1]) - o
    d = np.asarray(q['dir'], np.float64)
    return o, (torch.from_numpy(d) if isinstance(V, torch.Tensor) else d)


def _cut_faces(P, o, n):
    """P [f,3,3], o, n float64 numpy -> (idx of the cut faces, lone corner of each) by the forward's rule"""
    d = (n[0] * (P[..., 0] - o[0]) + n[1] * (P[..., 1] - o[1])) + n[2] * (P[..., 2] - o[2])
    s = d >= 0
    cut = ~((s[:, 0] == s[:, 1]) & (s[:, 1] == s[:, 2]))
    idx = np.nonzero(cut)[0]
    return idx, np.where(s[:, 1] == s[:, 2], 0, np.where(s[:, 0] == s[:, 2], 1, 2))[idx]


def _coords(X, o, n):
    """X [c,2,3], o, n float64 numpy -> (Q [2c,2], u, v): the header's basis and dot order"""
    u, v = TC.basis(n)
    D = X.reshape(-1, 3) - o
    return np.stack([(u[0] * D[:, 0] + u[1] * D[:, 1]) + u[2] * D[:, 2], (v[0] * D[:, 0] + v[1] * D[:, 1]) + v[2] * D[:, 2]], 1), u, v


# ---- the oracle: float64 torch, autograd --------------------------------------------------------------------------------------------
def values_torch(V, Pts, faces, face_parts, meas):
    """V [N,3], Pts [P,3] or None: float64 torch leaves -> the M values, a list of float64 torch scalars (a NaN HULL row: a detached NaN)"""
    N = V.shape[0]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    out = []
    zero = lambda: torch.zeros((), dtype=torch.float64)
    for q in meas:
        o, n = _plane(q, V, Pts)
        nd, od = n.detach().numpy(), o.detach().numpy()
        if not np.isfinite(nd).all() or not nd.any():
            out.append(zero())
            continue
        sel = MC.selected_faces(faces, face_parts, N, q['part_mask'])
        P = V[torch.from_numpy(faces[sel])]
        with np.errstate(invalid='ignore', over='ignore'):
            idx, lone = _cut_faces(P.detach().numpy(), od, nd)
        if not idx.size:
            out.append(zero())
            continue
        rows, a = torch.arange(idx.size), torch.from_numpy(lone)
        Pc = P[torch.from_numpy(idx)]
        d = (n[0] * (Pc[..., 0] - o[0]) + n[1] * (Pc[..., 1] - o[1])) + n[2] * (Pc[..., 2] - o[2])
        A, B, C = Pc[rows, a], Pc[rows, (a + 1) % 3], Pc[rows, (a + 2) % 3]
        da, db, dc = d[rows, a], d[rows, (a + 1) % 3], d[rows, (a + 2) % 3]
        xb = A + (da / (da - db))[:, None] * (B - A)
        xc = A + (da / (da - dc))[:, None] * (C - A)
        if q['kind'] == SECTION:
            len2 = ((xb - xc) ** 2).sum(1)
            out.append(torch.sqrt(len2[~(len2.detach() == 0)]).sum())
            continue
        X = torch.stack([xb, xc], 1)
        with np.errstate(invalid='ignore', over='ignore'):
            Qd, u, v = _coords(X.detach().numpy(), od, nd)
        if not np.isfinite(Qd).all():
            out.append(torch.tensor(float('nan'), dtype=torch.float64))
            continue
        chain = hull_chain(Qd)
        if not chain:
            out.append(zero())
            continue
        D = X.reshape(-1, 3)[torch.tensor(chain)] - o
        Q = torch.stack([D @ torch.from_numpy(u), D @ torch.from_numpy(v)], 1)
        out.append(torch.sqrt(((Q - torch.roll(Q, 1, 0)) ** 2).sum(1)).sum())
    return [x.reshape(()) for x in out]


def _leaves(verts, points, inputs):
    V = torch.from_numpy(np.asarray(verts, inputs).astype(np.float64)).requires_grad_(True)
    Pts = None if points is None else torch.from_numpy(np.asarray(points, inputs).astype(np.float64)).requires_grad_(True)
    return V, Pts


def _grad(scalar, V, Pts):
    leaves = [V] + ([Pts] if Pts is not None else [])
    g = torch.autograd.grad(scalar, leaves, retain_graph=True, allow_unused=True) if scalar.requires_grad else [None] * len(leaves)
    gv = np.zeros(tuple(V.shape)) if g[0] is None else g[0].numpy().copy()
    gp = np.zeros((0, 3)) if Pts is None else (np.zeros(tuple(Pts.shape)) if g[1] is None else g[1].numpy().copy())
    return gv, gp


def oracle_grad_body(verts, points, faces, face_parts, meas, dout, inputs=np.float32):
    """one body: dout [M] -> (values [M], dverts [N,3], dpoints [P,3]) float64: the autograd gradient of sum_m dout[m] * value_m over the rows
    with dout != 0, and dout x NaN in the row of anchor[0] of every NaN row among them"""
    V, Pts = _leaves(verts, points, inputs)
    N = V.shape[0]
    vals = values_torch(V, Pts, faces, face_parts, meas)
    dout = np.asarray(dout, np.float64)
    loss = torch.zeros((), dtype=torch.float64)
    for v, d in zip(vals, dout):
        if d != 0 and not np.isnan(float(v.detach())):
            loss = loss + v * float(d)
    gv, gp = _grad(loss, V, Pts)
    for v, d, q in zip(vals, dout, meas):
        if d != 0 and q['kind'] == HULL and np.isnan(float(v.detach())):
            a = q['anchor'][0]
            (gv if a < N else gp)[a if a < N else a - N] += np.nan
    return np.array([float(v.detach()) for v in vals]), gv, gp


# ---- the closed forms, term by term: numpy ------------------------------------------------------------------------------------------
def scatter(verts, points, faces, face_parts, meas, dout):
    """one body -> (dverts [N,3], dpoints [P,3], S_verts, S_points): every term of the header's formulas added into the row it belongs to"""
    V = np.asarray(verts, np.float32).astype(np.float64)
    Pts = None if points is None else np.asarray(points, np.float32).astype(np.float64)
    N, npts = V.shape[0], 0 if points is None else Pts.shape[0]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    grad, S = np.zeros((N + npts, 3)), np.zeros((N + npts, 3))
    eye = np.eye(3)

    def add(row, vec, block, gmax):
        grad[row] += vec
        S[row] += np.abs(vec) + gmax * np.sqrt((block ** 2).sum())
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for q, dm in zip(meas, np.asarray(dout, np.float64)):
            if dm == 0:
                continue
            o, n = _plane(q, V, Pts)
            if not np.isfinite(n).all() or not n.any():
                continue
            a0, a1 = q['anchor']
            sel = np.nonzero(MC.selected_faces(faces, face_parts, N, q['part_mask']))[0]
            P = V[faces[sel]]
            idx, lone = _cut_faces(P, o, n)
            if not idx.size:
                continue
            fid = faces[sel[idx]]
            rows = np.arange(idx.size)
            Pc = P[idx]
            d = (n[0] * (Pc[..., 0] - o[0]) + n[1] * (Pc[..., 1] - o[1])) + n[2] * (Pc[..., 2] - o[2])
            ia, ib, ic = lone, (lone + 1) % 3, (lone + 2) % 3
            A, B, C = Pc[rows, ia], Pc[rows, ib], Pc[rows, ic]
            da, db, dc = d[rows, ia], d[rows, ib], d[rows, ic]
            tb, tc = da / (da - db), da / (da - dc)
            X = np.stack([A + tb[:, None] * (B - A), A + tc[:, None] * (C - A)], 1)
            G = np.zeros((idx.size, 2, 3))                           # the upstream vector of every section point
            edge = np.zeros((idx.size, 2), bool)                     # HULL: the point lies on the hull's boundary
            hull = q['kind'] == HULL
            if hull:
                Q, u, v = _coords(X, o, n)
                if not np.isfinite(Q).all():
                    grad[a0] += np.nan
                    S[a0] += np.nan
                    continue
                chain = hull_chain(Q)
                edge = on_boundary(Q, chain).reshape(-1, 2)
                for k, i in enumerate(chain):
                    g2 = np.zeros(2)
                    for j in (chain[k - 1], chain[(k + 1) % len(chain)]):
                        e = Q[i] - Q[j]
                        g2 += e / np.sqrt((e ** 2).sum())
                    G[i // 2, i % 2] = g2[0] * u + g2[1] * v
            else:
                e = X[:, 0] - X[:, 1]
                L = np.sqrt((e ** 2).sum(1))
                ok = L > 0
                G[ok, 0] = e[ok] / L[ok, None]
                G[ok, 1] = -G[ok, 0]
            for r in range(idx.size):
                for pt, (other, t, E, Dd) in enumerate(((ib[r], tb[r], B[r] - A[r], db[r] - da[r]), (ic[r], tc[r], C[r] - A[r], dc[r] - da[r]))):
                    g = G[r, pt]
                    if not g.any() and not edge[r, pt]:
                        continue
                    s = (g @ E) / Dd
                    h = g - s * n
                    gmax = 2.0 if hull else 1.0                          # |g| of a hull corner (two unit vectors), of a section point
                    J = eye - np.outer(n, E) / Dd                        # dx/dp_a = (1 - t) J^T, dx/dp_b = t J^T
                    add(fid[r, ia[r]], dm * (1 - t) * h, dm * (1 - t) * J, gmax)
                    add(fid[r, other], dm * t * h, dm * t * J, gmax)
                    go, gn = s * n, -s * (X[r, pt] - o)
                    bo, bn = dm * np.outer(n, E) / Dd, dm * np.outer(X[r, pt] - o, E) / Dd
                    add(a0, dm * go, bo, gmax)
                    if a1 >= 0:
                        add(a0, -dm * gn, bn, gmax)
                        add(a1, dm * gn, bn, gmax)
    return grad[:N], grad[N:], S[:N], S[N:]


def oracle_grad(verts, points, faces, face_parts, meas, dout):
    """a batch: verts [B,N,3], points [B,P,3] or None, dout [B,M] -> (values [B,M], dverts [B,N,3], dpoints [B,P,3], S_verts, S_points) float64:
    the autograd gradient, and S of the closed-form terms"""
    res = []
    for b in range(verts.shape[0]):
        pb = None if points is None else points[b]
        vals, gv, gp = oracle_grad_body(verts[b], pb, faces, face_parts, meas, dout[b])
        _, _, sv, sp = scatter(verts[b], pb, faces, face_parts, meas, dout[b])
        assert ((sv > 0) | (gv == 0) | np.isnan(gv)).all() and ((sp > 0) | (gp == 0) | np.isnan(gp)).all(), 'body %d: an element with S == 0 is not exactly 0' % b
        res.append((vals, gv, gp, sv, sp))
    return tuple(np.stack([r[i] for r in res]) for i in range(5))


# ---- the conditions a case must satisfy ---------------------------------------------------------------------------------------------
def worst_distances(verts, points, faces, face_parts, meas):
    """-> (the smallest distance of a vertex of a cut face, other than an anchor, from its plane; the smallest distance between two hull
    corners from different mesh edges) over the finite bodies and their planes that cut; inf where there is none"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    plane, corner = np.inf, np.inf
    for b in range(verts.shape[0]):
        V = verts[b].astype(np.float64)
        Pts = None if points is None else points[b].astype(np.float64)
        if np.isnan(V).any() or np.isinf(V).any() or (Pts is not None and not np.isfinite(Pts).all()):
            continue
        N = V.shape[0]
        for q in meas:
            o, n = _plane(q, V, Pts)
            if not n.any():
                continue
            fs = faces[MC.selected_faces(faces, face_parts, N, q['part_mask'])]
            P = V[fs]
            idx, lone = _cut_faces(P, o, n)
            if not idx.size:
                continue
            d = ((P[idx] - o) * n).sum(2) / np.sqrt((n ** 2).sum())
            far = (fs[idx] != q['anchor'][0]) & (fs[idx] != q['anchor'][1])
            if far.any():
                plane = min(plane, float(np.abs(d[far]).min()))
            if q['kind'] != HULL:
                continue
            X = TC.section_points(P, o, n)
            Q, _, _ = _coords(X, o, n)
            chain = hull_chain(Q)
            rows = np.arange(idx.size)
            edge = lambda i: tuple(sorted((int(fs[idx[i // 2], lone[i // 2]]), int(fs[idx[i // 2], (lone[i // 2] + 1 + i % 2) % 3]))))
            for x in range(len(chain)):
                for y in range(x + 1, len(chain)):
                    if edge(chain[x]) != edge(chain[y]):
                        corner = min(corner, float(np.sqrt(((Q[chain[x]] - Q[chain[y]]) ** 2).sum())))
    return plane, corner


def assert_conditions(verts, points, faces, face_parts, meas):
    plane, corner = worst_distances(verts, points, faces, face_parts, meas)
    assert plane >= MIN_PLANE_DISTANCE, 'a vertex of a cut face lies %.3g m from a plane' % plane
    assert corner >= MIN_CORNER_DISTANCE, 'two hull corners from different mesh edges lie %.3g m apart' % corner

