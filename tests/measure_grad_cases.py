"""Float64 restatement of the GRADIENT of the measurements of csrc/measure.hip (straps_measure_mesh_bwd, csrc/measure_bwd.hip; include/straps_hip.h
states the definitions), on the meshes and measurement dicts of tests/measure_cases.py.

Two independent statements of the same derivative:
  * `values_torch`: the five kinds in float64 torch on the branch the forward takes (side tests, lone vertex, selected faces and the extreme
    vertices are decided on detached numbers; faces whose term is degenerate -- |n|^2 == 0, section length 0 -- and zero-length segments are
    left out of the sum, which is the definition's "contributes nothing").  Its autograd gradient is THE ORACLE (`oracle_grad`).
  * `scatter`: the closed-form per-term gradients in numpy, added term by term into the rows they belong to.  It also gives, per output
    element, S: the sum of |dout_m| x |contribution| over the terms added into it.  `gather` adds the same face terms through the CSR
    vertex-to-face table, the way the kernel does.
A GPU result is held to |got - want| <= 2^-23 |want| + 1e-10 S, the forward's bar in tests/measure_cases.py with the same margin argument: both
sides compute every term in double from the same fp32 inputs, so they differ by the summation order and fused multiply-adds -- far below
1e-10 S -- and by the one rounding to float.

A gradient, unlike a value, JUMPS when a side test flips or an extreme moves to another vertex.  `assert_conditions` states what a case must
satisfy so that the last bit of a double cannot decide a branch: no vertex of a cut face other than the anchor itself within 1e-5 m of the
plane, no two vertices tied for an EXTENT extreme (except where a case is built to test the tie rule).
"""
import numpy as np
import torch

import measure_cases as MC
from measure_cases import AREA, EXTENT, FACE_KINDS, GIRTH, PATH, VOLUME

MIN_PLANE_DISTANCE = 1e-5


def _n_anchors(q):
    if q['kind'] == PATH:
        k = 0
        while k < 4 and q['anchor'][k] >= 0:
            k += 1
        return k
    if q['kind'] == GIRTH or (q['kind'] == VOLUME and q['anchor'][0] >= 0):
        return 1
    return 0


def _lone(d):
    """d [f,3] signed distances -> (cut bool [f], lone corner [f]) by the forward's rule (d >= 0 is positive, a NaN is not)"""
    s = d >= 0
    cut = ~((s[:, 0] == s[:, 1]) & (s[:, 1] == s[:, 2]))
    return cut, np.where(s[:, 1] == s[:, 2], 0, np.where(s[:, 0] == s[:, 2], 1, 2))


# ---- the oracle: float64 torch, autograd --------------------------------------------------------------------------------------------
def values_torch(V, Pts, faces, face_parts, meas):
    """V [N,3], Pts [P,3] or None: float64 torch tensors (leaves with requires_grad for a gradient) -> the M values, a list of float64 torch scalars"""
    N = V.shape[0]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    anchor = lambda a: V[a] if a < N else Pts[a - N]
    out = []
    for q in meas:
        kind, anc = q['kind'], q['anchor']
        n = torch.tensor(q['dir'], dtype=torch.float64)
        if kind in FACE_KINDS:
            sel = MC.selected_faces(faces, face_parts, N, q['part_mask'])
            P = V[torch.from_numpy(faces[sel])]                                 # [f,3,3]
            if kind == VOLUME:
                r = P - (anchor(anc[0]) if anc[0] >= 0 else torch.zeros(3, dtype=torch.float64))
                out.append((r[:, 0] * torch.cross(r[:, 1], r[:, 2], dim=1)).sum() / 6.0)
            elif kind == AREA:
                n2 = (torch.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], dim=1) ** 2).sum(1)
                out.append(0.5 * torch.sqrt(n2[n2.detach() > 0]).sum())
            else:
                o = anchor(anc[0])
                d = ((P - o) * n).sum(2)
                cut, lone = _lone(d.detach().numpy())
                idx = torch.from_numpy(np.nonzero(cut)[0])
                a = torch.from_numpy(lone[cut])
                if idx.numel() == 0:
                    out.append(torch.zeros((), dtype=torch.float64))
                    continue
                rows = torch.arange(idx.numel())
                Pc, dcut = P[idx], d[idx]
                A, B, C = Pc[rows, a], Pc[rows, (a + 1) % 3], Pc[rows, (a + 2) % 3]
                da, db, dc = dcut[rows, a], dcut[rows, (a + 1) % 3], dcut[rows, (a + 2) % 3]
                xb = A + (da / (da - db))[:, None] * (B - A)
                xc = A + (da / (da - dc))[:, None] * (C - A)
                len2 = ((xb - xc) ** 2).sum(1)
                out.append(torch.sqrt(len2[len2.detach() > 0]).sum())
        elif kind == EXTENT:
            h = V @ n
            hn = h.detach().numpy()
            if np.isnan(hn).any():
                out.append(torch.tensor(float('nan'), dtype=torch.float64))
            else:
                out.append(h[int(np.argmax(hn))] - h[int(np.argmin(hn))])      # (argmax / argmin: the first, i.e. lowest, index)
        else:
            pts = [anchor(a) for a in anc[:_n_anchors(q)]]
            total = torch.zeros((), dtype=torch.float64)
            for p0, p1 in zip(pts[:-1], pts[1:]):
                l2 = ((p1 - p0) ** 2).sum()
                if float(l2.detach()) > 0 or np.isnan(float(l2.detach())):
                    total = total + torch.sqrt(l2)
            out.append(total)
    return [o.reshape(()) for o in out]


def _leaves(verts, points, inputs):
    V = torch.from_numpy(np.asarray(verts, inputs).astype(np.float64)).requires_grad_(True)
    Pts = None if points is None else torch.from_numpy(np.asarray(points, inputs).astype(np.float64)).requires_grad_(True)
    return V, Pts


def _grad(scalar, V, Pts):
    """autograd gradient of a scalar w.r.t. the leaves -> numpy (zeros where the scalar does not depend on a leaf)"""
    leaves = [V] + ([Pts] if Pts is not None else [])
    g = torch.autograd.grad(scalar, leaves, retain_graph=True, allow_unused=True) if scalar.requires_grad else [None] * len(leaves)
    gv = np.zeros(tuple(V.shape)) if g[0] is None else g[0].numpy()
    gp = np.zeros((0, 3)) if Pts is None else (np.zeros(tuple(Pts.shape)) if g[1] is None else g[1].numpy())
    return gv, gp


def oracle_jacobian(verts, points, faces, face_parts, meas, inputs=np.float32):
    """one body -> (values [M], dvalue/dverts [M,N,3], dvalue/dpoints [M,P,3] (P may be 0)): one backward pass per measurement"""
    V, Pts = _leaves(verts, points, inputs)
    vals = values_torch(V, Pts, faces, face_parts, meas)
    J = [_grad(v, V, Pts) for v in vals]
    return np.array([float(v.detach()) for v in vals]), np.stack([j[0] for j in J]), np.stack([j[1] for j in J])


def oracle_grad_body(verts, points, faces, face_parts, meas, dout, inputs=np.float32):
    """one body: dout [M] -> (dverts [N,3], dpoints [P,3]) float64 = the autograd gradient of sum_m dout[m] * value_m"""
    V, Pts = _leaves(verts, points, inputs)
    vals = values_torch(V, Pts, faces, face_parts, meas)
    loss = sum(v * float(d) for v, d in zip(vals, np.asarray(dout, np.float64)))
    return _grad(loss, V, Pts)


# ---- the closed forms, term by term: numpy ------------------------------------------------------------------------------------------
def face_terms(q, P, o):
    """P [f,3,3] float64 corners of the selected faces, o [3] the anchor (zeros without) -> (g [f,3,3] per corner, go [f,3] w.r.t. the anchor);
    rows of faces that contribute nothing are zero"""
    f = P.shape[0]
    g, go = np.zeros((f, 3, 3)), np.zeros((f, 3))
    kind = q['kind']
    with np.errstate(invalid='ignore', divide='ignore'):
        if kind == VOLUME:
            r = P - o
            g[:, 0], g[:, 1], g[:, 2] = np.cross(r[:, 1], r[:, 2]) / 6.0, np.cross(r[:, 2], r[:, 0]) / 6.0, np.cross(r[:, 0], r[:, 1]) / 6.0
            go = -g.sum(1)
        elif kind == AREA:
            n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
            n2 = (n ** 2).sum(1)
            ok = n2 > 0
            h = n[ok] / (2.0 * np.sqrt(n2[ok]))[:, None]
            Q = P[ok]
            g[ok, 0], g[ok, 1], g[ok, 2] = np.cross(h, Q[:, 2] - Q[:, 1]), np.cross(h, Q[:, 0] - Q[:, 2]), np.cross(h, Q[:, 1] - Q[:, 0])
        else:
            n = np.asarray(q['dir'], np.float64)
            d = (n[0] * (P[..., 0] - o[0]) + n[1] * (P[..., 1] - o[1])) + n[2] * (P[..., 2] - o[2])
            cut, lone = _lone(d)
            idx = np.nonzero(cut)[0]
            if idx.size:
                a = lone[idx]
                A, B, C = P[idx, a], P[idx, (a + 1) % 3], P[idx, (a + 2) % 3]
                da, db, dc = d[idx, a], d[idx, (a + 1) % 3], d[idx, (a + 2) % 3]
                Db, Dc = da - db, da - dc
                tb, tc = da / Db, da / Dc
                e = (A + tb[:, None] * (B - A)) - (A + tc[:, None] * (C - A))
                L = np.sqrt((e ** 2).sum(1))
                ok = L > 0
                u = np.where(ok[:, None], e / np.where(ok, L, 1.0)[:, None], 0.0)
                sb, sc = (u * (B - A)).sum(1), (u * (C - A)).sum(1)
                GA = u * (tc - tb)[:, None] + n * (sc * dc / Dc ** 2 - sb * db / Db ** 2)[:, None]
                GB = u * tb[:, None] + n * (sb * da / Db ** 2)[:, None]
                GC = -u * tc[:, None] - n * (sc * da / Dc ** 2)[:, None]
                GO = -n * (sb / Db - sc / Dc)[:, None]
                for G, role in ((GA, 0), (GB, 1), (GC, 2)):
                    g[idx, (a + role) % 3] = np.where(ok[:, None], G, 0.0)
                go[idx] = np.where(ok[:, None], GO, 0.0)
    return g, go


def _other_terms(q, V, Pts, dm, add):
    """the terms that are not per corner of a face: EXTENT extremes and PATH segments; add(anchor index, vector)"""
    N = V.shape[0]
    point = lambda a: V[a] if a < N else Pts[a - N]
    if q['kind'] == EXTENT:
        n = np.asarray(q['dir'], np.float64)
        h = (n[0] * V[:, 0] + n[1] * V[:, 1]) + n[2] * V[:, 2]
        if not np.isnan(h).any():
            add(int(np.argmax(h)), n * dm)
            add(int(np.argmin(h)), -n * dm)
    elif q['kind'] == PATH:
        anc = q['anchor'][:_n_anchors(q)]
        for a0, a1 in zip(anc[:-1], anc[1:]):
            e = point(a1) - point(a0)
            L = np.sqrt((e ** 2).sum())
            if L > 0 or np.isnan(L):
                add(a1, e / L * dm)
                add(a0, -e / L * dm)


def _accumulate(verts, points, faces, face_parts, meas, dout, face_adder):
    """shared frame of scatter and gather: face_adder(grad, S, faces[sel] [f,3], dm * g [f,3,3]) adds the corner terms"""
    V = np.asarray(verts, np.float32).astype(np.float64)
    Pts = None if points is None else np.asarray(points, np.float32).astype(np.float64)
    N, npts = V.shape[0], 0 if points is None else Pts.shape[0]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    grad, S = np.zeros((N + npts, 3)), np.zeros((N + npts, 3))

    def add(a, vec):
        grad[a] += vec
        S[a] += np.abs(vec)
    for q, dm in zip(meas, np.asarray(dout, np.float64)):
        if q['kind'] in FACE_KINDS:
            sel = MC.selected_faces(faces, face_parts, N, q['part_mask'])
            a0 = q['anchor'][0] if _n_anchors(q) else -1
            o = (V[a0] if a0 < N else Pts[a0 - N]) if a0 >= 0 else np.zeros(3)
            g, go = face_terms(q, V[faces[sel]], o)
            face_adder(grad, S, np.nonzero(sel)[0], faces, dm * g)
            if a0 >= 0:
                grad[a0] += dm * go.sum(0)
                S[a0] += np.abs(dm * go).sum(0)
        else:
            _other_terms(q, V, Pts, dm, add)
    return grad[:N], grad[N:], S[:N], S[N:]


def scatter(verts, points, faces, face_parts, meas, dout):
    """one body -> (dverts [N,3], dpoints [P,3], S_verts, S_points): every term added into the row it belongs to"""
    def adder(grad, S, fid, faces, t):
        for i in range(3):
            np.add.at(grad, faces[fid, i], t[:, i])
            np.add.at(S, faces[fid, i], np.abs(t[:, i]))
    return _accumulate(verts, points, faces, face_parts, meas, dout, adder)


def gather(verts, points, faces, face_parts, meas, dout, vf_offsets, vf_faces):
    """scatter's result through the CSR vertex-to-face table, as the kernel walks it: for every (vertex, listed face) pair, every corner of
    the face that names the vertex adds its term"""
    pair_v = np.repeat(np.arange(len(vf_offsets) - 1), np.diff(vf_offsets))
    pair_f = np.asarray(vf_faces, np.int64)

    def adder(grad, S, fid, faces, t):
        slot = np.full(faces.shape[0], -1, np.int64)
        slot[fid] = np.arange(fid.size)                        # face id -> row of t; -1: not selected by this measurement
        for i in range(3):
            hit = (slot[pair_f] >= 0) & (faces[pair_f, i] == pair_v)
            np.add.at(grad, pair_v[hit], t[slot[pair_f[hit]], i])
            np.add.at(S, pair_v[hit], np.abs(t[slot[pair_f[hit]], i]))
    return _accumulate(verts, points, faces, face_parts, meas, dout, adder)


def oracle_grad(verts, points, faces, face_parts, meas, dout):
    """a batch: verts [B,N,3], points [B,P,3] or None, dout [B,M] -> (dverts [B,N,3], dpoints [B,P,3], S_verts, S_points) float64: the autograd
    gradient, and S of the closed-form terms"""
    res = []
    for b in range(verts.shape[0]):
        pb = None if points is None else points[b]
        gv, gp = oracle_grad_body(verts[b], pb, faces, face_parts, meas, dout[b])
        _, _, sv, sp = scatter(verts[b], pb, faces, face_parts, meas, dout[b])
        # (a case must not hold an element whose terms all vanish in exact arithmetic -- the corner of a face [i, i, j] facing the repeated
        # pair, alone at its vertex -- since autograd leaves rounding noise there and S, rightly, is 0: nothing would bound the comparison)
        assert ((sv > 0) | (gv == 0) | np.isnan(gv)).all() and ((sp > 0) | (gp == 0) | np.isnan(gp)).all(), 'body %d: an element with S == 0 is not exactly 0' % b
        res.append((gv, gp, sv, sp))
    return tuple(np.stack([r[i] for r in res]) for i in range(4))


# ---- the conditions a case must satisfy ---------------------------------------------------------------------------------------------
def assert_conditions(verts, points, faces, face_parts, meas, allow_extent_ties=False):
    """asserts, per body: no vertex of a cut face other than the anchor itself lies within MIN_PLANE_DISTANCE of a GIRTH plane; no two distinct
    vertices tie for an EXTENT extreme.  Bodies with a NaN are not looked at (their rows are compared as NaN patterns)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    for b in range(verts.shape[0]):
        V = verts[b].astype(np.float64)
        if np.isnan(V).any() or (points is not None and np.isnan(points[b]).any()):
            continue
        N = V.shape[0]
        for m, q in enumerate(meas):
            n = np.asarray(q['dir'], np.float64)
            if q['kind'] == GIRTH:
                a0 = q['anchor'][0]
                o = V[a0] if a0 < N else points[b][a0 - N].astype(np.float64)
                fs = faces[MC.selected_faces(faces, face_parts, N, q['part_mask'])]
                d = ((V[fs] - o) * n).sum(2) / np.sqrt((n ** 2).sum())
                cut, _ = _lone(d)
                near = (np.abs(d[cut]) < MIN_PLANE_DISTANCE) & (fs[cut] != a0)
                assert not near.any(), 'body %d, measurement %d: a vertex of a cut face lies %.3g m from the plane' % (b, m, np.abs(d[cut])[near].min())
            elif q['kind'] == EXTENT and not allow_extent_ties:
                h = V @ n
                assert (h == h.max()).sum() == 1 and (h == h.min()).sum() == 1, 'body %d, measurement %d: vertices tie for an extent extreme' % (b, m)


def random_dout(batch, n_meas, seed=0):
    """dout with zeros and negative entries"""
    rng = np.random.RandomState(4000 + seed)
    d = rng.uniform(-2, 2, (batch, n_meas)).astype(np.float32)
    d[rng.rand(batch, n_meas) < 0.15] = 0.0
    return d
