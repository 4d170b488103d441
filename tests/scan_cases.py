"""Test helper: the float64 reference of straps_scan_energy and of the composed scan fit, and their cases (tests/test_scan_cases_cpu.py,
tests/test_gpu_scan_energy.py, tests/test_gpu_fit_scan.py).

The objective of include/straps_hip.h restated in float64 torch with autograd.  It starts from the fp32-rounded X = verts + t, the defined
intermediate, and searches the distance matrix in column blocks, so that the largest case fits in memory.  `energies(..., near_v=, near_p=)`
accepts the indices the GPU chose, as silfit_cases.energies(nearest=...) does.  The composed fit runs on the oracle alone -- `O.rot6d_to_rotmat`,
`O.smpl_forward(MODEL, ..., dtype=float64)`, the priors of fit_cases.energy, `torch.optim.Adam` with three parameter groups.  All inputs come
from `detgen.det_uniform`.
"""
import numpy as np
import torch

import fit_cases as FC
import silfit_cases as SC
import straps_oracle as O
from detgen import det_uniform

F64 = torch.float64
MODEL = FC.MODEL
INF = float('inf')

# the constants of csrc/scanfit.hip that decide which path a case takes
LANES = 256                # BLK: lanes of a workgroup = points / vertices of a partial sum
POINTS_PER_LANE = 4        # PPL: queries a lane of the search holds in registers
CHUNK = LANES * POINTS_PER_LANE      # QCHUNK: queries of a work item
VERTEX_TILE = 1024         # VTILE: vertices one LDS tile holds when the points search
POINT_TILE = 1024          # PTILE: points one LDS tile holds when the vertices search
WORKGROUPS = 512           # WPB: workgroups per body of a search; they walk the body's work items (query chunks x candidate tiles)
GATHER_TILE = 4096         # GTILE: entries of the nearest list a workgroup of the gather sifts between two barriers (a quarter per wave)


def path_facts(spec):
    """(nverts, npoints, ...) -> the paths of csrc/scanfit.hip the case takes.  Per search ('s2m': the points are the queries, the vertices
    the candidates; 'm2s': the other way round): 'chunks' of 1024 queries, 'ragged' (the last chunk is not whole), 'tiles' of candidates,
    'items' = chunks x tiles, 'trips' = (fewest, most) items walked by a workgroup.  'gather_tiles' of the nearest list, 'point_trips' /
    'vertex_trips' of scan_finish_kernel's strided sums over the per-256 partials."""
    nverts, npoints = spec[:2]
    up = lambda a, b: -(-a // b)

    def search(nq, nc, tile):
        chunks, tiles = up(nq, CHUNK), up(nc, tile)
        items = chunks * tiles
        groups = min(items, WORKGROUPS)
        return {'chunks': chunks, 'ragged': nq % CHUNK != 0, 'tiles': tiles, 'items': items, 'trips': (items // groups, up(items, groups))}
    return {'s2m': search(npoints, nverts, VERTEX_TILE), 'm2s': search(nverts, npoints, POINT_TILE), 'gather_tiles': up(npoints, GATHER_TILE),
            'point_trips': up(up(npoints, LANES), LANES), 'vertex_trips': up(up(nverts, LANES), LANES)}


# ------------------------------------------------------------------ the search
def _sq_block(Q, Cb):
    """[n,3], [m,3] -> [n,m] squared distances, in place on one temporary per axis"""
    d = Q[:, 0:1] - Cb[None, :, 0]
    d.mul_(d)
    for k in (1, 2):
        e = Q[:, k:k + 1] - Cb[None, :, k]
        e.mul_(e)
        d.add_(e)
    return d


def _sq_block_fp32(Q, Cb):
    """the kernel's own chain on fp32 inputs: fp32 differences, then fmaf(dz, dz, fmaf(dy, dy, dx * dx)).  A float64 product of two fp32 values
    is exact, so every fmaf is one float64 addition rounded to fp32 (a double rounding, which moves an fp32 result in about one of 2^29 cases)."""
    dx, dy, dz = (Q[:, k:k + 1] - Cb[None, :, k] for k in range(3))      # float32
    a = dx * dx
    a = (dy.double().pow_(2).add_(a.double())).float()
    return (dz.double().pow_(2).add_(a.double())).float()


def nearest(Q, C, fp32=False, budget=1 << 22):
    """Q [n,3], C [m,3] (float64, or float32 with fp32=True; candidates with a non-finite coordinate do not count)
    -> (index [n] of the lowest candidate among the minima, -1 without one; best [n]; second best [n]); searched in column blocks"""
    n, m = Q.shape[0], C.shape[0]
    dt = torch.float32 if fp32 else F64
    best, second = torch.full((n,), INF, dtype=dt), torch.full((n,), INF, dtype=dt)
    index = torch.full((n,), -1, dtype=torch.int64)
    ok = torch.isfinite(C).all(dim=1)
    rows = torch.arange(n)
    step = max(1, budget // max(1, n))
    for c0 in range(0, m, step):
        Cb = C[c0:c0 + step]
        d = _sq_block_fp32(Q, Cb) if fp32 else _sq_block(Q, Cb)
        d[:, ~ok[c0:c0 + step]] = INF
        b1, i1 = d.min(dim=1)
        i1 = torch.where(d == b1[:, None], torch.arange(d.shape[1])[None, :], torch.full((1, 1), d.shape[1])).min(dim=1).values      # the FIRST minimum
        d[rows, i1] = INF
        s1 = d.min(dim=1).values
        second = torch.minimum(torch.minimum(second, s1), torch.maximum(best, b1))
        take = b1 < best                                                  # strict: an earlier block keeps an equal distance
        index = torch.where(take, i1 + c0, index)
        best = torch.where(take, b1, best)
    return index, best, second


def translated(verts, trans):
    """fp32 [B,V,3], [B,3] -> X = verts + t rounded to fp32 (one rounding per component), as float64"""
    return (verts.float() + trans.float()[:, None, :]).double()


def rho(r2, sigma):
    return sigma * sigma * r2 / (sigma * sigma + r2) if sigma > 0 else r2


def energies(X, P, sigma, w_s2m=1.0, w_m2s=1.0, near_v=None, near_p=None):
    """float64 restatement: X [B,V,3] (may require grad), P [B,N,3] (non-finite rows are invalid points)
    -> (E_s2m [B], E_m2s [B], nearest_vertex [B,N], nearest_point [B,V]); with a weight of 0 that search is skipped (energy 0, indices -1).
    near_v / near_p given: those partners are used."""
    B, V, N = X.shape[0], X.shape[1], P.shape[1]
    e_s, e_m, nv, npt = [], [], [], []
    for b in range(B):
        valid = torch.isfinite(P[b]).all(dim=1)
        zero = (X[b] * 0.0).sum()
        iv, ip = torch.full((N,), -1, dtype=torch.int64), torch.full((V,), -1, dtype=torch.int64)
        es, em = zero, zero
        if bool(valid.any()):
            if w_s2m != 0:
                if near_v is None:
                    iv[valid] = nearest(P[b][valid], X[b].detach())[0]
                else:
                    iv = torch.as_tensor(near_v[b]).long().clone()
                use = valid & (iv >= 0)
                r2 = ((X[b][iv[use]] - P[b][use]) ** 2).sum(dim=1)
                es = rho(r2, sigma).sum() / max(1, int(valid.sum()))
            if w_m2s != 0:
                ip = nearest(X[b].detach(), P[b])[0] if near_p is None else torch.as_tensor(near_p[b]).long().clone()
                use = ip >= 0
                r2 = ((X[b][use] - P[b][ip[use]]) ** 2).sum(dim=1)
                em = rho(r2, sigma).sum() / V
        e_s.append(es), e_m.append(em), nv.append(iv), npt.append(ip)
    return torch.stack(e_s), torch.stack(e_m), torch.stack(nv), torch.stack(npt)


def energies_grad(verts, trans, points, sigma, w_s2m, w_m2s, near_v=None, near_p=None):
    """fp32 inputs -> (energy2 [B,2], dverts [B,V,3], dtrans [B,3], nearest_vertex, nearest_point) of w_s2m E_s2m + w_m2s E_m2s, float64, by
    autograd from X = fp32(verts + t): dverts = dE/dX, dtrans = the sum of its rows"""
    X = translated(verts, trans).requires_grad_(True)
    e_s, e_m, nv, npt = energies(X, points.double(), sigma, w_s2m, w_m2s, near_v, near_p)
    g, = torch.autograd.grad((w_s2m * e_s + w_m2s * e_m).sum(), X, allow_unused=True)
    g = torch.zeros_like(X) if g is None else g
    return torch.stack([e_s, e_m], dim=1).detach(), g, g.sum(dim=1), nv, npt


# ------------------------------------------------------------------ the cases
BOX = np.array([0.5, 1.0, 0.3])      # half extents of the box the vertices and points are drawn in (metres)


def scan_case(nverts, npoints, B, seed, sigma=0.0, w_s2m=100.0, w_m2s=70.0, nan_body=None, tail_nan_body=None, scattered_nan_body=None, tie=False):
    """-> dict: 'verts' [B,V,3], 'trans' [B,3], 'points' [B,N,3] float32 and the arguments.  Vertices and points are independent uniform draws
    in one box (the points moved by t, so that the clouds overlap).  nan_body: all points of that body are NaN.  tail_nan_body: the last third
    of that body's points is NaN (a ragged batch).  scattered_nan_body: about one point in twenty of that body has a NaN or an infinity in one
    coordinate.  tie (body 0; at least 6 vertices and 4 points): vertex 5 is an exact copy of vertex 2 with point 0 placed 1 mm from them, and
    point 3 an exact copy of point 1 with vertex 4 placed 1 mm from them -- each pair is somebody's nearest."""
    u = lambda shape, k, lo=-1.0, hi=1.0: det_uniform(shape, seed + k, lo, hi).astype(np.float64)
    verts = (u((B, nverts, 3), 1) * BOX).astype(np.float32)
    trans = u((B, 3), 2, -0.2, 0.2).astype(np.float32)
    points = (u((B, npoints, 3), 3) * BOX + trans[:, None, :]).astype(np.float32)
    dup = None
    if tie:
        assert nverts >= 6 and npoints >= 4
        verts[0, 5] = verts[0, 2]
        points[0, 0] = verts[0, 2] + trans[0] + np.float32(1e-3)
        points[0, 3] = points[0, 1]
        verts[0, 4] = points[0, 1] - trans[0] + np.float32(1e-3)
        dup = {'vertex': (2, 5), 'point': (1, 3)}
    if nan_body is not None:
        points[nan_body] = np.nan
    if tail_nan_body is not None:
        points[tail_nan_body, npoints - npoints // 3:] = np.nan
    if scattered_nan_body is not None:
        pick = u((npoints,), 4, 0.0, 1.0)
        axis = (u((npoints,), 5, 0.0, 1.0) * 3).astype(np.int64).clip(0, 2)
        bad = np.flatnonzero(pick < 0.05)
        bad = bad[bad >= 4] if tie and scattered_nan_body == 0 else bad
        points[scattered_nan_body, bad, axis[bad]] = np.where(pick[bad] < 0.04, np.nan, np.where(pick[bad] < 0.045, np.inf, -np.inf)).astype(np.float32)
    return {'verts': torch.from_numpy(verts), 'trans': torch.from_numpy(trans), 'points': torch.from_numpy(points), 'sigma': sigma, 'w_s2m': w_s2m,
            'w_m2s': w_m2s, 'dup': dup, 'seed': seed, 'nan_body': nan_body}


def searches(case):
    """the float64 search of a case, both directions whatever the weights -> per body (nearest_vertex [N] (-1 at invalid points), best, second,
    nearest_point [V], best, second).  With `dup`, the gaps (second over best) are those of the case without the higher copies."""
    X, P = translated(case['verts'], case['trans']), case['points'].double()
    out = []
    for b in range(X.shape[0]):
        valid = torch.isfinite(P[b]).all(dim=1)
        N, V = P.shape[1], X.shape[1]
        iv, bv, sv = torch.full((N,), -1, dtype=torch.int64), torch.full((N,), INF, dtype=F64), torch.full((N,), INF, dtype=F64)
        if bool(valid.any()):
            iv[valid], bv[valid], sv[valid] = nearest(P[b][valid], X[b])
        ip, bp, sp = nearest(X[b], P[b])
        if case['dup'] is not None and b == 0 and max(N, V) <= EXACT_MAX_POINTS:      # (the larger cases are judged by excess, not by their gaps)
            keep_v, keep_p = torch.ones(V, dtype=torch.bool), torch.ones(N, dtype=torch.bool)
            keep_v[case['dup']['vertex'][1]] = False
            keep_p[case['dup']['point'][1]] = False
            sv[valid] = nearest(P[b][valid], X[b][keep_v])[2]
            sp = sp.clone()
            sp[keep_v] = nearest(X[b][keep_v], P[b][keep_p])[2]
        out.append((iv, bv, sv, ip, bp, sp))
    return out


def input_conditions(case, found=None):
    """evaluated in float64 on the case's fp32 inputs -> {'gap': the smallest relative difference between the best and the second-best squared
    distance of a valid point or a vertex (planted copies count as one), 'min_d2': the smallest best squared distance, 'valid': valid points}"""
    gap, min_d2, nvalid = INF, INF, 0
    for iv, bv, sv, ip, bp, sp in (searches(case) if found is None else found):
        for best, second in ((bv[iv >= 0], sv[iv >= 0]), (bp[ip >= 0], sp[ip >= 0])):
            if best.numel():
                min_d2 = min(min_d2, float(best.min()))
                fin = torch.isfinite(second)
                if bool(fin.any()):
                    gap = min(gap, float(((second[fin] - best[fin]) / second[fin].clamp_min(1e-300)).min()))
        nvalid += int((iv >= 0).sum())
    return {'gap': gap, 'min_d2': min_d2, 'valid': nvalid}


EXACT_MAX_POINTS = 4096      # a case of up to so many points AND vertices must meet the gap condition, and the GPU's indices must be the float64 ones exactly
GAP = 1e-4
EXCESS = 2.0 ** -20          # larger cases: a differing partner's float64 squared distance may exceed the minimum by this much, relative
SHARE = 1e-4                 # and at most this share of a case's indices may differ at all

# name: (nverts, npoints, B, first seed, keyword arguments).  tests/test_scan_cases_cpu.py asserts, from path_facts, which paths these cases reach.
SPECS = {
    'v1_p1': (1, 1, 1, 9100, {}),
    'v63_p65_nan_body': (63, 65, 3, 9200, {'nan_body': 1, 'sigma': 0.05}),
    'v64_p64': (64, 64, 1, 9300, {}),
    'v257_p1025_ties': (257, 1 + CHUNK, 1, 9400, {'tie': True, 'sigma': 0.1}),                  # one chunk and one point; two point tiles
    'v1025_p257': (VERTEX_TILE + 1, 257, 1, 9500, {}),                                           # two vertex tiles; a second, ragged chunk of vertices
    'v257_p1025': (257, POINT_TILE + 1, 3, 9600, {'scattered_nan_body': 2, 'sigma': 0.05}),      # two point tiles, three bodies
    'v1024_p2048': (1024, 2048, 1, 9700, {}),                                                    # whole chunks and whole tiles on both sides
    'v65_p70_s2m_only': (65, 70, 3, 9800, {'w_m2s': 0.0, 'nan_body': 0}),
    'v65_p70_m2s_only': (65, 70, 3, 9900, {'w_s2m': 0.0, 'sigma': 0.05, 'tail_nan_body': 1}),
    # more work items than workgroups in either search: two workgroups walk one item more than the others; 2053 partial sums of points
    'v65_p525313': (65, CHUNK * WORKGROUPS + CHUNK + 1, 1, 10000, {}),
    'v65537_p64': (65537, 64, 1, 10100, {'sigma': 0.1}),                                         # 257 partial sums of vertices, 65 vertex tiles
    'v6890_p16384': (6890, 16384, 3, 10200, {'tail_nan_body': 1, 'scattered_nan_body': 2, 'tie': True, 'sigma': 0.1}),      # the workload's size
}
_CASES = {}


def exact(name):
    """the case is small enough to be held to the gap condition (SPECS: every case of up to 4096 points is)"""
    return max(SPECS[name][:2]) <= EXACT_MAX_POINTS


def get_case(name, max_seeds=40):
    """the named case, once per process, with 'conditions' and 'searches' (the float64 search).  Up to EXACT_MAX_POINTS points: at the first
    seed (counting up from the listed one) whose inputs meet the gap condition; nothing is dropped from a case to make it qualify."""
    if name not in _CASES:
        nv, npts, B, seed, kw = SPECS[name]
        for k in range(max_seeds):
            case = scan_case(nv, npts, B, seed + 11 * k, **kw)
            found = searches(case)
            cond = input_conditions(case, found)
            if max(nv, npts) > EXACT_MAX_POINTS or cond['gap'] > GAP:
                case['conditions'] = cond
                case['searches'] = found
                _CASES[name] = case
                break
        else:
            raise AssertionError('no seed of case %s meets the input conditions (last: %r)' % (name, cond))
    return _CASES[name]


def index_differences(case, near_v, near_p):
    """the indices somebody chose (near_v [B,N], near_p [B,V]) against the float64 search of the case, in the directions its weights enable
    -> (number that differ, number compared, worst relative excess of a differing partner's float64 squared distance over the minimum)"""
    X, P = translated(case['verts'], case['trans']), case['points'].double()
    differ, total, worst = 0, 0, 0.0
    for b, (iv, bv, _, ip, bp, _) in enumerate(case['searches']):
        pairs = []
        if case['w_s2m'] != 0:
            pairs.append((torch.as_tensor(near_v[b]).long(), iv, bv, P[b], X[b]))
        if case['w_m2s'] != 0:
            pairs.append((torch.as_tensor(near_p[b]).long(), ip, bp, X[b], P[b]))
        for got, want, best, Q, Cd in pairs:
            assert bool(((got >= 0) == (want >= 0)).all()), 'a partner is reported where there is none, or none where there is one'
            bad = got != want
            total += int((want >= 0).sum())
            differ += int(bad.sum())
            if bool(bad.any()):
                d = ((Q[bad] - Cd[got[bad]]) ** 2).sum(dim=1)
                worst = max(worst, float(((d - best[bad]) / best[bad]).max()))
    return differ, total, worst


def fp32_indices(case):
    """the search by the kernel's own fp32 chain, emulated on the CPU -> (near_v [B,N], near_p [B,V])"""
    X, P = (case['verts'] + case['trans'][:, None, :]), case['points']
    nv, npt = [], []
    for b in range(X.shape[0]):
        valid = torch.isfinite(P[b]).all(dim=1)
        iv = torch.full((P.shape[1],), -1, dtype=torch.int64)
        if bool(valid.any()):
            iv[valid] = nearest(P[b][valid], X[b], fp32=True)[0]
        nv.append(iv)
        npt.append(nearest(X[b], P[b], fp32=True)[0])
    return torch.stack(nv), torch.stack(npt)


# ------------------------------------------------------------------ the composed fit
def mesh(est):
    """est [B,157] float64 (translation | 6-D pose | shape) -> the posed vertices with the translation added [B,6890,3]"""
    return SC.mesh(est) + est[:, None, :3]


def objective(est, est0, points, sigma, w_s2m, w_m2s, near_v=None, near_p=None, lambda_pose=1e-3, lambda_shape=1e-3):
    """all float64 -> (E [B], terms [B,3] = (the priors, E_s2m, E_m2s), nearest_vertex, nearest_point)"""
    prior = lambda_pose * ((est[:, 3:147] - est0[:, 3:147]) ** 2).sum(dim=1) + lambda_shape * ((est[:, 147:] - est0[:, 147:]) ** 2).sum(dim=1)
    e_s, e_m, nv, npt = energies(mesh(est), points, sigma, w_s2m, w_m2s, near_v, near_p)
    return prior + w_s2m * e_s + w_m2s * e_m, torch.stack([prior, e_s, e_m], dim=1), nv, npt


def objective_grad(est, est0, points, sigma, w_s2m, w_m2s, **kw):
    x = est.clone().requires_grad_(True)
    E, terms, _, _ = objective(x, est0, points, sigma, w_s2m, w_m2s, **kw)
    g, = torch.autograd.grad(E.sum(), x)
    return E.detach(), g, terms.detach()


def adam_fit(est, est0, points, iters, sigma, w_s2m, w_m2s, lr=(0.01, 0.01, 0.01), betas=(0.9, 0.999), eps=1e-8, **kw):
    """torch.optim.Adam, parameter groups (t, x6, beta) -> (final est [B,157], terms [iters+1,B,3])"""
    t, x6, beta = (est[:, a:b].clone().requires_grad_(True) for a, b in ((0, 3), (3, 147), (147, 157)))
    opt = torch.optim.Adam([{'params': [t], 'lr': lr[0]}, {'params': [x6], 'lr': lr[1]}, {'params': [beta], 'lr': lr[2]}], betas=betas, eps=eps)
    trace = []
    for i in range(iters + 1):
        opt.zero_grad()
        E, terms, _, _ = objective(torch.cat([t, x6, beta], dim=1), est0, points, sigma, w_s2m, w_m2s, **kw)
        trace.append(terms.detach().clone())
        if i == iters:
            break
        E.sum().backward()
        opt.step()
    return torch.cat([t, x6, beta], dim=1).detach(), torch.stack(trace)


# the prototype's recipe: the two bodies of the silhouette trajectory recipe (silfit_cases._target: the mean parameters as start; the true body's
# shape is the mean moved by N(0, 1) draws, its 6-D pose the mean moved by 0.05 N(0, 1)), no translation; the scan is every third vertex of the
# true body moved by N(0, 2 mm) noise; 80 Adam iterations at lr 0.01, weights 100 and 100, sigma 0
TRAJ = dict(B=2, iters=80, lr=(0.01, 0.01, 0.01), sigma=0.0, w_s2m=100.0, w_m2s=100.0, lambda_pose=1e-3, lambda_shape=1e-3, every=3, noise=2e-3)
_TRAJ = {}


def scan_bodies(streams):
    """-> dict: 'est' [B,157] float32 (the start, translation zero), 'true' [B,157] float32, 'points' [B,2297,3] float32, 'true_verts' [B,6890,3]
    float64; once per process"""
    key = tuple(streams)
    if key not in _TRAJ:
        est, true, pts, tv = [], [], [], []
        for k in streams:
            start, tr = (a.copy() for a in SC._target(k)[:2])
            start[:3] = 0.0
            tr[:3] = 0.0
            with torch.no_grad():
                v = mesh(torch.from_numpy(tr[None]).double())[0]
            scan = v[::TRAJ['every']].numpy()
            scan = scan + TRAJ['noise'] * SC.det_normal(scan.shape, 7300 + 10 * k)
            est.append(start), true.append(tr), pts.append(scan.astype(np.float32)), tv.append(v)
        _TRAJ[key] = {'est': torch.from_numpy(np.stack(est)), 'true': torch.from_numpy(np.stack(true)), 'points': torch.from_numpy(np.stack(pts)),
                      'true_verts': torch.stack(tv)}
    return _TRAJ[key]


def trajectory_case():
    return scan_bodies(SC.TRAJ_STREAMS)


def three_body_case():
    """three bodies for the evaluation and loop tests at B = 3 (and, sliced, B = 1): the two of the trajectory case and one more draw"""
    return scan_bodies(SC.TRAJ_STREAMS + (13,))


def vertex_rms(est, true_verts):
    """est [B,157] -> the vertex-to-vertex RMS distance of its mesh to the true one [B] (float64)"""
    with torch.no_grad():
        return ((mesh(est.double()) - true_verts) ** 2).sum(dim=2).mean(dim=1).sqrt()


def trajectory_reference():
    """the float64 composed fit of the trajectory case -> {'est': final [B,157], 'terms': [81,B,3], 'rms0', 'rms': [B]}; once per process"""
    if 'fit' not in _TRAJ:
        c = trajectory_case()
        est = c['est'].double()
        final, terms = adam_fit(est, est.clone(), c['points'].double(), TRAJ['iters'], TRAJ['sigma'], TRAJ['w_s2m'], TRAJ['w_m2s'], lr=TRAJ['lr'],
                                lambda_pose=TRAJ['lambda_pose'], lambda_shape=TRAJ['lambda_shape'])
        _TRAJ['fit'] = {'est': final, 'terms': terms, 'rms0': vertex_rms(est, c['true_verts']), 'rms': vertex_rms(final, c['true_verts'])}
    return _TRAJ['fit']
