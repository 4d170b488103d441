"""Test helper: the float64 reference of straps_distance_field, straps_silhouette_energy, straps_fit_adam and the composed silhouette fit,
and their cases (tests/test_silfit_cases_cpu.py, tests/test_gpu_distance_field.py, tests/test_gpu_silhouette_energy.py,
tests/test_gpu_fit_silhouette.py).

The objective of include/straps_hip.h restated in float64: a brute-force distance transform (every pixel against every foreground pixel; a
row-blocked two-pass transform, held equal to it on the CPU, stands in above 257 pixels), the two energies in torch with autograd for the gradients, and the composed fit on the oracle alone -- `O.rot6d_to_rotmat`,
`O.smpl_forward(MODEL, ..., dtype=float64)`, `O.orthographic_project`, `fit_cases.energy` for the keypoint and prior terms, `torch.optim.Adam`
with three parameter groups.  All inputs come from `detgen.det_uniform`.
"""
import numpy as np
import torch

import eval_cases as EC
import fit_cases as FC
import straps_oracle as O
from detgen import det_uniform
from straps_amd.synthetic_smpl import synthetic_mean_params

F64 = torch.float64
MODEL = FC.MODEL


def det_normal(shape, seed):
    """standard normal draws from two det_uniform streams (Box-Muller), float64"""
    u1 = det_uniform(shape, seed, 0.0, 1.0).astype(np.float64)
    u2 = det_uniform(shape, seed + 1000003, 0.0, 1.0).astype(np.float64)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


# ------------------------------------------------------------------ distance transform
def sentinel(wh):
    return 2 * wh * wh


def brute_d2(mask):
    """mask [wh,wh] (any non-zero = foreground) -> int32 [wh,wh]: every pixel against every foreground pixel"""
    mask = np.asarray(mask)
    wh = mask.shape[0]
    fg = torch.from_numpy(np.argwhere(mask != 0).astype(np.int32))
    if fg.shape[0] == 0:
        return np.full((wh, wh), sentinel(wh), np.int32)
    rr, cc = torch.meshgrid(torch.arange(wh, dtype=torch.int32), torch.arange(wh, dtype=torch.int32), indexing='ij')
    P = torch.stack([rr.reshape(-1), cc.reshape(-1)], dim=1)
    out = torch.empty(wh * wh, dtype=torch.int32)
    step = max(1, (1 << 21) // fg.shape[0])      # (8 MiB per temporary, in place: three times as fast as 64 MiB ones and `** 2`)
    for a in range(0, wh * wh, step):
        p = P[a:a + step]
        d = p[:, None, 0] - fg[None, :, 0]
        d.mul_(d)
        e = p[:, None, 1] - fg[None, :, 1]
        e.mul_(e)
        out[a:a + step] = d.add_(e).min(dim=1).values
    return out.view(wh, wh).numpy()


ROW_BLOCK = 8      # rows per block of the row pass: [8, wh, wh] int32 is 32 MiB at wh = 1024 (all rows at once would be 4 GiB)


def two_pass_d2(mask):
    """the same transform as a column pass (distance to the nearest foreground row of the column) and a row pass (min over c' of
    (c - c')^2 + g(c')^2): the structure of csrc/silfit.hip, in integers.  The row pass runs over blocks of ROW_BLOCK rows (a row's result
    depends on that row of g alone, so the blocking changes nothing); every value stays below 3 * wh * wh <= 2^22, int32 holds it."""
    mask = np.asarray(mask) != 0
    wh = mask.shape[0]
    far = 2 * wh
    g = np.full((wh, wh), far, np.int64)
    run = np.full(wh, far, np.int64)
    for r in range(wh):
        run = np.where(mask[r], 0, np.minimum(run + 1, far))
        g[r] = run
    run = np.full(wh, far, np.int64)
    for r in range(wh - 1, -1, -1):
        run = np.where(mask[r], 0, np.minimum(run + 1, far))
        g[r] = np.minimum(g[r], run)
    g2 = torch.from_numpy(np.where(g >= far, sentinel(wh), g * g).astype(np.int32))
    c = torch.arange(wh, dtype=torch.int32)
    dc2 = (c[:, None] - c[None, :]) ** 2                                   # [c][c']
    out = torch.empty(wh, wh, dtype=torch.int32)
    for r0 in range(0, wh, ROW_BLOCK):
        out[r0:r0 + ROW_BLOCK] = (dc2[None, :, :] + g2[r0:r0 + ROW_BLOCK, None, :]).min(dim=2).values
    return out.clamp_(max=sentinel(wh)).numpy()


def mask_cases(wh):
    """-> ordered {name: uint8 [wh,wh]}: empty, full, one pixel in each corner, random at density 0.4 (foreground bytes 2 and 255) and 0.01"""
    z = np.zeros((wh, wh), np.uint8)
    out = {'empty': z.copy(), 'full': np.full((wh, wh), 1, np.uint8)}
    for name, (r, c) in (('corner_tl', (0, 0)), ('corner_tr', (0, wh - 1)), ('corner_bl', (wh - 1, 0)), ('corner_br', (wh - 1, wh - 1))):
        m = z.copy()
        m[r, c] = 255
        out[name] = m
    u = det_uniform((wh, wh), 5100 + wh, 0.0, 1.0)
    byte = np.where(det_uniform((wh, wh), 5200 + wh, 0.0, 1.0) < 0.5, 2, 255).astype(np.uint8)
    out['rand04'] = np.where(u < 0.4, byte, 0).astype(np.uint8)
    out['rand001'] = np.where(det_uniform((wh, wh), 5300 + wh, 0.0, 1.0) < 0.01, byte, 0).astype(np.uint8)
    return out


def mask_batches(wh):
    """-> list of (names, uint8 [B,wh,wh]) with B in {1, 3}: every case alone, and batches of three -- among them an empty frame between two
    non-empty ones"""
    mc = mask_cases(wh)
    out = [((k,), v[None].copy()) for k, v in mc.items()]
    for names in (('rand04', 'empty', 'rand001'), ('full', 'corner_tl', 'corner_br'), ('corner_tr', 'corner_bl', 'rand04')):
        out.append((names, np.stack([mc[n] for n in names])))
    return out


SPARSE = ('corner_tl', 'corner_tr', 'corner_bl', 'corner_br', 'rand1e4')


def sparse_mask_cases(wh):
    """-> ordered {name: uint8 [wh,wh]} of the masks on which brute force stays affordable at wh = 1024: the four corner cases of mask_cases
    and a random one at density 1e-4 (about a hundred foreground pixels at wh = 1000; pixel (wh // 2, wh // 3) is set, so it is never empty)"""
    mc = mask_cases(wh)
    out = {k: mc[k] for k in SPARSE[:4]}
    m = (det_uniform((wh, wh), 5400 + wh, 0.0, 1.0) < 1e-4).astype(np.uint8) * 255
    m[wh // 2, wh // 3] = 255
    out['rand1e4'] = m
    return out


def _mask(wh, name):
    return sparse_mask_cases(wh)[name] if name == 'rand1e4' else mask_cases(wh)[name]


_D2 = {}


def reference_d2(wh, name):
    """brute-force transform of a mask case, computed once per process"""
    if (wh, name) not in _D2:
        _D2[(wh, name)] = brute_d2(_mask(wh, name))
    return _D2[(wh, name)]


_D2_TWO_PASS = {}


def reference_d2_two_pass(wh, name):
    """the row-blocked two-pass transform of a mask case, computed once per process: the reference above wh = 257, where brute force on a dense
    mask is out of reach (tests/test_silfit_cases_cpu.py holds the two equal at every size up to 257 on all masks, and at 1000 and 1024 on the
    sparse ones)"""
    if (wh, name) not in _D2_TWO_PASS:
        _D2_TWO_PASS[(wh, name)] = two_pass_d2(_mask(wh, name))
    return _D2_TWO_PASS[(wh, name)]


BRUTE_MAX_WH = 257
LARGE_BATCHES = (('rand04',), ('full',), ('empty',), ('rand001', 'empty', 'corner_br'))


def distance_field_batches(wh):
    """-> list of (names, uint8 [B,wh,wh], int32 [B,wh,wh] reference) for the GPU test.  Up to BRUTE_MAX_WH: all of mask_batches against brute
    force.  Above: LARGE_BATCHES (dense, full, empty, and an empty frame between two others) against the two-pass."""
    if wh <= BRUTE_MAX_WH:
        return [(names, masks, np.stack([reference_d2(wh, n) for n in names])) for names, masks in mask_batches(wh)]
    mc = mask_cases(wh)
    return [(names, np.stack([mc[n] for n in names]), np.stack([reference_d2_two_pass(wh, n) for n in names])) for names in LARGE_BATCHES]


# ------------------------------------------------------------------ the two energies
def grid_coords(verts, cam, wh):
    """[B,N,3], [B,3] (float64) -> g [B,N,2] = (column, row) grid coordinates"""
    p = O.orthographic_project(verts, cam)
    return (p + 1.0) * (wh / 2.0) - 0.5


def lattice_points(mask, lattice):
    """mask [wh,wh] -> (a [nl*nl,2] float64 (x = column, y = row), valid [nl*nl] bool), row-major over (i, j)"""
    wh = mask.shape[0]
    lattice = min(lattice, wh)
    idx = np.arange(0, wh, lattice)
    ii, jj = np.meshgrid(idx, idx, indexing='ij')
    a = np.stack([jj.reshape(-1), ii.reshape(-1)], axis=1).astype(np.float64)
    valid = (np.asarray(mask)[ii.reshape(-1), jj.reshape(-1)] != 0)
    return torch.from_numpy(a), torch.from_numpy(valid)


def nearest_vertices(g, a):
    """g [N,2], a [P,2] float64 -> (lowest index of the minimum [P], squared distances [P,N])"""
    d = ((g[None, :, :] - a[:, None, :]) ** 2).sum(dim=2)
    n = g.shape[0]
    first = torch.where(d == d.min(dim=1, keepdim=True).values, torch.arange(n)[None, :], torch.full((1, 1), n)).min(dim=1).values
    return first, d


def energies(verts, cam, masks, d2, lattice, tau, nearest=None):
    """float64 restatement: verts [B,N,3], cam [B,3] (torch float64, may require grad), masks uint8 [B,wh,wh], d2 int [B,wh,wh] (numpy)
    -> (E_in [B], E_out [B], nearest [B,nl*nl] int64 with -1 at invalid points).  `nearest` given: those vertices are used for E_out."""
    B, N, wh = verts.shape[0], verts.shape[1], masks.shape[1]
    g = grid_coords(verts, cam, wh)
    unit = 2.0 / wh
    e_in, e_out, near = [], [], []
    for b in range(B):
        a, valid = lattice_points(masks[b], lattice)
        if int(d2[b, 0, 0]) >= sentinel(wh):
            zero = (g[b] * 0.0).sum()
            e_in.append(zero)
            e_out.append(zero)
            near.append(torch.full((a.shape[0],), -1, dtype=torch.int64))
            continue
        D = torch.from_numpy(np.sqrt(np.asarray(d2[b], np.float64)))
        q = g[b].clamp(0.0, wh - 1.0)
        off = g[b] - q
        clamped = (off.detach() != 0).any(dim=1)
        o2 = (off ** 2).sum(dim=1)
        o = torch.where(clamped, torch.where(clamped, o2, torch.ones_like(o2)).sqrt(), torch.zeros_like(o2))
        cell = q.detach().floor().clamp(max=wh - 2.0)
        f = q - cell
        ix, iy = cell[:, 0].long(), cell[:, 1].long()
        fx, fy = f[:, 0], f[:, 1]
        Dv = (1 - fy) * ((1 - fx) * D[iy, ix] + fx * D[iy, ix + 1]) + fy * ((1 - fx) * D[iy + 1, ix] + fx * D[iy + 1, ix + 1])
        e_in.append((((Dv + o) * unit) ** 2).mean())
        nb = torch.full((a.shape[0],), -1, dtype=torch.int64)
        if bool(valid.any()):
            av = a[valid]
            if nearest is None:
                first, _ = nearest_vertices(g[b].detach(), av)
            else:
                first = torch.as_tensor(nearest[b]).reshape(-1).long()[valid]
            r = ((g[b][first] - av) ** 2).sum(dim=1)
            pos = r.detach() > 0
            r = torch.where(pos, torch.where(pos, r, torch.ones_like(r)).sqrt(), torch.zeros_like(r))
            h = (r - tau).clamp(min=0.0) * unit
            e_out.append((h ** 2).sum() / int(valid.sum()))
            nb[valid] = first
        else:
            e_out.append((g[b] * 0.0).sum())
        near.append(nb)
    return torch.stack(e_in), torch.stack(e_out), torch.stack(near)


def energies_grad(verts, cam, masks, d2, lattice, tau, w_in, w_out, nearest=None):
    """-> (energy2 [B,2], dverts [B,N,3], dcam [B,3], nearest) of w_in E_in + w_out E_out, float64, by autograd"""
    v = verts.clone().requires_grad_(True)
    c = cam.clone().requires_grad_(True)
    e_in, e_out, near = energies(v, c, masks, d2, lattice, tau, nearest)
    gv, gc = torch.autograd.grad((w_in * e_in + w_out * e_out).sum(), (v, c), allow_unused=True)
    gv = torch.zeros_like(v) if gv is None else gv
    gc = torch.zeros_like(c) if gc is None else gc
    return torch.stack([e_in, e_out], dim=1).detach(), gv, gc, near


def blob_mask(wh, seed):
    """an ellipse with random holes and a few stray pixels; bytes 1"""
    r, c = np.meshgrid(np.arange(wh), np.arange(wh), indexing='ij')
    u = det_uniform((4,), seed, 0.0, 1.0).astype(np.float64)
    cy, cx = wh * (0.4 + 0.2 * u[0]), wh * (0.4 + 0.2 * u[1])
    ry, rx = max(0.8, wh * (0.25 + 0.15 * u[2])), max(0.8, wh * (0.12 + 0.15 * u[3]))
    inside = ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0
    noise = det_uniform((wh, wh), seed + 1, 0.0, 1.0)
    m = (inside & (noise > 0.1)) | (noise > 0.995)
    if not m.any():
        m[min(wh - 1, int(cy)), min(wh - 1, int(cx))] = True
    return m.astype(np.uint8)


def energy_case(nverts, wh, lattice, tau, B, seed, empty_body=None, odd_only_body=None, tie=False, corner_fg=False):
    """-> dict: 'verts' [B,N,3] float32, 'cam' [B,3] float32, 'masks' uint8 [B,wh,wh], 'd2' int32 [B,wh,wh] (two_pass_d2), and the arguments.
    Grid coordinates are drawn as cell + U(0.05, 0.95) per axis (so no vertex sits near a cell boundary) and turned into vertices through
    the camera; with more than 8 vertices the first eight lie beyond the four sides and the four corners of the frame.  empty_body: that
    body's mask is empty.  odd_only_body: that body's foreground avoids every lattice point.  tie: vertex 1 is a copy of vertex 0 (wh >= 4:
    placed 0.3 px from a valid lattice point, so that the pair is somebody's nearest).  corner_fg: pixel (0, 0) is foreground."""
    u = lambda shape, k, lo, hi: det_uniform(shape, seed + k, lo, hi).astype(np.float64)
    cells = np.floor(u((B, nverts, 2), 1, 0.0, 1.0) * (wh - 1))
    g = cells + u((B, nverts, 2), 2, 0.05, 0.95)
    if nverts > 8:
        far = 1.3 + 4.0 * u((B, 8), 3, 0.0, 1.0)
        lo, hi = -far, wh - 1 + far
        mid = g[:, :8].copy()
        g[:, 0] = np.stack([lo[:, 0], mid[:, 0, 1]], 1)
        g[:, 1] = np.stack([hi[:, 1], mid[:, 1, 1]], 1)
        g[:, 2] = np.stack([mid[:, 2, 0], lo[:, 2]], 1)
        g[:, 3] = np.stack([mid[:, 3, 0], hi[:, 3]], 1)
        g[:, 4] = np.stack([lo[:, 4], lo[:, 4] - 0.7], 1)
        g[:, 5] = np.stack([hi[:, 5], lo[:, 5] + 0.4], 1)
        g[:, 6] = np.stack([lo[:, 6], hi[:, 6]], 1)
        g[:, 7] = np.stack([hi[:, 7] + 0.6, hi[:, 7]], 1)
    masks = np.stack([blob_mask(wh, seed + 100 + b) for b in range(B)])
    if corner_fg:            # (a lattice above wh - 1 leaves the single point (0, 0): make it a valid one)
        masks[:, 0, 0] = 1
    if empty_body is not None:
        masks[empty_body] = 0
    if odd_only_body is not None:
        lat = min(lattice, wh)
        masks[odd_only_body][::lat, ::lat] = 0
        assert lat > 1 and masks[odd_only_body].any()
    if tie:
        b = 0
        a, valid = lattice_points(masks[b], lattice)
        k = int(np.flatnonzero(valid.numpy())[len(np.flatnonzero(valid.numpy())) // 2])
        spot = a[k].numpy() + np.array([0.3, 0.05])
        spot = np.clip(spot, 0.05, wh - 1.05)
        first = 9 if nverts > 10 else 0
        g[b, first] = spot
        g[b, first + 1] = spot
    cam = np.array([0.9, 0.0, 0.0]) + np.concatenate([u((B, 1), 4, -0.1, 0.1), u((B, 2), 5, -0.05, 0.05)], axis=1)
    p = (g + 0.5) * (2.0 / wh) - 1.0
    xy = p / cam[:, None, 0:1] - cam[:, None, 1:3]
    verts = np.concatenate([xy, u((B, nverts, 1), 6, -0.3, 0.3)], axis=2).astype(np.float32)
    if tie:
        verts[0, first + 1] = verts[0, first]
    d2 = np.stack([two_pass_d2(m) for m in masks])
    return {'verts': torch.from_numpy(verts), 'cam': torch.from_numpy(cam.astype(np.float32)), 'masks': masks, 'd2': d2, 'wh': wh, 'lattice': lattice,
            'tau': tau, 'tie': (first, first + 1) if tie else None, 'seed': seed}


def input_conditions(case):
    """the margins that keep fp32 and float64 on the same branch, evaluated in float64 on the case's fp32 inputs:
    -> {'cell': smallest distance (px) of a grid coordinate to a cell boundary / the clamp border,
        'tau': smallest | r_a - tau | over the valid lattice points,
        'gap': smallest relative difference between the best and the second-best squared distance of a valid lattice point (the tied pair
               of a tie case counts as one vertex), 'points': valid lattice points, 'verts': vertices}"""
    wh, lattice, tau = case['wh'], case['lattice'], case['tau']
    g = grid_coords(case['verts'].double(), case['cam'].double(), wh)
    near_int = g.round().clamp(0.0, wh - 1.0)
    cell = float((g - near_int).abs().min())
    m_tau, gap, npts = float('inf'), float('inf'), 0
    for b in range(g.shape[0]):
        if int(case['d2'][b, 0, 0]) >= sentinel(wh):
            continue
        a, valid = lattice_points(case['masks'][b], lattice)
        if not bool(valid.any()):
            continue
        gb = g[b]
        if case['tie'] is not None and b == 0:
            keep = torch.ones(gb.shape[0], dtype=torch.bool)
            keep[case['tie'][1]] = False
            gb = gb[keep]
        _, d = nearest_vertices(gb, a[valid])
        npts += d.shape[0]
        if d.shape[1] > 1:
            two = d.topk(2, dim=1, largest=False).values
            gap = min(gap, float(((two[:, 1] - two[:, 0]) / two[:, 1].clamp_min(1e-300)).min()))
            best = two[:, 0]
        else:
            best = d[:, 0]
        m_tau = min(m_tau, float((best.sqrt() - tau).abs().min()))
    return {'cell': cell, 'tau': m_tau, 'gap': gap, 'points': npts, 'verts': g.shape[0] * g.shape[1]}


def conditions_hold(cond):
    return cond['cell'] > 1e-3 and cond['tau'] > 1e-3 and cond['gap'] > 1e-4


# the constants of csrc/silfit.hip that decide which path a case takes
LANES = 256                # BLK: lanes of a workgroup = lattice points of a chunk = vertices of a partial sum
VERTEX_TILE = 6912         # VTILE: projected vertices one LDS tile of the search holds
GATHER_TILE = 2048         # PTILE: entries of the nearest list one LDS tile of the gather holds
MAX_WORKGROUPS = 32        # MAX_NBP: workgroups per body of the search


def path_facts(spec):
    """(nverts, wh, lattice, ...) -> the paths of csrc/silfit.hip the case takes: 'vertex_tiles' (LDS tiles of the search; above one, the
    barriers and reloads sit inside the chunk loop), 'gather_tiles', 'chunks' of 256 lattice points, 'trips' = (fewest, most) chunks walked by a
    workgroup of the search, 'finish_trips' of sil_finish_kernel's strided sum over the per-256-vertex partials, 'wh'"""
    nverts, wh, lattice = spec[:3]
    up = lambda a, b: -(-a // b)
    nl = up(wh, min(lattice, wh))
    chunks = up(nl * nl, LANES)
    groups = min(chunks, MAX_WORKGROUPS)
    return {'vertex_tiles': up(nverts, VERTEX_TILE), 'gather_tiles': up(nl * nl, GATHER_TILE), 'chunks': chunks, 'trips': (chunks // groups, up(chunks, groups)),
            'finish_trips': up(up(nverts, LANES), LANES), 'wh': wh}


# (nverts, wh, lattice, tau, B, first seed, keyword arguments): every value the GPU test is asked to cover appears at least once, with the sizes at
# which the kernels change path; tests/test_silfit_cases_cpu.py (test_energy_cases_reach_every_path) asserts, from path_facts, which paths these
# cases reach -- a path named there cannot lose its last case unnoticed.  The first seeds of the cases above 8192 lattice points or 65 536
# vertices are those at which get_energy_case qualifies at once (a try at wh = 1024 costs a 1024 x 1024 transform).
ENERGY_SPECS = {
    'v1_wh2': (1, 2, 1, 0.0, 1, 6100, {}),
    'v63_wh16_l3': (63, 16, 3, 1.5, 3, 6200, {'empty_body': 1}),
    'v64_wh16_single_point': (64, 16, 17, 0.0, 1, 6300, {'corner_fg': True}),
    'v65_wh33_l4': (65, 33, 4, 1.5, 3, 6400, {'odd_only_body': 2}),
    'v257_wh33_l1_tie': (257, 33, 1, 0.0, 1, 6500, {'tie': True}),
    'v257_wh256_l3': (257, 256, 3, 0.0, 1, 6600, {}),
    'v7000_wh16_l1': (7000, 16, 1, 1.5, 1, 6700, {}),
    'v6890_wh256_l4': (6890, 256, 4, 1.5, 3, 6835, {'empty_body': 1, 'tie': True}),
    'v257_wh96_l1': (257, 96, 1, 1.5, 1, 8100, {}),                             # 36 chunks on 32 workgroups: four of them take two
    'v7000_wh96_l1': (7000, 96, 1, 0.0, 1, 8207, {}),                           # the same with two vertex tiles
    'v65_wh320_l3': (65, 320, 3, 1.5, 3, 8307, {'empty_body': 1}),              # 45 chunks, wh above 256
    'v65537_wh16_l2': (65537, 16, 2, 0.0, 1, 8400, {}),                         # ten vertex tiles, 257 partial sums
    'v65_wh1024_l8': (65, 1024, 8, 1.5, 1, 8535, {}),                           # 64 chunks: two whole trips in every workgroup, the largest wh
}
_CASES = {}


def get_energy_case(name, max_seeds=40):
    """the named case at the first seed (counting up from the listed one) whose inputs meet input_conditions; nothing is dropped from a case to
    make it qualify.  Computed once per process."""
    if name not in _CASES:
        nv, wh, lat, tau, B, seed, kw = ENERGY_SPECS[name]
        for k in range(max_seeds):
            case = energy_case(nv, wh, lat, tau, B, seed + 7 * k, **kw)
            cond = input_conditions(case)
            if conditions_hold(cond):
                case['conditions'] = cond
                _CASES[name] = case
                break
        else:
            raise AssertionError('no seed of case %s meets the input conditions (last: %r)' % (name, cond))
    return _CASES[name]


# ------------------------------------------------------------------ the composed fit
def mesh(est):
    """est [B,157] float64 -> vertices [B,6890,3]"""
    B = est.shape[0]
    R = O.rot6d_to_rotmat(est[:, 3:147].reshape(-1, 6)).view(B, 24, 3, 3)
    verts, _ = O.smpl_forward(MODEL, est[:, 147:], rotmats=R, dtype=F64)
    return verts


def objective(est, est0, masks, d2, targets, conf, lattice, tau, w_in, w_out, nearest=None, **kw):
    """all float64 -> (E [B], terms [B,3] = (E_kp with the priors, E_in, E_out)); targets / conf None: no keypoints (all confidences zero)"""
    B = est.shape[0]
    if targets is None:
        targets = torch.zeros(B, len(FC.COCO), 2, dtype=F64)
        conf = torch.zeros(B, len(FC.COCO), dtype=F64)
    e_kp, _ = FC.energy(est, est0, targets, conf, img_wh=float(masks.shape[1]), **kw)
    e_in, e_out, _ = energies(mesh(est), est[:, :3], masks, d2, lattice, tau, nearest)
    return e_kp + w_in * e_in + w_out * e_out, torch.stack([e_kp, e_in, e_out], dim=1)


def objective_grad(est, est0, masks, d2, targets, conf, lattice, tau, w_in, w_out, **kw):
    x = est.clone().requires_grad_(True)
    E, terms = objective(x, est0, masks, d2, targets, conf, lattice, tau, w_in, w_out, **kw)
    g, = torch.autograd.grad(E.sum(), x)
    return E.detach(), g, terms.detach()


def adam_fit(est, est0, masks, d2, targets, conf, iters, lattice, tau, w_in, w_out, lr=(0.01, 0.01, 0.01), betas=(0.9, 0.999), eps=1e-8, **kw):
    """torch.optim.Adam, parameter groups (cam, x6, beta) -> (final est [B,157], terms [iters+1,B,3])"""
    cam, x6, beta = (est[:, a:b].clone().requires_grad_(True) for a, b in ((0, 3), (3, 147), (147, 157)))
    opt = torch.optim.Adam([{'params': [cam], 'lr': lr[0]}, {'params': [x6], 'lr': lr[1]}, {'params': [beta], 'lr': lr[2]}], betas=betas, eps=eps)
    trace = []
    for i in range(iters + 1):
        opt.zero_grad()
        E, terms = objective(torch.cat([cam, x6, beta], dim=1), est0, masks, d2, targets, conf, lattice, tau, w_in, w_out, **kw)
        trace.append(terms.detach().clone())
        if i == iters:
            break
        E.sum().backward()
        opt.step()
    return torch.cat([cam, x6, beta], dim=1).detach(), torch.stack(trace)


TRAJ = dict(wh=64, lattice=2, tau=1.5, w_in=100.0, w_out=100.0, B=2, iters=80, lr=(0.01, 0.01, 0.01), lambda_pose=1e-3, lambda_shape=1e-3)
TRAJ_STREAMS = (24, 30)
_TRAJ = {}


def _target(stream):
    """one body of the trajectory recipe, rendered once per process: the mean parameters under cam (0.9, 0, 0) as start; target =
    eval_cases.wp_silhouette of the body whose shape is the mean moved by N(0, 1) draws and whose 6-D pose is the mean moved by 0.05 N(0, 1)
    -> (start [157], true [157] float32, mask uint8 [64,64], d2 int32 [64,64])"""
    if stream not in _TRAJ:
        mp = synthetic_mean_params(0)
        start = np.concatenate([[0.9, 0.0, 0.0], mp['pose'].astype(np.float64), mp['shape'].astype(np.float64)])
        true = start.copy()
        true[3:147] += 0.05 * det_normal((144,), 7100 + 10 * stream)
        true[147:] += det_normal((10,), 7200 + 10 * stream)
        start, true = start.astype(np.float32), true.astype(np.float32)
        with torch.no_grad():
            v = mesh(torch.from_numpy(true[None]).double()).float().numpy()
        mask = EC.wp_silhouette(v, MODEL['faces'], true[None, :3], TRAJ['wh'])[0]
        _TRAJ[stream] = (start, true, mask, two_pass_d2(mask))
    return _TRAJ[stream]


def _bodies(streams):
    parts = [_target(k) for k in streams]
    return {'est': torch.from_numpy(np.stack([p[0] for p in parts])), 'true': torch.from_numpy(np.stack([p[1] for p in parts])),
            'masks': np.stack([p[2] for p in parts]), 'd2': np.stack([p[3] for p in parts])}


def trajectory_case():
    """the standard trajectory case: synthetic model, 64 x 64 masks, two bodies of `_target`.
    -> dict: 'est' [B,157] float32 (the start), 'true' [B,157] float32, 'masks' uint8 [B,64,64], 'd2' int32.

    The targets are not typical draws.  The synthetic model's faces connect far-apart vertices, so its rendered silhouette is not the outline
    of its vertex cloud, and the float64 fit of any such target stops at a silhouette energy of 1.2e-4 .. 1.6e-4.  Most draws start at 2e-4 ..
    4e-4, so close to that floor that their ratio (0.35 .. 0.7 in float64) measures the floor, not the fit.  TRAJ_STREAMS are two draws that
    start far from it (1.1e-3 and 1.0e-3, like the 1.5e-3 of the prototype this case restates); their float64 fit reaches 0.12 and 0.14."""
    return _bodies(TRAJ_STREAMS)


def three_body_case():
    """three bodies for the evaluation and loop tests at B = 3 (and, sliced, B = 1): the two of the trajectory case and one more draw"""
    return _bodies(TRAJ_STREAMS + (13,))


def trajectory_reference():
    """the float64 composed fit of the standard trajectory case -> (final est, terms [81,B,3]); once per process"""
    if 'fit' not in _TRAJ:
        c = trajectory_case()
        est = c['est'].double()
        _TRAJ['fit'] = adam_fit(est, est.clone(), c['masks'], c['d2'], None, None, TRAJ['iters'], TRAJ['lattice'], TRAJ['tau'], TRAJ['w_in'], TRAJ['w_out'],
                                lr=TRAJ['lr'], lambda_pose=TRAJ['lambda_pose'], lambda_shape=TRAJ['lambda_shape'])
    return _TRAJ['fit']
