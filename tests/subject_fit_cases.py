"""Test helper: the float64 restatement of straps_fit_adam_subjects, straps_subject_mean_rows and the tied-shape fit, and their cases
(tests/test_subject_fit_cases_cpu.py, tests/test_gpu_fit_subjects.py).

`subject_update` is one call's arithmetic in float64 with the call's fp32 inputs taken as exact (sums of the counting frames, Adam by
`fit_cases.adam_update`); `subject_adam_fit` is the fit as `torch.optim.Adam` on per-frame cam and pose and ONE shape parameter per subject,
on top of the objectives of `fit_cases` / `silfit_cases`.  All inputs come from `detgen.det_uniform`.
"""
import numpy as np
import torch

import eval_cases as EC
import fit_cases as FC
import silfit_cases as SC
from detgen import det_uniform
from straps_amd.synthetic_smpl import synthetic_mean_params

F64 = torch.float64
NE = 157
EPS32 = 2.0 ** -23


def offsets_of(fps):
    return np.concatenate([[0], np.cumsum(fps)]).astype(np.int32)


def subject_of(fps):
    return torch.from_numpy(np.repeat(np.arange(len(fps)), fps).astype(np.int64))


def counting(lo, hi, mask):
    """rows of lo..hi-1 that count: all of them without a mask"""
    return [f for f in range(lo, hi) if mask is None or int(mask[f]) != 0]


# ------------------------------------------------------------------ one call
def frame_terms(B, g_kp, dcam, dx6, dbetas, e_kp, energy2, w_in, w_out):
    """fp32 inputs (None = absent) -> (g [B,157], E [B]) float64: what straps_fit_adam forms per frame"""
    g = torch.zeros(B, NE, dtype=F64) if g_kp is None else g_kp.double().clone()
    for t, (a, b) in ((dcam, (0, 3)), (dx6, (3, 147)), (dbetas, (147, 157))):
        if t is not None:
            g[:, a:b] += t.double()
    E = torch.zeros(B, dtype=F64) if e_kp is None else e_kp.double().reshape(B).clone()
    if energy2 is not None:
        E = E + w_in * energy2.double()[:, 0] + w_out * energy2.double()[:, 1]
    return g, E


def subject_update(est, offsets, mask, g_kp, dcam, dx6, dbetas, e_kp, energy2, w_in, w_out, m, v, sm, sv, step, lr, betas=(0.9, 0.999), eps=1e-8,
                   update=True):
    """one straps_fit_adam_subjects call in float64.  est [B,157], m, v [B,157], sm, sv [G,10] fp32 (taken as exact); offsets [G+1] ints, mask [B] or None.
    -> dict: 'g' [B,157] (the tied gradient: g_s in columns 147.. of every row of a subject), 'E' [B], 'g_s' [G,10], 'E_s' [G], 'abs_g' [G,10] and
    'abs_E' [G] (the sums of the magnitudes of the terms), 'n' [G] (counting frames), and after the update 'est', 'm', 'v', 'sm', 'sv'.
    Rows outside every subject and the shape columns of m / v come back as they went in."""
    B, G = est.shape[0], len(offsets) - 1
    g, E = frame_terms(B, g_kp, dcam, dx6, dbetas, e_kp, energy2, w_in, w_out)
    g_s, E_s, abs_g, abs_E = torch.zeros(G, 10, dtype=F64), torch.zeros(G, dtype=F64), torch.zeros(G, 10, dtype=F64), torch.zeros(G, dtype=F64)
    n = torch.zeros(G, dtype=torch.int64)
    tied = g.clone()
    for s in range(G):
        lo = min(max(int(offsets[s]), 0), B)
        hi = min(max(int(offsets[s + 1]), lo), B)
        rows = counting(lo, hi, mask)
        n[s] = len(rows)
        if rows:
            g_s[s], E_s[s] = g[rows, 147:].sum(dim=0), E[rows].sum()
            abs_g[s], abs_E[s] = g[rows, 147:].abs().sum(dim=0), E[rows].abs().sum()
        tied[lo:hi, 147:] = g_s[s]
    out = {'g': tied, 'E': E, 'g_s': g_s, 'E_s': E_s, 'abs_g': abs_g, 'abs_E': abs_E, 'n': n}
    if not update:
        return out
    lrc = FC.lr_columns(lr)
    e1, m1, v1, sm1, sv1 = est.double().clone(), m.double().clone(), v.double().clone(), sm.double().clone(), sv.double().clone()
    for s in range(G):
        lo = min(max(int(offsets[s]), 0), B)
        hi = min(max(int(offsets[s + 1]), lo), B)
        if lo == hi:
            continue
        a, b, c = FC.adam_update(est[lo:hi, :147].double(), g[lo:hi, :147], m[lo:hi, :147].double(), v[lo:hi, :147].double(), step + 1, lrc[:147], betas, eps)
        e1[lo:hi, :147], m1[lo:hi, :147], v1[lo:hi, :147] = a, b, c
        if int(n[s]):
            a, b, c = FC.adam_update(est[lo, 147:].double(), g_s[s], sm[s].double(), sv[s].double(), step + 1, lrc[147:], betas, eps)
            e1[lo:hi, 147:], sm1[s], sv1[s] = a, b, c
    out.update(est=e1, m=m1, v=v1, sm=sm1, sv=sv1)
    return out


def mean_rows(rows, offsets, mask):
    """straps_subject_mean_rows in float64 -> (mean [G,cols], sum of magnitudes [G,cols], rows used [G])"""
    B, G = rows.shape[0], len(offsets) - 1
    out, mag, n = torch.zeros(G, rows.shape[1], dtype=F64), torch.zeros(G, rows.shape[1], dtype=F64), torch.zeros(G, dtype=torch.int64)
    for s in range(G):
        lo = min(max(int(offsets[s]), 0), B)
        hi = min(max(int(offsets[s + 1]), lo), B)
        use = counting(lo, hi, mask) or list(range(lo, hi))
        n[s] = len(use)
        if use:
            out[s], mag[s] = rows[use].double().mean(dim=0), rows[use].double().abs().sum(dim=0)
    return out, mag, n


# ------------------------------------------------------------------ the cases of the update kernel
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 257)      # frames per subject: B = 464; up to five frames, around one round of the kernel (16 waves x 4 frames in flight = 64), and a clip one past four rounds


def update_case(fps=SIZES, seed=9100, signed=True):
    """-> dict of fp32 tensors for one call on sum(fps) frames: 'est' (all rows of a subject hold one shape), 'g_kp', 'dcam', 'dx6', 'dbetas', 'e_kp' [B,1],
    'energy2' [B,2], 'm', 'v' [B,157], 'sm', 'sv' [G,10], 'offsets' (numpy int32), 'mask' uint8 [B] that knocks out the first frame of subject 2, the last
    frame of subject 4 and (with more than six subjects) the whole of subject 6.
    signed: the shape terms of a (subject, column) share one sign, so that their sum is as large as the sum of their magnitudes and the Adam-step
    comparison is not a comparison of rounding errors (condition (c) of tests/test_subject_fit_cases_cpu.py); the magnitudes are U(0.2, 1)."""
    fps = tuple(fps)
    B, G = sum(fps), len(fps)
    u = lambda shape, k, lo, hi: torch.from_numpy(det_uniform(shape, seed + k, lo, hi))
    off, sub = offsets_of(fps), subject_of(fps)
    est = u((B, NE), 0, -1.0, 1.0)
    est[:, 147:] = u((G, 10), 1, -1.5, 1.5)[sub]
    sign = torch.where(u((G, 10), 2, -1.0, 1.0) < 0, -1.0, 1.0).float()[sub]
    g_kp, dbetas = u((B, NE), 3, -1.0, 1.0), u((B, 10), 4, -1.0, 1.0)
    if signed:
        g_kp[:, 147:] = sign * u((B, 10), 5, 0.1, 0.5)
        dbetas = sign * u((B, 10), 6, 0.1, 0.5)
    mask = torch.ones(B, dtype=torch.uint8)
    if G > 2:
        mask[off[2]] = 0
    if G > 4:
        mask[off[5] - 1] = 0
    if G > 6:
        mask[off[6]:off[7]] = 0
    return {'est': est, 'g_kp': g_kp, 'dcam': u((B, 3), 7, -1.0, 1.0), 'dx6': u((B, 144), 8, -1.0, 1.0), 'dbetas': dbetas,
            'e_kp': u((B, 1), 9, 0.1, 1.0), 'energy2': u((B, 2), 10, 0.0, 0.01), 'm': u((B, NE), 11, -0.1, 0.1), 'v': u((B, NE), 12, 0.0, 0.01),
            'sm': u((G, 10), 13, -0.1, 0.1), 'sv': u((G, 10), 14, 0.0, 0.01), 'offsets': off, 'mask': mask, 'fps': fps}


def rounding_bound(n, mag):
    """the bar of an fp32 sum of n terms against the exact sum of the same terms: n * 2^-23 * sum |terms|"""
    return n.double().reshape(-1, *([1] * (mag.dim() - 1))) * EPS32 * mag


# ------------------------------------------------------------------ the tied fit
def subject_adam_fit(est, fps, energy_fn, iters, lr=(0.01, 0.01, 0.01), betas=(0.9, 0.999), eps=1e-8, mask=None):
    """torch.optim.Adam on (cam [B,3], x6 [B,144], beta [G,10]): the shape of a frame is its subject's parameter, which starts at the mean of the subject's
    counting rows of `est`.  energy_fn(est [B,157] float64) -> (E [B], terms or None).
    -> (trajectory [iters+1,B,157], subject energies [G,iters+1], frame energies [B,iters+1], terms of the last evaluation)"""
    off, sub = offsets_of(fps), subject_of(fps)
    w = torch.ones(est.shape[0], dtype=F64) if mask is None else (torch.as_tensor(mask) != 0).double()
    start, _, _ = mean_rows(est[:, 147:], off, mask)
    cam, x6 = (est[:, a:b].clone().requires_grad_(True) for a, b in ((0, 3), (3, 147)))
    beta = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([{'params': [cam], 'lr': lr[0]}, {'params': [x6], 'lr': lr[1]}, {'params': [beta], 'lr': lr[2]}], betas=betas, eps=eps)
    traj, sub_e, frame_e, terms = [], [], [], None
    for i in range(iters + 1):
        opt.zero_grad()
        full = torch.cat([cam, x6, beta[sub]], dim=1)
        E, terms = energy_fn(full)
        traj.append(full.detach().clone())
        frame_e.append(E.detach().clone())
        sub_e.append(torch.zeros(len(fps), dtype=F64).index_add_(0, sub, (E * w).detach()))
        if i == iters:
            break
        # cam and pose of a masked frame still see their own frame's energy; the shape sees the counting frames alone
        if mask is None:
            E.sum().backward()
        else:
            gc, gx = torch.autograd.grad(E.sum(), (cam, x6), retain_graph=True)
            gb, = torch.autograd.grad((E * w).sum(), beta)
            cam.grad, x6.grad, beta.grad = gc, gx, gb
        opt.step()
    return torch.stack(traj), torch.stack(sub_e, dim=1), torch.stack(frame_e, dim=1), (None if terms is None else terms.detach())


def tied_gradient(est, fps, energy_fn):
    """autograd of the summed energy w.r.t. per-frame cam / pose and ONE shared shape variable per subject (est's rows of a subject must hold one shape)
    -> (E [B], g [B,157] with the shared variable's gradient in columns 147.. of every row of the subject)"""
    off, sub = offsets_of(fps), subject_of(fps)
    head = est[:, :147].clone().requires_grad_(True)
    beta = est[off[:-1].astype(np.int64), 147:].clone().requires_grad_(True)
    E, _ = energy_fn(torch.cat([head, beta[sub]], dim=1))
    gh, gb = torch.autograd.grad(E.sum(), (head, beta))
    return E.detach(), torch.cat([gh, gb[sub]], dim=1)


KP_FPS = (3, 3)      # fit_cases.standard_case(B=6) read as two subjects
_FITS = {}


def keypoint_energy_fn(case, est0, **kw):
    tg, cf = case['targets'].double(), case['conf'].double()
    return lambda est: (FC.energy(est, est0, tg, cf, **kw)[0], None)


def keypoint_reference():
    """the float64 tied fit of the standard keypoint case, 100 iterations, once per process -> (case, trajectory, subject energies, frame energies)"""
    if 'kp' not in _FITS:
        case = FC.standard_case()
        est = case['est'].double()
        traj, sub_e, frame_e, _ = subject_adam_fit(est, KP_FPS, keypoint_energy_fn(case, est.clone()), 100)
        _FITS['kp'] = (case, traj, sub_e, frame_e)
    return _FITS['kp']


T = SC.TRAJ
SIL_STREAM, SIL_FRAMES = 24, 4


def silhouette_subject_case(stream=SIL_STREAM, frames=SIL_FRAMES):
    """one subject seen in `frames` frames, rendered once per process: every frame starts at the mean parameters under cam (0.9, 0, 0); the true body has
    ONE shape (the mean moved by the N(0, 1) draw of silfit_cases' stream) and per frame the mean 6-D pose moved by 0.1 N(0, 1); targets =
    eval_cases.wp_silhouette of the true bodies at 64 x 64.  -> dict as silfit_cases.trajectory_case, and 'fps'"""
    key = ('sil', stream, frames)
    if key not in _FITS:
        mp = synthetic_mean_params(0)
        start = np.concatenate([[0.9, 0.0, 0.0], mp['pose'].astype(np.float64), mp['shape'].astype(np.float64)])
        true = np.tile(start, (frames, 1))
        true[:, 147:] += SC.det_normal((10,), 7200 + 10 * stream)[None]
        for k in range(frames):
            true[k, 3:147] += 0.1 * SC.det_normal((144,), 7100 + 10 * stream + 1 + k)
        start, true = np.tile(start, (frames, 1)).astype(np.float32), true.astype(np.float32)
        with torch.no_grad():
            v = SC.mesh(torch.from_numpy(true).double()).float().numpy()
        masks = EC.wp_silhouette(v, SC.MODEL['faces'], true[:, :3], T['wh'])
        _FITS[key] = {'est': torch.from_numpy(start), 'true': torch.from_numpy(true), 'masks': masks, 'd2': np.stack([SC.two_pass_d2(m) for m in masks]),
                      'fps': (frames,)}
    return _FITS[key]


def silhouette_energy_fn(c, est0):
    kw = dict(lambda_pose=T['lambda_pose'], lambda_shape=T['lambda_shape'])
    return lambda est: SC.objective(est, est0, c['masks'], c['d2'], None, None, T['lattice'], T['tau'], T['w_in'], T['w_out'], **kw)


def silhouette_reference():
    """the float64 tied fit of silhouette_subject_case at silfit_cases.TRAJ's settings -> (terms at the start [B,3], terms at the end [B,3]); once per process"""
    if 'sil_fit' not in _FITS:
        c = silhouette_subject_case()
        est = c['est'].double()
        fn = silhouette_energy_fn(c, est.clone())
        with torch.no_grad():
            _, t0 = fn(est)
        _, _, _, t1 = subject_adam_fit(est, c['fps'], fn, T['iters'], lr=T['lr'])
        _FITS['sil_fit'] = (t0, t1)
    return _FITS['sil_fit']
