"""Test helper: the float64 reference of straps_fit_keypoints and its cases (tests/test_fit_cases_cpu.py, tests/test_gpu_fit_keypoints.py).

The objective of include/straps_hip.h restated in float64 torch on the oracle alone -- `O.rot6d_to_rotmat`, `O.smpl_forward(MODEL, ...,
dtype=float64)` (the FULL mesh: a tracked vertex is a row of its vertices), `O.orthographic_project` -- with autograd for the gradient and
`torch.optim.Adam` with three parameter groups for the fit.  All inputs come from `detgen.det_uniform`.
"""
import numpy as np
import torch

import straps_oracle as O
from detgen import det_uniform
from straps_amd.synthetic_smpl import synthetic_smpl_model

MODEL = synthetic_smpl_model(0)
COCO = list(O.ALL_JOINTS_TO_COCO_MAP)
IMG_WH = 256.0
NE = 157
F64 = torch.float64


def keypoints3d(est, spec, model=MODEL):
    """est [B,157] float64 -> [B,K,3]: rows of the 90-joint output, or ('vertex', id) rows of the mesh"""
    B = est.shape[0]
    R = O.rot6d_to_rotmat(est[:, 3:147].reshape(-1, 6)).view(B, 24, 3, 3)
    verts, joints = O.smpl_forward(model, est[:, 147:], rotmats=R, dtype=F64)
    cols = [verts[:, int(k[1])] if isinstance(k, (tuple, list)) else joints[:, int(k)] for k in spec]
    return torch.stack(cols, dim=1)


def weights(targets, conf):
    """-> (w [B,K], targets with the unused ones replaced by 0)"""
    ok = torch.isfinite(targets).all(dim=2)
    if conf is not None:
        ok = ok & torch.isfinite(conf) & (conf > 0)
    c = torch.ones_like(targets[:, :, 0]) if conf is None else conf
    w = torch.where(ok, c * c, torch.zeros_like(c))
    return w, torch.where(ok[:, :, None], targets, torch.zeros_like(targets))


def energy(est, est0, targets, conf, spec=COCO, sigma=0.0, lambda_pose=1e-3, lambda_shape=1e-3, img_wh=IMG_WH, model=MODEL):
    """all float64 -> (E [B], kp2d [B,K,2] normalised)"""
    w, t = weights(targets, conf)
    p = O.orthographic_project(keypoints3d(est, spec, model), est[:, :3])
    that = 2.0 * t / img_wh - 1.0
    r2 = ((p - that) ** 2).sum(dim=2)
    r2 = torch.where(w > 0, r2, torch.zeros_like(r2))
    rho = sigma * sigma * r2 / (sigma * sigma + r2) if sigma > 0 else r2
    E = (w * rho).sum(dim=1) + lambda_pose * ((est[:, 3:147] - est0[:, 3:147]) ** 2).sum(dim=1) \
        + lambda_shape * ((est[:, 147:] - est0[:, 147:]) ** 2).sum(dim=1)
    return E, p


def energy_grad(est, est0, targets, conf, **kw):
    """-> (E [B], g [B,157], kp2d) by autograd (bodies are independent: the gradient of the sum is every body's own)"""
    x = est.clone().requires_grad_(True)
    E, p = energy(x, est0, targets, conf, **kw)
    g, = torch.autograd.grad(E.sum(), x)
    return E.detach(), g, p.detach()


def adam_fit(est, est0, targets, conf, iters, lr=(0.01, 0.01, 0.01), betas=(0.9, 0.999), eps=1e-8, **kw):
    """torch.optim.Adam, parameter groups (cam, x6, beta) -> (trajectory [iters+1,B,157], energies [B,iters+1])"""
    cam, x6, beta = (est[:, a:b].clone().requires_grad_(True) for a, b in ((0, 3), (3, 147), (147, 157)))
    opt = torch.optim.Adam([{'params': [cam], 'lr': lr[0]}, {'params': [x6], 'lr': lr[1]}, {'params': [beta], 'lr': lr[2]}], betas=betas, eps=eps)
    traj, en = [], []
    for i in range(iters + 1):
        opt.zero_grad()
        E, _ = energy(torch.cat([cam, x6, beta], dim=1), est0, targets, conf, **kw)
        traj.append(torch.cat([cam, x6, beta], dim=1).detach().clone())
        en.append(E.detach().clone())
        if i == iters:
            break
        E.sum().backward()
        opt.step()
    return torch.stack(traj), torch.stack(en, dim=1)


def adam_update(est, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """one step of the update formula of straps_adam_step in float64: -> (est', m', v'); lr [157] per column"""
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    return est - lr / (1 - betas[0] ** t) * m / (v.sqrt() / (1 - betas[1] ** t) ** 0.5 + eps), m, v


def lr_columns(lr):
    return torch.tensor([lr[0]] * 3 + [lr[1]] * 144 + [lr[2]] * 10, dtype=F64)


def _x6(aa):
    """axis-angle [B,72] float64 -> 6-D pose [B,144]: the first two columns of every rotation, interleaved"""
    R = O.batch_rodrigues(aa.reshape(-1, 3)).view(-1, 24, 3, 3)
    return R[:, :, :, :2].reshape(aa.shape[0], 144)


def standard_case(B=6, seed=4100, spec=COCO, zero_body=4, zero_kp=(0, 3)):
    """-> dict of float32 tensors: 'est' (the perturbed start) [B,157], 'true' [B,157], 'targets' [B,K,2] px, 'conf' [B,K].
    True pose axis-angle U(-0.4, 0.4), betas U(-1.5, 1.5), cam [0.9, 0, 0] +- 0.1; targets = the true bodies' projections in pixels; start:
    pose + U(-0.25, 0.25) rad, betas +- 1, cam +- 0.05; conf U(0.3, 1) with one single zero and (B > zero_body) one body all zero."""
    u = lambda shape, k, lo, hi: torch.from_numpy(det_uniform(shape, seed + k, lo, hi).astype(np.float64))
    aa, betas = u((B, 72), 1, -0.4, 0.4), u((B, 10), 2, -1.5, 1.5)
    cam = torch.tensor([0.9, 0.0, 0.0], dtype=F64) + u((B, 3), 3, -0.1, 0.1)
    true = torch.cat([cam, _x6(aa), betas], dim=1).float()
    start = torch.cat([cam + u((B, 3), 4, -0.05, 0.05), _x6(aa + u((B, 72), 5, -0.25, 0.25)), betas + u((B, 10), 6, -1.0, 1.0)], dim=1).float()
    with torch.no_grad():
        p = O.orthographic_project(keypoints3d(true.double(), spec), true.double()[:, :3])
    targets = ((p + 1.0) * (IMG_WH / 2.0)).float()
    conf = u((B, len(spec)), 7, 0.3, 1.0).float()
    conf[zero_kp[0] % B, zero_kp[1] % len(spec)] = 0.0
    if B > zero_body:
        conf[zero_body] = 0.0
    return {'est': start, 'true': true, 'targets': targets, 'conf': conf}


_FITS = {}


def reference_fit(name):
    """the float64 fits the tests share, computed once per process: 'sigma0' / 'sigma01' (the standard case, 100 iterations) and
    'nonmonotone' (lr 0.02, lambda_pose 1e-2, sigma 0.1) -> (case, trajectory [101,B,157], energies [B,101], keyword arguments)"""
    if name not in _FITS:
        kw = {'sigma0': dict(sigma=0.0), 'sigma01': dict(sigma=0.1), 'nonmonotone': dict(sigma=0.1, lambda_pose=1e-2)}[name]
        lr = (0.02,) * 3 if name == 'nonmonotone' else (0.01,) * 3
        case = standard_case()
        est = case['est'].double()
        traj, en = adam_fit(est, est.clone(), case['targets'].double(), case['conf'].double(), 100, lr=lr, **kw)
        _FITS[name] = (case, traj, en, dict(kw, lr=lr))
    return _FITS[name]
