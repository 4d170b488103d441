"""Test helper: the fused loss head (straps_loss_fwd_bwd / _gm) against the oracle's multi_task_loss composed with float64 autograd --
the composition of test_fused_loss_vs_oracle, shared with tests/test_gpu_loss_head_edges.py -- and a launcher whose outputs and
workspace are guarded (tests/redzone.py).
"""
import ctypes as C

import numpy as np
import torch

import straps_oracle as O
from detgen import det_uniform

ORDER = ('verts', 'joints2D', 'joints3D', 'shape_params', 'pose_params')
INIT_WEIGHTS = {'verts': 1.0, 'joints2D': 0.1, 'pose_params': 0.1, 'shape_params': 0.1, 'joints3D': 1.0}
IMG_WH = 256


def oracle_loss(joints, est, prot, pverts, tverts, tj2d, tj3d, tshape, trot, lv0, dtype=torch.float64, j2d_count=None, grad_verts=True,
                grad_rot=True):
    """heads (orthographic projection of the 17 COCO joints, the 14 H36M-LSP joints, shape = est[:, 147:157]) + O.multi_task_loss,
    backward done.  lv0: {task: float}.  -> (total, parts, lab, leaves {'J', 'E', 'PR', 'PV'}, log-variance leaves {task: tensor})"""
    c = lambda t: t.to(dtype)
    J, E = c(joints).requires_grad_(), c(est).requires_grad_()
    PR, PV = c(prot), c(pverts)
    if grad_rot:
        PR.requires_grad_()
    if grad_verts:
        PV.requires_grad_()
    lv = {k: torch.tensor(lv0[k], dtype=dtype, requires_grad=True) for k in ORDER}
    outp = {'verts': PV, 'joints2D': O.orthographic_project(J[:, O.ALL_JOINTS_TO_COCO_MAP], E[:, :3]),
            'joints3D': J[:, O.ALL_JOINTS_TO_H36M_MAP][:, O.H36M_TO_J14], 'shape_params': E[:, 147:157], 'pose_params_rot_matrices': PR}
    lab = {'verts': c(tverts), 'joints2D': c(tj2d), 'joints3D': c(tj3d), 'shape_params': c(tshape),
           'pose_params_rot_matrices': c(trot), 'vis': O.check_joints2d_visibility(tj2d)}
    total, parts = O.multi_task_loss(lab, outp, lv, j2d_count=j2d_count)
    total.backward()
    return total, parts, lab, {'J': J, 'E': E, 'PR': PR, 'PV': PV}, lv


def make_inputs(B, ld_est=160, seed=60, random_log_vars=True, j2d_range=(-40.0, 300.0)):
    """CPU fp32 inputs of one call.  est [B, ld_est]: 157 used columns, the padding columns hold 7.0 (never read by the reference)"""
    est = torch.full((B, ld_est), 7.0)
    est[:, :157] = torch.from_numpy(det_uniform((B, 157), seed + 1, -1, 1))[:, :ld_est]
    est[:, 0] = est[:, 0].abs() + 0.5
    lv0 = O.init_log_vars(INIT_WEIGHTS)
    if random_log_vars:
        lv0 = {k: float(v) for k, v in zip(ORDER, det_uniform((5,), seed + 9, -2.0, 2.0))}
    return dict(joints=torch.from_numpy(det_uniform((B, 90, 3), seed, -1, 1)), est=est,
                prot=torch.from_numpy(det_uniform((B, 24, 3, 3), seed + 2)), pverts=torch.from_numpy(det_uniform((B, 6890, 3), seed + 3)),
                tverts=torch.from_numpy(det_uniform((B, 6890, 3), seed + 4)), tj2d=torch.from_numpy(det_uniform((B, 17, 2), seed + 5, *j2d_range)),
                tj3d=torch.from_numpy(det_uniform((B, 14, 3), seed + 6)), tshape=torch.from_numpy(det_uniform((B, 10), seed + 7, -2, 2)),
                trot=torch.from_numpy(det_uniform((B, 24, 3, 3), seed + 8)), lv0=lv0)


def reference(x, j2d_count=None):
    """float64 oracle of make_inputs() -> dict of float64 CPU tensors (loss [12] laid out as the kernel's loss_out; NaN where the oracle's is)"""
    total, parts, lab, leaf, lv = oracle_loss(x['joints'], x['est'][:, :157], x['prot'], x['pverts'], x['tverts'], x['tj2d'], x['tj3d'],
                                               x['tshape'], x['trot'], x['lv0'], j2d_count=j2d_count)
    loss = torch.full((12,), float('nan'), dtype=torch.float64)
    loss[0] = total.detach()
    for i, k in enumerate(ORDER):
        loss[1 + i] = parts[k].detach()
        loss[6 + i] = parts[k].detach() * torch.exp(lv[k].detach())
    loss[11] = float(lab['vis'].sum())
    return dict(loss=loss, dlogvar=torch.stack([lv[k].grad for k in ORDER]), dverts=leaf['PV'].grad, djoints=leaf['J'].grad,
                dest=leaf['E'].grad, drot=leaf['PR'].grad, vis=lab['vis'])


def count_visible(dev, tj2d, zone):
    """straps_count_visible on a [B,nj,2] CPU tensor -> float"""
    from straps_amd import hipabi
    out = zone.guarded((1,), name='count')
    t = zone.at_end(tj2d)
    rc = hipabi.lib().straps_count_visible(hipabi.ptr(t), hipabi.ptr(out), tj2d.shape[0], tj2d.shape[1], IMG_WH, None)
    hipabi.check(rc, 'straps_count_visible')
    zone.check()
    return float(out)


def run_kernel(dev, zone, x, grads=True, count=None, count_scale=1.0, outputs=None, expect_rc=0):
    """one call of straps_loss_fwd_bwd (count None) / straps_loss_fwd_bwd_gm through the C ABI: inputs at the end of poison, outputs and the
    workspace (exactly the advertised size) guarded.  outputs: names of the gradient outputs to pass (default: all when `grads`).
    -> dict of CPU tensors (the whole dest [B, ld_est]); with expect_rc != 0 asserts the refusal and that nothing was written."""
    from straps_amd import hipabi
    L = hipabi.lib()
    B, ld = x['est'].shape
    names = ('dverts', 'djoints', 'dest', 'drot', 'dlogvar')
    outputs = (names if grads else ()) if outputs is None else outputs
    shapes = {'dverts': (B, 6890, 3), 'djoints': (B, 90, 3), 'dest': (B, ld), 'drot': (B, 24, 3, 3), 'dlogvar': (5,)}
    out = {n: (zone.guarded(shapes[n], name=n, margin=(128 << 10) if n == 'dverts' else (64 << 10)) if n in outputs else None) for n in names}
    loss = zone.guarded((12,), name='loss')
    ws = zone.guarded((L.straps_loss_workspace_bytes(B) // 4,), name='workspace')
    t = {k: zone.at_end(x[k]) for k in ('pverts', 'joints', 'est', 'prot', 'tverts', 'tj2d', 'tj3d', 'tshape', 'trot')}
    lvd = zone.at_end(torch.tensor([x['lv0'][k] for k in ORDER], dtype=torch.float32))
    p = hipabi.ptr
    args = [p(t['pverts']), p(t['joints']), p(t['est']), ld, p(t['prot']), p(t['tverts']), p(t['tj2d']), p(t['tj3d']), p(t['tshape']), p(t['trot']),
            p(lvd), p(loss), p(out['dverts']), p(out['djoints']), p(out['dest']), p(out['drot']), p(out['dlogvar']), p(ws), B, IMG_WH]
    if count is None:
        rc = L.straps_loss_fwd_bwd(*args, None)
    else:
        cd = zone.at_end(torch.tensor([count], dtype=torch.float32))
        rc = L.straps_loss_fwd_bwd_gm(*args, p(cd), C.c_float(count_scale), None)
    assert rc == expect_rc, 'return code %d, expected %d: %s' % (rc, expect_rc, L.straps_last_error().decode())
    zone.check()
    res = {n: (None if v is None else v.cpu()) for n, v in out.items()}
    res['loss'] = loss.cpu()
    if expect_rc != 0:
        for n, v in res.items():
            assert v is None or bool(torch.isnan(v).all()), 'a refused call wrote to %s' % n
    return res


def assert_close_nan(name, got, ref, rtol):
    """element-wise: NaN exactly where the reference is NaN, |got - ref| <= rtol |ref| elsewhere"""
    g, r = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(g), np.isnan(r)), '%s: NaN pattern %s, the oracle\'s %s' % (name, np.isnan(g), np.isnan(r))
    ok = ~np.isnan(r)
    np.testing.assert_allclose(g[ok], r[ok], rtol=rtol, atol=0, err_msg=name)
