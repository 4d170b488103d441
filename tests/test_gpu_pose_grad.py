"""GPU: axis-angle gradients -- straps_rodrigues_bwd, the differentiable batch_rodrigues, and SMPL(pose2rot=True) gradients through
straps_smpl_bwd_aa (the Rodrigues derivative fused into the pose pass of the SMPL gradient) -- against float64 autograd of the oracle.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import straps_amd
import straps_oracle as O
from detgen import det_uniform
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
MODEL = straps_amd.synthetic_smpl_model(0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    hipabi.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def smpl(dev):
    return straps_amd.SMPL(MODEL, batch_size=1).to(dev)


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rodrigues_bwd(aa, dR):
    daa = torch.empty_like(aa)
    hipabi.check(hipabi.lib().straps_rodrigues_bwd(hipabi.ptr(aa), hipabi.ptr(dR), hipabi.ptr(daa), aa.shape[0], hipabi.stream_ptr()),
                 'straps_rodrigues_bwd')
    return daa


def _test_rows():
    """axis-angle rows: exact zeros, +-1e-7, 1e-5, 1e-3, moderate angles, within 1e-3 of pi, 3 pi, mixed signs."""
    axes = det_uniform((16, 3), 500, -1.0, 1.0).astype(np.float64)
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    angles = [1e-7, -1e-7, 1e-5, -1e-5, 1e-3, 0.3, 1.0, -2.0, math.pi - 1e-3, math.pi - 2e-4, math.pi + 5e-4, -(math.pi - 7e-4),
              3 * math.pi, -3 * math.pi, 2.5, 0.05]
    rows = [[0.0, 0.0, 0.0]] * 4
    rows += [list(a * axes[i % 16]) for i, a in enumerate(angles)]
    rows += [[1e-7, 0.0, 0.0], [0.0, -1e-7, 0.0], [1e-7, -1e-7, 1e-7], [1e-3, -1e-3, 0.0], [0.0, 0.0, math.pi - 5e-4]]
    mixed = det_uniform((40, 3), 501, -3.0, 3.0).astype(np.float64)
    rows += mixed.tolist()
    return torch.tensor(rows, dtype=torch.float32), 4          # (rows, number of leading zero rows)


def test_rodrigues_bwd_vs_float64_autograd(dev):
    aa, nz = _test_rows()
    n = aa.shape[0]
    dR = torch.from_numpy(det_uniform((n, 3, 3), 502, -1.0, 1.0))
    x = aa.double().requires_grad_()
    O.batch_rodrigues(x).backward(dR.double())
    ref = x.grad
    got = _rodrigues_bwd(aa.to(dev), dR.to(dev)).cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert float(err.max()) <= 1e-5 * float(ref.abs().max()), 'max err %.3e vs max |ref| %.3e' % (float(err.max()), float(ref.abs().max()))
    # the zero rows on their own: finite and equal to autograd of the formula there (theta = sqrt(3) 1e-8)
    assert float(err[:nz].max()) <= 1e-5 * float(ref[:nz].abs().max())
    assert float(ref[:nz].abs().max()) > 0.1


def test_batch_rodrigues_is_differentiable(dev):
    aa, _ = _test_rows()
    n = aa.shape[0]
    dR = torch.from_numpy(det_uniform((n, 3, 3), 503, -1.0, 1.0)).to(dev)
    a = aa.to(dev).requires_grad_()
    R = straps_amd.batch_rodrigues(a)
    with torch.no_grad():
        R0 = straps_amd.batch_rodrigues(aa.to(dev))
    assert torch.equal(R.detach(), R0)
    R.backward(dR)
    assert torch.equal(a.grad, _rodrigues_bwd(aa.to(dev), dR))
    # a non-contiguous [..., 3] view: the gradient lands in the viewed columns of the base tensor only
    B = 5
    base = torch.from_numpy(det_uniform((B, 80), 504, -1.5, 1.5)).to(dev).requires_grad_()
    v = base[:, 3:75].view(B, 24, 3)
    assert not v.is_contiguous()
    R = straps_amd.batch_rodrigues(v)
    assert R.shape == (B * 24, 3, 3)
    dR = torch.from_numpy(det_uniform((B * 24, 3, 3), 505, -1.0, 1.0)).to(dev)
    R.backward(dR)
    want = _rodrigues_bwd(base.detach()[:, 3:75].contiguous().view(-1, 3), dR).view(B, 72)
    assert torch.equal(base.grad[:, 3:75], want)
    assert not base.grad[:, :3].any() and not base.grad[:, 75:].any()


def _oracle_grads(betas, aa, gv, gj, go_shape=None):
    """float64 autograd of the oracle's pose2rot=True SMPL for the three upstream-gradient kinds: {kind: (dbetas, dglobal_orient, dbody_pose)}."""
    B = betas.shape[0]
    b = betas.double().requires_grad_()
    go = (aa[:1, :3] if go_shape == 1 else aa[:, :3]).double().requires_grad_()
    bp = aa[:, 3:].double().requires_grad_()
    v, j = O.smpl_forward(MODEL, b, full_pose_aa=torch.cat([go.expand(B, 3), bp], 1), dtype=torch.float64)
    out = {}
    for kind, loss in (('both', (v * gv.double()).sum() + (j * gj.double()).sum()), ('verts', (v * gv.double()).sum()),
                       ('joints', (j * gj.double()).sum())):
        out[kind] = torch.autograd.grad(loss, (b, go, bp), retain_graph=True)
    return out


@pytest.mark.parametrize('B', [3, 37, 1100])
def test_smpl_pose2rot_gradients_vs_oracle(dev, smpl, B):
    betas = torch.from_numpy(det_uniform((B, 10), 510 + B, -2, 2))
    aa = torch.from_numpy(det_uniform((B, 72), 511 + B, -0.8, 0.8))
    gv = torch.from_numpy(det_uniform((B, 6890, 3), 512, -1, 1))
    gj = torch.from_numpy(det_uniform((B, 90, 3), 513, -1, 1))
    ref = _oracle_grads(betas, aa, gv, gj)
    b, go, bp = betas.to(dev).requires_grad_(), aa[:, :3].to(dev).requires_grad_(), aa[:, 3:].to(dev).requires_grad_()
    out = smpl(betas=b, global_orient=go, body_pose=bp)          # pose2rot=True (the default)
    assert out.full_pose.requires_grad
    gvd, gjd = gv.to(dev), gj.to(dev)
    for kind, loss in (('both', (out.vertices * gvd).sum() + (out.joints * gjd).sum()), ('verts', (out.vertices * gvd).sum()),
                       ('joints', (out.joints * gjd).sum())):
        got = torch.autograd.grad(loss, (b, go, bp), retain_graph=True)
        for name, g, r in zip(('dbetas', 'dglobal_orient', 'dbody_pose'), got, ref[kind]):
            assert g is not None and torch.isfinite(g).all(), '%s %s B=%d' % (kind, name, B)
            assert _relerr(g, r) < 1e-4, '%s %s B=%d: rel err %.3e' % (kind, name, B, _relerr(g, r))


def _smpl_bwd_aa(smpl, b, r, aa, dv, dj, want_drot):
    L = hipabi.lib()
    B = b.shape[0]
    dbetas, daa = torch.empty_like(b), torch.empty_like(aa)
    drot = torch.empty_like(r) if want_drot else None
    ws = torch.empty(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4, device=b.device, dtype=torch.float32)
    hipabi.check(L.straps_smpl_bwd_aa(C.byref(smpl._model_struct()), hipabi.ptr(b), hipabi.ptr(r), hipabi.ptr(aa), hipabi.ptr(dv), hipabi.ptr(dj),
                                      hipabi.ptr(dbetas), hipabi.ptr(daa), hipabi.ptr(drot), hipabi.ptr(ws), B, 0, hipabi.stream_ptr()),
                 'straps_smpl_bwd_aa')
    return dbetas, daa, drot


@pytest.mark.parametrize('B', [37, 1100, 4096])
def test_fused_equals_composed(dev, smpl, B):
    """straps_smpl_bwd_aa == straps_smpl_bwd followed by straps_rodrigues_bwd, bit for bit (one shared device function), and its dbetas /
    drotmats == straps_smpl_bwd's."""
    L = hipabi.lib()
    b = torch.from_numpy(det_uniform((B, 10), 520, -2, 2)).to(dev)
    aa = torch.from_numpy(det_uniform((B, 72), 521, -2.0, 2.0))
    aa[1, 6:9] = 0.0                                                  # a zero axis-angle row
    aa = aa.to(dev)
    r = straps_amd.batch_rodrigues(aa.view(-1, 3)).view(B, 24, 3, 3)
    dv = torch.from_numpy(det_uniform((B, 6890, 3), 522, -1, 1)).to(dev)
    dj = torch.from_numpy(det_uniform((B, 90, 3), 523, -1, 1)).to(dev)
    dbetas0, drot0 = torch.empty_like(b), torch.empty_like(r)
    ws = torch.empty(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4, device=dev, dtype=torch.float32)
    hipabi.check(L.straps_smpl_bwd(C.byref(smpl._model_struct()), hipabi.ptr(b), hipabi.ptr(r), hipabi.ptr(dv), hipabi.ptr(dj), hipabi.ptr(dbetas0),
                                   hipabi.ptr(drot0), hipabi.ptr(ws), B, 0, hipabi.stream_ptr()), 'straps_smpl_bwd')
    daa0 = _rodrigues_bwd(aa.view(-1, 3), drot0.view(-1, 9)).view(B, 72)
    dbetas1, daa1, drot1 = _smpl_bwd_aa(smpl, b, r, aa, dv, dj, want_drot=True)
    dbetas2, daa2, _ = _smpl_bwd_aa(smpl, b, r, aa, dv, dj, want_drot=False)
    assert torch.isfinite(daa0).all()
    assert torch.equal(daa1, daa0) and torch.equal(daa2, daa0)
    assert torch.equal(dbetas1, dbetas0) and torch.equal(dbetas2, dbetas0)
    assert torch.equal(drot1, drot0)


def test_pose2rot_forward_unchanged(dev, smpl):
    B = 6
    betas = torch.from_numpy(det_uniform((B, 10), 530, -2, 2)).to(dev)
    aa = torch.from_numpy(det_uniform((B, 72), 531, -1.0, 1.0)).to(dev)
    b, go, bp = betas.clone().requires_grad_(), aa[:, :3].clone().requires_grad_(), aa[:, 3:].clone().requires_grad_()
    out = smpl(betas=b, global_orient=go, body_pose=bp)
    assert out.vertices.requires_grad
    with torch.no_grad():
        ng = smpl(betas=betas, global_orient=aa[:, :3], body_pose=aa[:, 3:])
        R = straps_amd.batch_rodrigues(aa.reshape(-1, 3)).view(B, 24, 3, 3)
        rm = smpl(betas=betas, global_orient=R[:, :1], body_pose=R[:, 1:], pose2rot=False)
    for o in (ng, rm):
        assert torch.equal(out.vertices.detach(), o.vertices) and torch.equal(out.joints.detach(), o.joints)
    assert torch.equal(out.full_pose.detach(), aa)


def test_broadcast_and_module_parameters(dev):
    B = 4
    betas = torch.from_numpy(det_uniform((B, 10), 540, -2, 2))
    aa = torch.from_numpy(det_uniform((B, 72), 541, -0.8, 0.8))
    gv = torch.from_numpy(det_uniform((B, 6890, 3), 542, -1, 1))
    gj = torch.from_numpy(det_uniform((B, 90, 3), 543, -1, 1))
    smpl = straps_amd.SMPL(MODEL, batch_size=B).to(dev)
    # global_orient [1,3] broadcast over body_pose [B,69]: the batch-summed gradient
    ref = _oracle_grads(betas, aa, gv, gj, go_shape=1)['both']
    go, bp = aa[:1, :3].to(dev).requires_grad_(), aa[:, 3:].to(dev).requires_grad_()
    out = smpl(betas=betas.to(dev), global_orient=go, body_pose=bp)
    ((out.vertices * gv.to(dev)).sum() + (out.joints * gj.to(dev)).sum()).backward()
    assert go.grad.shape == (1, 3)
    assert _relerr(go.grad, ref[1]) < 1e-4 and _relerr(bp.grad, ref[2]) < 1e-4
    # smpl(betas=b) with the module's own body_pose / global_orient Parameters (as smplx users do)
    ref = _oracle_grads(betas, aa, gv, gj)['both']
    with torch.no_grad():
        smpl.global_orient.copy_(aa[:, :3])
        smpl.body_pose.copy_(aa[:, 3:])
    smpl.zero_grad(set_to_none=True)
    out = smpl(betas=betas.to(dev))
    ((out.vertices * gv.to(dev)).sum() + (out.joints * gj.to(dev)).sum()).backward()
    assert smpl.global_orient.grad is not None and smpl.body_pose.grad is not None
    assert _relerr(smpl.global_orient.grad, ref[1]) < 1e-4 and _relerr(smpl.body_pose.grad, ref[2]) < 1e-4


def test_fitting_loop_converges(dev):
    """30 Adam steps on the module's body_pose / global_orient / betas toward the joints of a fixed target body."""
    B = 2
    smpl = straps_amd.SMPL(MODEL, batch_size=B).to(dev)
    tp = torch.from_numpy(det_uniform((B, 72), 700, -0.5, 0.5)).to(dev)
    tb = torch.from_numpy(det_uniform((B, 10), 701, -1, 1)).to(dev)
    with torch.no_grad():
        target = smpl(betas=tb, global_orient=tp[:, :3], body_pose=tp[:, 3:]).joints
    opt = torch.optim.Adam([smpl.body_pose, smpl.global_orient, smpl.betas], lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = ((smpl().joints - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    with torch.no_grad():
        final = float(((smpl().joints - target) ** 2).mean())
    assert all(math.isfinite(v) for v in losses) and math.isfinite(final)
    for p in (smpl.body_pose, smpl.global_orient, smpl.betas):
        assert torch.isfinite(p).all()
    assert final < 0.2 * losses[0], 'joint MSE %.4e -> %.4e' % (losses[0], final)


def test_axis_angle_pose_must_be_fp32(dev, smpl):
    """the grad path refuses a float64 pose as batch_rodrigues does (no silent conversion), before any launch."""
    B = 2
    bp = torch.zeros(B, 69, dtype=torch.float64, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match='dtype'):
        smpl(betas=torch.zeros(B, 10, device=dev), body_pose=bp, global_orient=torch.zeros(B, 3, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match='dtype'):
        straps_amd.batch_rodrigues(torch.zeros(4, 3, dtype=torch.float64, device=dev, requires_grad=True))
