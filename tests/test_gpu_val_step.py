"""GPU: validation.ValStep -- one validation batch of the reference's loop (train/train_synthetic_otf_rendering.py:251-348) on the device:
every stage against the oracle through `keep` (the bars of tests/test_gpu_datagen.py for the same stages of make_batch), the eval-mode
forward and the head bit for bit against direct calls, and the guarantee that a validation step moves nothing a training step owns."""
import numpy as np
import pytest
import torch

import straps_amd
import straps_oracle as O
from detgen import det_uniform
from straps_amd import hipabi
from straps_amd.metrics import BatchMetrics
from straps_amd.validation import PER_SAMPLE, ValStep
from test_gpu_datagen import DEV, LOSSES, MP, W, _step

pytestmark = pytest.mark.gpu
B = 2
MEAN_CAM_T = (0., 0.2, 42.)


def _randomise_running_statistics(reg, seed=5):
    """non-trivial BatchNorm state: running means / variances away from (0, 1), a step count away from 0"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in reg.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(((torch.rand(m.num_features, generator=g) - 0.5) * 0.2).to(DEV))
                m.running_var.copy_((0.5 + torch.rand(m.num_features, generator=g)).to(DEV))
                m.num_batches_tracked.fill_(3)


def _parts(seed=0, train=False):
    torch.manual_seed(seed)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP).to(DEV)
    reg.train(train)
    _randomise_running_statistics(reg)
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=B).to(DEV)
    crit = straps_amd.HomoscedasticUncertaintyWeightedMultiTaskLoss(LOSSES, init_loss_weights=W, reduction='mean').to(DEV)
    return reg, smpl, crit


def _pools(n, seed=800):
    pose = det_uniform((n, 72), seed, -0.4, 0.4)
    pose[:, :3] *= 0.25
    return torch.from_numpy(pose).to(DEV), torch.from_numpy(det_uniform((n, 10), seed + 1, -1.5, 1.5)).to(DEV)


def _direct_head(keep):
    """straps_val_head on the tensors a step kept, into a zero accumulator -> (loss [12], per_sample [B,11], acc [24])"""
    L, p = hipabi.lib(), hipabi.ptr
    loss, rows = torch.full((12,), float('nan'), device=DEV), torch.full((B, 11), float('nan'), device=DEV)
    acc = torch.zeros(24, device=DEV, dtype=torch.float64)
    ws = torch.empty((L.straps_val_head_workspace_bytes(B) + 7) // 8, device=DEV, dtype=torch.float64)
    hipabi.check(L.straps_val_head(p(keep['pred_verts']), p(keep['pred_reposed']), p(keep['pred_joints']), p(keep['est']), keep['ld_est'], p(keep['pred_rot']),
                                   p(keep['verts']), p(keep['reposed']), p(keep['joints2d']), p(keep['joints3d']), p(keep['shape']), p(keep['rot']),
                                   p(keep['log_vars']), p(loss), p(rows), p(acc), p(ws), B, 6890, 256, hipabi.stream_ptr()), 'straps_val_head')
    return loss, rows, acc


@pytest.mark.parametrize('crop_input', [True, False])
def test_stages_against_the_oracle_and_direct_calls(crop_input):
    reg, smpl, crit = _parts()
    bbox = {'crop_input': crop_input, 'mean_scale_factor': 1.2, 'delta_scale_range': [-0.2, 0.2], 'delta_centre_range': [-5, 5]}
    vs = ValStep(reg, smpl, crit, B, mean_cam_t=MEAN_CAM_T, bbox_augment_params=bbox)
    pose, shape = _pools(B)
    keep = {}
    loss = vs.step(pose, shape, keep=keep)
    torch.cuda.synchronize()
    model = straps_amd.synthetic_smpl_model(0)
    cpu = lambda k: keep[k].cpu()
    # 1. rotations
    want_rot = O.batch_rodrigues(pose.cpu().reshape(-1, 3)).view(B, 24, 3, 3)
    assert float((cpu('rot') - want_rot).abs().max()) < 2e-6
    # 2. SMPL on identical (beta, R)
    ov, oj = O.smpl_forward(model, shape.cpu(), rotmats=cpu('rot'))
    assert float((cpu('verts') - ov).abs().max()) < 1e-5 and float((cpu('joints') - oj).abs().max()) < 1e-5
    orv, _ = O.smpl_forward(model, shape.cpu(), rotmats=torch.eye(3).expand(B, 24, 3, 3))
    assert float((cpu('reposed') - orv).abs().max()) < 1e-5
    # 3. projection at the mean camera + H36M-LSP joints, on the GPU's own joints
    jg = cpu('joints')
    cam_t = torch.tensor([MEAN_CAM_T]).expand(B, -1)
    K = torch.from_numpy(O.intrinsics_matrix().astype(np.float32))[None].expand(B, -1, -1)
    want2d = O.perspective_project(jg[:, O.ALL_JOINTS_TO_COCO_MAP], torch.eye(3)[None].expand(B, -1, -1), cam_t, K)
    assert float((cpu('joints2d_uncropped') - want2d).abs().max()) < 2e-3
    assert torch.equal(cpu('joints3d'), jg[:, O.ALL_JOINTS_TO_H36M_MAP][:, O.H36M_TO_J14])
    # 4. rasteriser without vertex noise: bit-exact on the GPU's vertices
    want_seg = O.rasterize_parts(cpu('verts').numpy(), model['faces'], model['face_parts'], O.intrinsics_matrix().astype(np.float32), np.eye(3), cam_t.numpy())
    np.testing.assert_array_equal(cpu('seg').numpy(), want_seg)
    assert 0.01 < float((want_seg != 0).mean()) < 0.6
    # 5. crop without jitter
    if crop_input:
        wc, wj, wb = O.crop_resize(want_seg, cpu('joints2d_uncropped').numpy(), None)
        np.testing.assert_array_equal(cpu('boxes').numpy()[:, :4], wb)
        np.testing.assert_array_equal(cpu('seg_cropped').numpy(), wc)
        np.testing.assert_allclose(cpu('joints2d').numpy(), wj, rtol=1e-5, atol=1e-3)
    else:
        wc = want_seg
        assert keep['boxes'] is None and keep['seg_cropped'] is keep['seg'] and keep['joints2d'] is keep['joints2d_uncropped']
    # 6. proxy input: nothing removed, occluded or jittered
    want_x = O.build_proxy_input(torch.from_numpy(wc), cpu('joints2d')).numpy()
    got_x = cpu('input').numpy()
    assert np.array_equal(got_x != 0, want_x != 0)
    np.testing.assert_allclose(got_x, want_x, rtol=0, atol=2e-6)
    assert np.array_equal(got_x[:, 0], (wc != 0).astype(np.float32))
    # 7. the eval-mode forward is the module's own
    assert not reg.training
    with torch.no_grad():
        cam, pose6, pshape = reg.eval()(keep['input'])
    assert torch.equal(cam, keep['cam']) and torch.equal(pose6, keep['pose']) and torch.equal(pshape, keep['pred_shape_view'])
    assert torch.equal(keep['pred_shape'], pshape)
    want_R = O.rot6d_to_rotmat(pose6.cpu().contiguous()).view(B, 24, 3, 3)
    assert float((cpu('pred_rot') - want_R).abs().max()) < 2e-6
    pv, pj = O.smpl_forward(model, pshape.cpu(), rotmats=cpu('pred_rot'))
    assert float((cpu('pred_verts') - pv).abs().max()) < 1e-5 and float((cpu('pred_joints') - pj).abs().max()) < 1e-5
    # 9. the head: a direct call on the kept tensors, bit for bit
    dl, dr, da = _direct_head(keep)
    assert torch.equal(dl, loss) and torch.equal(dl, keep['loss']) and torch.equal(dr, keep['per_sample']) and torch.equal(da, vs.acc)
    assert bool(torch.isfinite(dl).all()) and float(dl[11]) > 0 and float(vs.acc[23]) == B
    assert torch.equal(keep['log_vars'], crit.log_var_vector())


@pytest.mark.parametrize('train_mode', [False, True])
def test_a_step_moves_no_state(train_mode):
    reg, smpl, crit = _parts(train=train_mode)
    vs = ValStep(reg, smpl, crit, B)
    before = {k: v.detach().clone() for k, v in reg.state_dict().items()}
    crit_before = {k: v.detach().clone() for k, v in crit.state_dict().items()}
    flags = [m.training for m in reg.modules()]
    pose, shape = _pools(B)
    vs.step(pose, shape)
    vs(pose, shape)
    torch.cuda.synchronize()
    after = reg.state_dict()
    assert set(after) == set(before) and any(k.endswith('num_batches_tracked') for k in before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    for k, v in crit_before.items():
        assert torch.equal(crit.state_dict()[k], v), k
    assert reg.training == train_mode and [m.training for m in reg.modules()] == flags
    assert float(vs.acc[23]) == 2 * B


def test_validation_between_training_steps_changes_nothing():
    """step, step against step, ValStep.step, step on two identically seeded TrainSteps: losses and parameters bit for bit"""
    pose, shape = _pools(B)
    ts_a, _ = _step(B)
    ts_b, smpl_b = _step(B)
    vs = ValStep(ts_b.reg, smpl_b, ts_b.crit, B)
    la1, la2 = ts_a.step().clone(), ts_a.step().clone()
    lb1 = ts_b.step().clone()
    vloss = vs.step(pose, shape).clone()
    lb2 = ts_b.step().clone()
    torch.cuda.synchronize()
    assert torch.equal(la1, lb1) and torch.equal(la2, lb2)
    assert torch.equal(ts_a.flat_p, ts_b.flat_p) and torch.equal(ts_a.exp_avg, ts_b.exp_avg) and torch.equal(ts_a.exp_avg_sq, ts_b.exp_avg_sq)
    for (ka, va), (kb, vb) in zip(ts_a.reg.state_dict().items(), ts_b.reg.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    assert ts_b.reg.training and bool(torch.isfinite(vloss).all())
    # the next validation step sees the updated parameters, not a packed copy left from before the update
    assert not torch.equal(vs.step(pose, shape), vloss)
    ts_a.close()
    ts_b.close()


def test_run_summary_reset_and_short_batch():
    reg, smpl, crit = _parts()
    vs = ValStep(reg, smpl, crit, B)
    pose, shape = _pools(7)                              # three whole batches and a remainder of one
    s = vs.run(pose, shape)
    acc = vs.acc.cpu().numpy()
    assert s['num_samples'] == 6 and acc[23] == 6.0
    assert s['losses'] == acc[0] / 6.0
    for k, task in enumerate(('verts', 'joints2D', 'joints3D', 'shape_params', 'pose_params')):
        assert s[task + '_losses'] == acc[1 + k] / 6.0, task
    for k, key in enumerate(BatchMetrics.KEYS):
        assert s[key] == acc[12 + k] / (6.0 * PER_SAMPLE[key]) and s[key] > 0, key
    assert set(s) == {'losses', 'num_samples'} | {t + '_losses' for t in LOSSES} | set(BatchMetrics.KEYS)
    # the pass is the sum of its batches: the same three batches one by one
    vs.reset()
    assert not vs.acc.any()
    for k in range(3):
        vs.step(pose[k * B:(k + 1) * B], shape[k * B:(k + 1) * B])
    assert np.array_equal(vs.acc.cpu().numpy(), acc)
    vs.reset()
    assert not vs.acc.any()
    with pytest.raises(RuntimeError):
        vs.summary()
    with pytest.raises(ValueError):
        vs.step(pose[:1], shape[:1])
    with pytest.raises(ValueError):
        vs.run(pose[:1], shape[:1])
    assert not vs.acc.any()
