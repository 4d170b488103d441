"""GPU: the fused loss head (csrc/train.hip: straps_loss_fwd_bwd, straps_loss_fwd_bwd_gm, straps_count_visible) at its edges, behind
redzones.

Reference: O.multi_task_loss with float64 autograd, composed as in test_fused_loss_vs_oracle (tests/loss_cases.py).  Every output
(loss[12], dverts, djoints, dest, drot, dlogvar) and the workspace (exactly straps_loss_workspace_bytes) is a guarded buffer pre-filled
with NaN, every input sits at the end of a NaN-poisoned allocation (tests/redzone.py).

Bars: those of test_fused_loss_vs_oracle -- 2e-5 on the losses and the log-variance gradients, 1e-5 on the gradients -- with the
gradients under the per-column (per joint, per vertex) and per-body metric of tests/grad_metrics.py instead of the tensor maximum, and
dverts compared in full.  djoints and dest are mostly structurally zero (joints outside the COCO / H36M maps, invisible joints, the
columns 3..146 of dest and its padding): the sparse form of the metric, exact zeros where the oracle's slice is zero.
"""
import numpy as np
import pytest
import torch

import grad_metrics as G
import loss_cases as LC
import smpl_cases as S
import straps_oracle as O
from detgen import det_uniform
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
EINVAL = 1
LOSS_RTOL, GRAD_BAR = 2e-5, 1e-5
COCO = list(O.ALL_JOINTS_TO_COCO_MAP)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    hipabi.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _oracle_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(S.cpu_threads())
    yield
    torch.set_num_threads(before)


def _compare(tag, got, ref, ld_est):
    lo = got['loss'].double().numpy()
    LC.assert_close_nan(tag + ' total', lo[0], ref['loss'][0], LOSS_RTOL)
    LC.assert_close_nan(tag + ' weighted task losses', lo[1:6], ref['loss'][1:6], LOSS_RTOL)
    LC.assert_close_nan(tag + ' raw MSEs', lo[6:11], ref['loss'][6:11], LOSS_RTOL)
    assert lo[11] == float(ref['loss'][11]), '%s: %d visible joints counted, the oracle sees %d' % (tag, lo[11], ref['loss'][11])
    if got['dlogvar'] is None:
        return
    LC.assert_close_nan(tag + ' dlogvar', got['dlogvar'].double().numpy(), ref['dlogvar'], LOSS_RTOL)
    de = got['dest']
    assert de.shape[1] == ld_est and not de[:, 157:].any(), tag + ': a padding column of dest is not exactly zero'
    G.assert_slices(tag + ' dverts', got['dverts'], ref['dverts'], GRAD_BAR)
    G.assert_slices(tag + ' drot', got['drot'], ref['drot'], GRAD_BAR)
    G.assert_slices(tag + ' djoints', got['djoints'], ref['djoints'], GRAD_BAR, sparse=True)
    G.assert_slices(tag + ' dest', de[:, :157], ref['dest'], GRAD_BAR, sparse=True)


def _modes(dev, x):
    """(tag, count argument, count_scale, the oracle's j2d_count): the plain entry point and _gm with this batch's own count from
    straps_count_visible, as the job-wide count of one rank (scale 1) and as half of a two-rank job's (scale 0.5)"""
    n = LC.count_visible(dev, x['tj2d'], Zone(dev))
    assert n == float(O.check_joints2d_visibility(x['tj2d']).sum())
    return (('plain', None, 1.0, None), ('gm x1', n, 1.0, n), ('gm x0.5', n, 0.5, 0.5 * n))


@pytest.mark.parametrize('B', [1, 2, 64, 255, 256, 257, 700])
def test_loss_head_batch_edges(dev, B):
    """one lane per body in blocks of 256 (heads), bodies strided by 256 (finalize), one wave per body (gradients); log-variances from +-2"""
    x = LC.make_inputs(B, seed=600 + B)
    for tag, count, scale, j2d_count in _modes(dev, x):
        ref = LC.reference(x, j2d_count=j2d_count)
        got = LC.run_kernel(dev, Zone(dev), x, count=count, count_scale=scale)
        _compare('B=%d %s' % (B, tag), got, ref, 160)
        if count is not None and scale == 1.0:
            plain = LC.run_kernel(dev, Zone(dev), x)
            assert all(torch.equal(got[k], plain[k]) for k in got), 'the global count of a single rank changes the result'


@pytest.mark.parametrize('ld_est', [157, 160, 192])
def test_loss_head_row_stride_of_est(dev, ld_est):
    """dest [B, ld_est]: the padding columns are exactly zero and nothing outside the buffer is written"""
    x = LC.make_inputs(5, ld_est=ld_est, seed=640)
    _compare('ld_est=%d' % ld_est, LC.run_kernel(dev, Zone(dev), x), LC.reference(x), ld_est)


def test_loss_head_refuses_before_any_launch(dev):
    """ld_est = 156, and some gradient outputs without the others: STRAPS_EINVAL, and no output has been touched"""
    LC.run_kernel(dev, Zone(dev), LC.make_inputs(3, ld_est=156, seed=641), expect_rc=EINVAL)
    x = LC.make_inputs(3, seed=641)
    for outs in (('dverts',), ('dlogvar',), ('dverts', 'djoints', 'dest', 'drot'), ('djoints', 'dest', 'drot', 'dlogvar')):
        LC.run_kernel(dev, Zone(dev), x, outputs=outs, expect_rc=EINVAL)


@pytest.mark.parametrize('B', [3, 257])
def test_loss_only_form_has_the_same_bits(dev, B):
    x = LC.make_inputs(B, seed=642)
    full = LC.run_kernel(dev, Zone(dev), x)
    only = LC.run_kernel(dev, Zone(dev), x, grads=False)
    assert torch.equal(full['loss'], only['loss'])
    _compare('loss only B=%d' % B, only, LC.reference(x), 160)


def _boundary_inputs():
    """body 0: targets exactly on 0.0 and on 256.0 in x and in y (visible: the reference compares strictly) and one step outside either
    (invisible; below zero that is the negative float32 subnormal); body 1: no visible joint; bodies 2, 3: generic"""
    x = LC.make_inputs(4, seed=650)
    t = x['tj2d']
    t[0] = torch.from_numpy(det_uniform((17, 2), 651, 20.0, 230.0))
    up, dn = np.nextafter(np.float32(256.0), np.float32(np.inf)), np.nextafter(np.float32(0.0), np.float32(-np.inf))
    assert up > 256.0 and dn < 0.0
    t[0, 0, 0], t[0, 1, 1], t[0, 2, 0], t[0, 3, 1] = 0.0, 0.0, 256.0, 256.0
    t[0, 4] = torch.tensor([0.0, 256.0])
    t[0, 5] = torch.tensor([-0.0, 100.0])
    t[0, 6, 0], t[0, 7, 1], t[0, 8, 0], t[0, 9, 1] = float(up), float(up), float(dn), float(dn)
    t[1, :, 0] = torch.from_numpy(det_uniform((17,), 652, 256.5, 300.0))
    t[1, 3, 0], t[1, 3, 1] = 100.0, -1.0
    vis = O.check_joints2d_visibility(t)
    assert vis[0].tolist() == [True] * 6 + [False] * 4 + [True] * 7 and not vis[1].any()
    return x, vis


def test_visibility_boundaries_and_a_body_without_a_visible_joint(dev):
    x, vis = _boundary_inputs()
    assert LC.count_visible(dev, x['tj2d'], Zone(dev)) == float(vis.sum())
    ref = LC.reference(x)
    got = LC.run_kernel(dev, Zone(dev), x)
    _compare('boundaries', got, ref, 160)
    assert int(got['loss'][11]) == int(vis.sum())
    # joints on the boundary carry a 2-D gradient, joints one step outside carry none (x, y of their COCO rows come from joints2D alone
    # unless the joint is in the H36M map as well: compare with the oracle's own zeros)
    dj, rj = got['djoints'], ref['djoints']
    assert torch.equal(dj == 0, rj == 0), 'zero pattern of djoints differs from the oracle\'s'
    for k in range(6):
        assert dj[0, COCO[k], :2].abs().sum() > 0
    assert not got['dest'][1, :3].any(), 'camera gradient of the body without a visible joint'
    only_coco = [j for j in COCO if not rj[1, j].any()]
    assert only_coco and not dj[1, only_coco].any()


def test_a_batch_without_any_visible_joint_is_nan_where_the_oracle_is(dev):
    """0 / 0: the joints2D loss, the total and the joints2D log-variance gradient are NaN like float64 autograd of the oracle (nn.MSELoss
    over an empty selection); every gradient the oracle keeps finite is finite and equal, dest[:, :3] exactly zero"""
    x = LC.make_inputs(3, seed=660)
    x['tj2d'] = torch.from_numpy(det_uniform((3, 17, 2), 661, 257.0, 300.0))
    ref = LC.reference(x)
    assert torch.isnan(ref['loss'][[0, 2, 7]]).all() and torch.isfinite(ref['loss'][[1, 3, 4, 5, 6, 8, 9, 10]]).all()
    assert torch.isnan(ref['dlogvar']).tolist() == [False, True, False, False, False]
    assert torch.isfinite(ref['djoints']).all() and torch.isfinite(ref['dest']).all() and not ref['dest'][:, :3].any()
    assert LC.count_visible(dev, x['tj2d'], Zone(dev)) == 0.0
    got = LC.run_kernel(dev, Zone(dev), x)
    _compare('no visible joint', got, ref, 160)
    assert all(bool(torch.isfinite(got[k]).all()) for k in ('dverts', 'djoints', 'dest', 'drot'))
    assert not got['dest'][:, :3].any()


@pytest.mark.parametrize('n', [1, 255, 256, 257, 17 * 700])
def test_count_visible_sizes(dev, n):
    """batch * nj = n (one block of 256 lanes strides the joints)"""
    t = torch.from_numpy(det_uniform((n, 1, 2), 670 + n % 7, -40.0, 300.0))
    for i, v in enumerate((0.0, 256.0, float(np.nextafter(np.float32(256.0), np.float32(np.inf))), float(np.nextafter(np.float32(0.0), np.float32(-1.0))))):
        t[(i * 37) % n, 0, i % 2] = v
        t[n - 1 - (i * 5) % n, 0, (i + 1) % 2] = v
    want = float(O.check_joints2d_visibility(t).sum())
    assert LC.count_visible(dev, t, Zone(dev)) == want
    assert LC.count_visible(dev, t.view(1, n, 2), Zone(dev)) == want


def test_camera_scale_negative_zero_and_tiny(dev):
    """est[:, 0] = -0.7, 0, 1e-3: a zero scale makes the 2-D joint gradient vanish and leaves the scale's own gradient"""
    x = LC.make_inputs(4, seed=680, j2d_range=(20.0, 230.0))
    x['est'][:3, 0] = torch.tensor([-0.7, 0.0, 1e-3])
    ref = LC.reference(x)
    got = LC.run_kernel(dev, Zone(dev), x)
    _compare('camera scale', got, ref, 160)
    only_coco = [j for j in COCO if not ref['djoints'][1, j].any()]
    assert only_coco and not got['djoints'][1, only_coco].any() and got['dest'][1, 0] != 0 and not got['dest'][1, 1:3].any()
