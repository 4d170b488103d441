"""GPU: straps_amd.Predictor -- predict/predict_3D.py:116-149 for a batch on the device.  It composes existing entry points only, so its
results equal the composition written out by hand bit for bit; a captured graph replays to the eager results; float and bool
silhouettes are the uint8 ones; `valid` marks the samples the reference would raise on; and the regressed parameters meet the CPU
oracle on the same proxy."""
import numpy as np
import pytest
import torch

import predict_cases as PC
import straps_amd
import straps_oracle as O
from straps_amd import cam_utils, hipabi

pytestmark = pytest.mark.gpu
MP = straps_amd.synthetic_mean_params(0)
MODEL = straps_amd.synthetic_smpl_model(0)
B = 3
KEYS = ('proxy_rep', 'cam_wp', 'pose', 'pose_rotmats', 'shape', 'vertices', 'joints', 'vertices2D', 'reposed_vertices', 'joints2D_cropped', 'boxes',
        'valid')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def parts(dev):
    """a seeded resnet18 regressor with randomised BatchNorm state in eval mode, the synthetic SMPL model, three golden-table inputs"""
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP)
    g = torch.Generator().manual_seed(19)
    with torch.no_grad():
        for m in reg.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.weight.shape[0]
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
    reg = reg.to(dev).eval()
    smpl = straps_amd.SMPL(MODEL, batch_size=B).to(dev)
    sil, joints = PC.inputs('a')
    return reg, smpl, torch.from_numpy(sil[:B]).to(dev), torch.from_numpy(joints[:B]).to(dev)


def _same(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert torch.equal(a[k], b[k]), '%s: %s differs' % (what, k)


def test_equals_the_manual_composition(dev, parts):
    reg, smpl, sil, joints = parts
    got = straps_amd.Predictor(reg, smpl)(sil, joints, vis_wh=512)
    assert set(got) == set(KEYS)
    with torch.no_grad():
        proxy, jc, boxes = straps_amd.create_proxy_representation_batch(sil, joints, out_wh=256, bbox_scale_factor=1.2, std=4)
        cam, pose, shape, rot = straps_amd.InferenceRegressor(reg)(proxy, rotmats=True)
        rot = rot.view(B, 24, 3, 3)
        verts, jts = smpl.forward_arrays(shape.contiguous(), rot)
        v2d = cam_utils.undo_keypoint_normalisation(cam_utils.orthographic_project_torch(verts, cam), 512)
        reposed, _ = smpl.forward_arrays(shape.contiguous(), torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous())
    want = dict(zip(KEYS, (proxy, cam, pose, rot, shape.contiguous(), verts, jts, v2d, reposed, jc, boxes, boxes[:, 4] != 0)))
    torch.cuda.synchronize()
    _same(got, want, 'Predictor vs manual composition')
    assert tuple(got['proxy_rep'].shape) == (B, 18, 256, 256) and tuple(got['pose_rotmats'].shape) == (B, 24, 3, 3)
    assert tuple(got['vertices'].shape) == (B, 6890, 3) and tuple(got['joints'].shape) == (B, 90, 3) and tuple(got['vertices2D'].shape) == (B, 6890, 2)
    assert got['valid'].dtype == torch.bool and got['valid'].all()
    assert all(torch.isfinite(got[k]).all() for k in KEYS if got[k].is_floating_point())
    # the module's own eval forward on the same proxy (what InferenceRegressor equals bit for bit), and vis_wh's default
    with torch.no_grad():
        mcam, mpose, mshape = reg(proxy)
    assert torch.equal(mcam, got['cam_wp']) and torch.equal(mpose, got['pose']) and torch.equal(mshape, got['shape'])
    dflt = straps_amd.Predictor(reg, smpl)(sil, joints)
    assert torch.equal(dflt['vertices2D'], cam_utils.undo_keypoint_normalisation(cam_utils.orthographic_project_torch(verts, cam), 256))
    # the proxy is the reference's: the restatement of the header at out_wh 256 (tests/test_gpu_predict_proxy.py holds it to the golden)
    rp, rj, rb = PC.proxy_input(sil.cpu().numpy(), joints.cpu().numpy(), straps_amd.heatmap_patch(4), 256)
    assert np.array_equal(got['proxy_rep'].cpu().numpy(), rp) and np.array_equal(got['boxes'].cpu().numpy(), rb)
    assert np.array_equal(got['joints2D_cropped'].cpu().numpy(), rj.astype(np.float32))


def test_graph_replay_equals_eager(dev, parts):
    reg, smpl, sil, joints = parts
    p = straps_amd.Predictor(reg, smpl)
    static_sil, static_j = sil.clone(), joints.clone()
    p(static_sil, static_j)                     # warm-up: workspace, Gaussian table and identity rotations exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = p(static_sil, static_j)
    allsil, alljoints = PC.inputs('a')
    for pick in ([2, 3, 4], [4, 0, 1]):
        s, j = torch.from_numpy(allsil[pick]).to(dev), torch.from_numpy(alljoints[pick]).to(dev)
        static_sil.copy_(s)
        static_j.copy_(j)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, p(s, j), 'graph replay %s vs eager' % pick)


def test_float_and_bool_silhouettes_and_valid(dev, parts):
    reg, smpl, sil, joints = parts
    p = straps_amd.Predictor(reg, smpl)
    mask = sil != 0
    mask[1] = False                             # an empty silhouette: the reference raises; here valid = 0 and an all-zero proxy
    want = p(mask.to(torch.uint8), joints)
    torch.cuda.synchronize()
    assert want['valid'].tolist() == [True, False, True] and want['boxes'][:, 4].tolist() == [1, 0, 1]
    assert not want['proxy_rep'][1].any() and not want['joints2D_cropped'][1].any()
    assert want['proxy_rep'][0].any() and want['proxy_rep'][2].any()
    _same(p(mask, joints), want, 'bool silhouettes')
    _same(p(mask.float(), joints), want, 'float silhouettes')
    _same(p(mask.to(torch.uint8), joints[:, :, :2].contiguous()), want, 'joints without a confidence column')
    # the valid samples do not depend on their invalid neighbour
    ref = p(sil != 0, joints)
    for k in ('proxy_rep', 'joints2D_cropped', 'boxes'):
        assert torch.equal(ref[k][0], want[k][0]) and torch.equal(ref[k][2], want[k][2]), k


def test_refresh_forwards_to_the_inference_regressor(dev, parts):
    reg, smpl, sil, joints = parts
    p = straps_amd.Predictor(reg, smpl)
    before = {k: v.clone() for k, v in p(sil, joints).items()}
    saved = reg.ief_module.fc3.bias.detach().clone()
    try:
        with torch.no_grad():
            reg.ief_module.fc3.bias.add_(0.01)
        _same(p(sil, joints), before, 'without refresh()')
        assert p.refresh() is p
        after = p(sil, joints)
        assert not torch.equal(after['cam_wp'], before['cam_wp'])
        _same(after, straps_amd.Predictor(reg, smpl)(sil, joints), 'after refresh()')
    finally:
        with torch.no_grad():
            reg.ief_module.fc3.bias.copy_(saved)


def test_regressed_parameters_meet_the_oracle_on_the_proxy(dev, parts):
    """oracle.predict_forward on the Predictor's own proxy, at the bound tests/test_gpu_regressor_infer.py::test_reference_golden holds the
    one-call regressor to against the reference's outputs: |d| <= 2e-4 + 2e-4 |ref| on (cam, pose, shape)"""
    reg, smpl, sil, joints = parts
    got = straps_amd.Predictor(reg, smpl)(sil, joints)
    sd = {k: v.detach().cpu() for k, v in reg.state_dict().items()}
    with torch.no_grad():
        ocam, opose, oshape, _, _ = O.predict_forward(got['proxy_rep'].cpu(), sd, O.ief_init_estimate(MP['pose'], MP['shape']), MODEL, 18, 3)
    out = torch.cat([got['cam_wp'], got['pose'], got['shape']], 1).cpu().double()
    ref = torch.cat([ocam, opose, oshape], 1).double()
    err = float(((out - ref).abs() / (2e-4 + 2e-4 * ref.abs())).max())
    print('Predictor vs oracle.predict_forward: %.3e of the 2e-4 tolerance' % err)
    assert err <= 1.0, 'Predictor vs oracle on the proxy: %.3e of the 2e-4 tolerance' % err
