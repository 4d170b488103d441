"""GPU: straps_fit_keypoints (csrc/fit.hip) and its Python surface against the float64 reference of tests/fit_cases.py.

Every output of a raw call sits behind redzone guards, every input ends against a NaN margin.  The float64 trajectories are computed once
per process (fit_cases.reference_fit).  Bounds: kp2d 2e-5 (this project's SMPL-vs-oracle bar), energy relative 1e-5, gradient relative
1e-4 per block (the bar of test_gpu_pose_grad.py); the trajectory bounds 2e-5 / 1e-4 are about 13x / 26x what an fp32 restatement of the
loop measured on the CPU (1.5e-6 / 3.8e-6).
Measured on MI355X (standard case, 100 iterations): |est_100 - float64| 8.3e-7 (sigma 0) and 2.5e-6 (sigma 0.1); energy trace relative
6.2e-6 and 8.2e-6 -- all below a third of their bounds.  Evaluation, largest over all keypoint sets and batch sizes: kp2d 2.5e-7, energy 6.2e-7, gradient per block 1.8e-6 (DESIGN.md has the same figures)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fit_cases as FC
import predict_cases as PC
import straps_amd
from redzone import Zone
from smpl_cases import cpu_threads
from straps_amd import hipabi
from straps_amd.fit import KeypointFitter, fit_keypoints_raw, pack_fit_model

pytestmark = pytest.mark.gpu
BLOCKS = ((0, 3), (3, 147), (147, 157))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    torch.set_num_threads(cpu_threads())
    return torch.device('cuda:0')


_TABLES = {}


def tables(dev, spec=None):
    """-> (FitModelStruct, n_kp) of the synthetic model for a keypoint set, uploaded once"""
    key = repr(spec)
    if key not in _TABLES:
        p = pack_fit_model(FC.MODEL, spec)
        t = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(dev) for k in ('j_template', 'j_shapedirs', 'parents', 'vert_dirs', 'vert_w', 'kp_src')}
        s = hipabi.FitModelStruct()
        for k, v in t.items():
            setattr(s, k, v.data_ptr() if v.numel() else None)
        s.n_verts, s.n_kp = p['n_verts'], p['n_kp']
        _TABLES[key] = (s, t, p['n_kp'])
    return _TABLES[key][0], _TABLES[key][2]


def run(dev, est, targets, conf, iters, est0=None, state=None, step0=0, sigma=0.0, lr=(0.01, 0.01, 0.01), lam=(1e-3, 1e-3), spec=None):
    """one raw call on guarded buffers -> dict of CPU tensors"""
    ms, nk = tables(dev, spec)
    z = Zone(dev)
    B = est.shape[0]
    e = z.guarded((B, 157), name='est')
    e.copy_(est)
    m = v = None
    if state is not None:
        m, v = z.guarded((B, 157), name='exp_avg'), z.guarded((B, 157), name='exp_avg_sq')
        m.copy_(state[0])
        v.copy_(state[1])
    out = {'energy': z.guarded((B, iters + 1), name='energy'), 'grad': z.guarded((B, 157), name='grad'), 'best_est': z.guarded((B, 157), name='best_est'),
           'best_energy': z.guarded((B,), name='best_energy'), 'kp2d': z.guarded((B, nk, 2), name='kp2d')}
    opts = hipabi.FitOptsStruct(iters, step0, lr[0], lr[1], lr[2], 0.9, 0.999, 1e-8, sigma, lam[0], lam[1], FC.IMG_WH)
    fit_keypoints_raw(ms, opts, e, None if est0 is None else z.at_end(est0.float()), z.at_end(targets.float()), None if conf is None else z.at_end(conf.float()),
                      m, v, out['energy'], out['grad'], out['best_est'], out['best_energy'], out['kp2d'])
    z.check()
    res = {k: t.cpu() for k, t in out.items()}
    res['est'] = e.cpu()
    if m is not None:
        res['exp_avg'], res['exp_avg_sq'] = m.cpu(), v.cpu()
    return res


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def check_evaluation(dev, case, spec, sigma, tag):
    est, tg, cf = case['est'], case['targets'], case['conf']
    est0 = est + torch.from_numpy(np.linspace(-0.02, 0.02, 157, dtype=np.float32))[None]
    got = run(dev, est, tg, cf, 0, est0=est0, sigma=sigma, spec=spec)
    E, g, p = FC.energy_grad(est.double(), est0.double(), tg.double(), cf.double(), sigma=sigma, spec=FC.COCO if spec is None else spec)
    e_kp = float((got['kp2d'].double() - p).abs().max())
    e_en = float(((got['energy'][:, 0].double() - E).abs() / E.abs().clamp_min(1e-30)).max())
    e_g = [float((got['grad'][:, a:b].double() - g[:, a:b]).abs().max() / g[:, a:b].abs().max()) for a, b in BLOCKS]
    print('%s sigma %g: kp2d %.2e, energy rel %.2e, grad rel (cam, pose, shape) %.2e %.2e %.2e' % (tag, sigma, e_kp, e_en, *e_g))
    assert e_kp < 2e-5 and e_en < 1e-5 and max(e_g) < 1e-4, (tag, sigma, e_kp, e_en, e_g)
    assert same_bits(got['est'], est)
    return got


@pytest.mark.parametrize('B', [1, 5, 9])
@pytest.mark.parametrize('sigma', [0.0, 0.1])
def test_evaluation_vs_float64(dev, B, sigma):
    full = FC.standard_case(B=9)
    case = {k: v[:B].clone() for k, v in full.items()}
    check_evaluation(dev, case, None, sigma, 'B=%d' % B)
    est, tg, cf = case['est'], case['targets'], case['conf']
    if B > 4:      # the body without keypoints, priors centred on the start: energy 0, gradient exactly 0
        got = run(dev, est, tg, cf, 0, sigma=sigma)
        assert float(got['energy'][4, 0]) == 0.0 and not bool(got['grad'][4].any())
    # a NaN target under a positive confidence: nothing changes but that keypoint's term
    b, k = B - 1 if B != 5 else 0, 5
    assert float(cf[b, k]) > 0
    tn, c0 = tg.clone(), cf.clone()
    tn[b, k, 0] = float('nan')
    c0[b, k] = 0.0
    a, w = run(dev, est, tn, cf, 0, sigma=sigma), run(dev, est, tg, c0, 0, sigma=sigma)
    assert same_bits(a['energy'], w['energy']) and same_bits(a['grad'], w['grad']) and bool(torch.isfinite(a['grad']).all())
    full_e = run(dev, est, tg, cf, 0, sigma=sigma)['energy']
    assert float(full_e[b, 0]) > float(a['energy'][b, 0])


def test_zero_iterations_leave_everything_alone(dev):
    case = FC.standard_case()
    m = torch.from_numpy(FC.det_uniform((6, 157), 77, -0.1, 0.1))
    v = torch.from_numpy(FC.det_uniform((6, 157), 78, 0.0, 0.01))
    got = run(dev, case['est'], case['targets'], case['conf'], 0, state=(m, v), step0=5)
    assert same_bits(got['est'], case['est']) and same_bits(got['exp_avg'], m) and same_bits(got['exp_avg_sq'], v)
    assert same_bits(got['best_est'], case['est']) and same_bits(got['best_energy'], got['energy'][:, 0])


def test_one_step_is_adam(dev):
    case = FC.standard_case()
    est, tg, cf = case['est'], case['targets'], case['conf']
    z = torch.zeros(6, 157)
    g = run(dev, est, tg, cf, 0)['grad']
    betas = (float(np.float32(0.9)), float(np.float32(0.999)))      # the float arguments the call receives
    for lr in ((0.01, 0.01, 0.01), (0.02, 0.005, 0.0), (0.0, 0.01, 0.01), (0.01, 0.0, 0.02)):
        got = run(dev, est, tg, cf, 1, state=(z, z), lr=lr)
        want, m1, v1 = FC.adam_update(est.double(), g.double(), z.double(), z.double(), 1, FC.lr_columns(lr), betas=betas)
        err = float((got['est'].double() - want).abs().max())
        print('one Adam step, lr %s: |est_1 - float64 formula| = %.2e' % (lr, err))
        assert err < 5e-7, (lr, err)
        # (the moments: two fp32 roundings of values below 0.4 and 0.02)
        assert float((got['exp_avg'].double() - m1).abs().max()) < 1e-7 and float((got['exp_avg_sq'].double() - v1).abs().max()) < 1e-8
        for (a, b), l in zip(BLOCKS, lr):
            moved = not same_bits(got['est'][:, a:b], est[:, a:b])
            assert moved == (l != 0.0), (lr, a)
    # later steps use t = step0 + 1 in the bias corrections
    m = torch.from_numpy(FC.det_uniform((6, 157), 79, -0.1, 0.1))
    v = torch.from_numpy(FC.det_uniform((6, 157), 80, 0.0, 0.01))
    got = run(dev, est, tg, cf, 1, state=(m, v), step0=41)
    want, _, _ = FC.adam_update(est.double(), g.double(), m.double(), v.double(), 42, FC.lr_columns((0.01,) * 3), betas=betas)
    assert float((got['est'].double() - want).abs().max()) < 5e-7


def test_chaining_is_bit_exact(dev):
    case = FC.standard_case()
    est, tg, cf = case['est'], case['targets'], case['conf']
    z = torch.zeros(6, 157)
    for sigma in (0.0, 0.1):
        whole = run(dev, est, tg, cf, 7, est0=est, state=(z, z), sigma=sigma)
        first = run(dev, est, tg, cf, 3, est0=est, state=(z, z), sigma=sigma)
        second = run(dev, first['est'], tg, cf, 4, est0=est, state=(first['exp_avg'], first['exp_avg_sq']), step0=3, sigma=sigma)
        for k in ('est', 'exp_avg', 'exp_avg_sq', 'grad', 'kp2d'):
            assert same_bits(whole[k], second[k]), k
        assert same_bits(whole['energy'][:, :4], first['energy']) and same_bits(whole['energy'][:, 3:], second['energy'])
        assert same_bits(first['energy'][:, 3], second['energy'][:, 0])
        assert not same_bits(whole['est'], est)


@pytest.mark.parametrize('name', ['sigma0', 'sigma01'])
def test_trajectory_vs_float64(dev, name):
    case, traj, en, kw = FC.reference_fit(name)
    got = run(dev, case['est'], case['targets'], case['conf'], 100, sigma=kw['sigma'])
    has_kp = (case['conf'] > 0).any(dim=1)
    e_est = float((got['est'].double() - traj[-1]).abs().max())
    e_en = float(((got['energy'][has_kp].double() - en[has_kp]).abs() / en[has_kp].abs()).max())
    print('trajectory %s: |est_100 - float64| = %.2e (bound 2e-5), energy trace relative %.2e (bound 1e-4)' % (name, e_est, e_en))
    assert e_est < 2e-5 and e_en < 1e-4, (e_est, e_en)
    assert same_bits(got['est'][4], case['est'][4]) and not bool(got['energy'][4].any())      # no keypoints: not a bit moves
    # the fit did what a fit is for: the reprojection error of the bodies with keypoints fell
    assert float((got['energy'][has_kp, -1] / got['energy'][has_kp, 0]).max()) < 0.1


def test_best_iterate(dev):
    case, _, en, kw = FC.reference_fit('nonmonotone')
    args = dict(sigma=kw['sigma'], lr=kw['lr'], lam=(kw['lambda_pose'], 1e-3))
    est, tg, cf = case['est'], case['targets'], case['conf']
    got = run(dev, est, tg, cf, 100, **args)
    tr = got['energy']
    rises = (tr[:, 1:] > tr[:, :-1]).sum(dim=1)
    assert int(rises[(cf > 0).any(dim=1)].min()) >= 5, rises
    assert same_bits(got['best_energy'], tr.min(dim=1).values)
    first = (tr == tr.min(dim=1, keepdim=True).values).float().argmax(dim=1)
    assert int(first[4]) == 0 and len(set(first.tolist())) > 1
    for idx in sorted(set(first.tolist())):
        stop = run(dev, est, tg, cf, idx, **args)
        for b in range(6):
            if int(first[b]) == idx:
                assert same_bits(stop['est'][b], got['best_est'][b]), (b, idx)
                assert same_bits(stop['energy'][b, idx], got['best_energy'][b])


def test_batch_independence(dev):
    full = FC.standard_case(B=9)
    est, tg, cf = full['est'], full['targets'], full['conf']
    keys = ('est', 'energy', 'grad', 'best_est', 'best_energy', 'kp2d')
    whole = run(dev, est, tg, cf, 6, sigma=0.1)
    for b in range(9):
        one = run(dev, est[b:b + 1], tg[b:b + 1], cf[b:b + 1], 6, sigma=0.1)
        for k in keys:
            assert same_bits(whole[k][b], one[k][0]), (b, k)
    perm = torch.tensor([3, 8, 0, 5, 1, 7, 2, 6, 4])
    p = run(dev, est[perm], tg[perm], cf[perm], 6, sigma=0.1)
    for k in keys:
        assert same_bits(p[k], whole[k][perm]), k
    bad = est.clone()
    bad[5, 40] = float('nan')
    n = run(dev, bad, tg, cf, 6, sigma=0.1)
    others = [b for b in range(9) if b != 5]
    for k in keys:
        assert same_bits(n[k][others], whole[k][others]), k
    assert bool(torch.isnan(n['energy'][5]).all())
    assert same_bits(n['best_est'][5], bad[5])                 # a NaN energy never replaces the first iterate


@pytest.mark.parametrize('which', ['kinematic32', 'vertices16'])
def test_other_keypoint_sets(dev, which):
    if which == 'kinematic32':
        spec = list(range(24)) + [23, 0, 15, 9, 12, 20, 21, 7]
    else:
        spec = [('vertex', v) for v in (0, 6889, 3, 411, 1000, 2222, 3333, 4444, 5000, 5555, 6000, 6500, 6888, 17, 3071, 4100)] + [('vertex', 6889), 5]
    pk = pack_fit_model(FC.MODEL, spec)
    assert (pk['n_verts'], pk['n_kp']) == ((0, 32) if which == 'kinematic32' else (16, 18))
    case = FC.standard_case(B=3, spec=spec, zero_body=99)
    for sigma in (0.0, 0.1):
        check_evaluation(dev, case, spec, sigma, which)
    got = run(dev, case['est'], case['targets'], case['conf'], 5, spec=spec)
    assert bool((got['energy'][:, -1] < got['energy'][:, 0]).all())


# ---------------------------------------------------------------- Python surface ----------------------------------------------------------------
@pytest.fixture(scope='module')
def smpl(dev):
    return straps_amd.SMPL(FC.MODEL, batch_size=1).to(dev)


def test_keypoint_fitter_equals_the_raw_call(dev, smpl):
    case = FC.standard_case()
    est, tg, cf = (case[k].to(dev) for k in ('est', 'targets', 'conf'))
    cam, pose, shape = est[:, :3].contiguous(), est[:, 3:147].contiguous(), est[:, 147:].contiguous()
    keep = [t.clone() for t in (cam, pose, shape, tg, cf)]
    fitter = KeypointFitter(smpl, iters=12, robust_sigma=0.1)
    assert (fitter.n_kp, fitter.n_verts) == (17, 5)
    out = fitter(cam, pose, shape, tg, conf=cf, trace=True)
    z = torch.zeros(6, 157)
    raw = run(dev, case['est'], case['targets'], case['conf'], 12, state=(z, z), sigma=0.1)
    torch.cuda.synchronize()
    for t, k in zip((cam, pose, shape, tg, cf), keep):
        assert torch.equal(t, k)
    got = torch.cat([out['cam_wp'], out['pose'], out['shape']], dim=1).cpu()
    assert same_bits(got, raw['est']) and same_bits(out['trace'].cpu(), raw['energy'])
    assert same_bits(out['energy0'].cpu(), raw['energy'][:, 0]) and same_bits(out['energy'].cpu(), raw['energy'][:, 12])
    assert same_bits(torch.cat([out['best'][k] for k in ('cam_wp', 'pose', 'shape')], dim=1).cpu(), raw['best_est'])
    assert same_bits(out['best']['energy'].cpu(), raw['best_energy'])
    assert same_bits(out['joints2D'].cpu(), (raw['kp2d'] + 1) * (FC.IMG_WH / 2.0))
    assert same_bits(out['state']['exp_avg'].cpu(), raw['exp_avg']) and out['state']['step'] == 12
    assert torch.equal(out['pose_rotmats'], straps_amd.rot6d_to_rotmat(out['pose'].contiguous()).view(6, 24, 3, 3))
    # a confidence column is the confidence; the state carries on
    out3 = fitter(cam, pose, shape, torch.cat([tg, cf[:, :, None]], dim=2))
    assert torch.equal(out3['pose'], out['pose'])
    more = fitter(out['cam_wp'], out['pose'], out['shape'], tg, conf=cf, prior=(cam, pose, shape), state=out['state'])
    both = run(dev, case['est'], case['targets'], case['conf'], 24, est0=case['est'], state=(z, z), sigma=0.1)
    assert same_bits(torch.cat([more['cam_wp'], more['pose'], more['shape']], dim=1).cpu(), both['est'])
    # evaluate is the iters = 0 call
    E, g, kp = fitter.evaluate(cam, pose, shape, tg, conf=cf)
    r0 = run(dev, case['est'], case['targets'], case['conf'], 0, sigma=0.1)
    assert same_bits(E.cpu(), r0['energy'][:, 0]) and same_bits(g.cpu(), r0['grad']) and same_bits(kp.cpu(), r0['kp2d'])
    # the module's rest-joint tables are the ones pack_fit_model computes from the model dict
    p = pack_fit_model(FC.MODEL)
    assert np.array_equal(smpl._k_j_template.cpu().numpy(), p['j_template']) and np.array_equal(smpl._k_j_shapedirs.cpu().numpy(), p['j_shapedirs'])


def test_keypoint_fitter_refuses_foreign_prior_and_state(dev, smpl):
    case = FC.standard_case()
    est, tg, cf = (case[k].to(dev) for k in ('est', 'targets', 'conf'))
    cam, pose, shape = est[:, :3].contiguous(), est[:, 3:147].contiguous(), est[:, 147:].contiguous()
    fitter = KeypointFitter(smpl, iters=2)
    with pytest.raises(RuntimeError, match='prior'):
        fitter(cam, pose, shape, tg, conf=cf, prior=case['est'])                         # a host tensor
    with pytest.raises(RuntimeError, match='prior'):
        fitter(cam, pose, shape, tg, conf=cf, prior=est[:5])
    good = fitter(cam, pose, shape, tg, conf=cf)['state']
    for bad in ({'exp_avg': good['exp_avg'].cpu()}, {'exp_avg_sq': good['exp_avg_sq'][:5]}, {'exp_avg': good['exp_avg'].double()}):
        with pytest.raises(RuntimeError, match='exp_avg'):
            fitter(cam, pose, shape, tg, conf=cf, state=dict(good, **bad))
    # a strided state is read as its values, and stays as it was
    wide = torch.zeros(6, 314, device=dev)
    wide[:, ::2] = good['exp_avg']
    a = fitter(cam, pose, shape, tg, conf=cf, state=dict(good, exp_avg=wide[:, ::2]))
    b = fitter(cam, pose, shape, tg, conf=cf, state=good)
    assert torch.equal(a['pose'], b['pose']) and torch.equal(wide[:, ::2], good['exp_avg'])


def test_prior_centre_of_the_camera_is_never_read(dev):
    case = FC.standard_case()
    est, tg, cf = case['est'], case['targets'], case['conf']
    est0 = est + 0.01
    bad = est0.clone()
    bad[:, :3] = float('nan')
    a, b = run(dev, est, tg, cf, 3, est0=est0), run(dev, est, tg, cf, 3, est0=bad)
    for k in ('est', 'energy', 'grad', 'best_est', 'kp2d'):
        assert same_bits(a[k], b[k]), k
    assert bool(torch.isfinite(b['energy']).all())


def test_keypoint_fitter_is_capturable(dev, smpl):
    case = FC.standard_case()
    est, tg, cf = (case[k].to(dev) for k in ('est', 'targets', 'conf'))
    cam, pose, shape = est[:, :3].contiguous(), est[:, 3:147].contiguous(), est[:, 147:].contiguous()
    fitter = KeypointFitter(smpl, iters=10)
    eager = fitter(cam, pose, shape, tg, conf=cf, trace=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = fitter(cam, pose, shape, tg, conf=cf, trace=True)
    graph.replay()
    torch.cuda.synchronize()
    for k in ('cam_wp', 'pose', 'shape', 'pose_rotmats', 'energy0', 'energy', 'joints2D', 'trace'):
        assert same_bits(cap[k], eager[k]), k
    assert same_bits(cap['best']['pose'], eager['best']['pose'])


def test_predictor_refine(dev, smpl):
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=straps_amd.synthetic_mean_params(0)).to(dev).eval()
    sil, joints = PC.inputs('a')
    sil, joints = torch.from_numpy(sil[:3].copy()).to(dev), torch.from_numpy(joints[:3]).to(dev)
    sil[2] = 0                                                    # an empty silhouette: invalid, passes through
    pred = straps_amd.Predictor(reg, smpl)
    out = pred(sil, joints)
    with pytest.raises(ValueError, match='img_wh'):
        pred.refine(out, KeypointFitter(smpl, iters=1, img_wh=224))
    with pytest.raises(ValueError, match='keypoints'):
        pred.refine(out, KeypointFitter(smpl, iters=1, keypoints=[0, 1, 2]))
    fitter = KeypointFitter(smpl, iters=20)
    ref = pred.refine(out, fitter)
    torch.cuda.synchronize()
    assert set(ref) == set(out) | {'energy0', 'energy'}
    assert out['valid'].tolist() == [True, True, False] and torch.equal(ref['valid'], out['valid'])
    verts, jts = smpl.forward_arrays(ref['shape'].contiguous(), ref['pose_rotmats'].contiguous())
    assert torch.equal(ref['vertices'], verts) and torch.equal(ref['joints'], jts)
    assert torch.equal(ref['pose_rotmats'], straps_amd.rot6d_to_rotmat(ref['pose'].contiguous()).view(3, 24, 3, 3))
    assert bool((ref['energy'][:2] < ref['energy0'][:2]).all())
    for k in ('cam_wp', 'pose', 'shape'):
        assert torch.equal(ref[k][2], out[k][2]) and not torch.equal(ref[k][0], out[k][0]), k
    assert float(ref['energy0'][2]) == 0.0 and torch.equal(ref['proxy_rep'], out['proxy_rep'])
