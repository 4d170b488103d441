"""GPU: fit.ScanFitter (csrc/scanfit.hip, fit.py) on the full synthetic model, batches of 1 and 3.

ScanFitter.evaluate is compared with the float64 composed objective of tests/scan_cases.py at the partners the GPU chose (energy 1e-5
relative, gradient 1e-4 of the largest magnitude per block: the keypoint fit's bars); the loop must equal the seven entry points written out
by hand, a split call must equal the whole, a captured graph must replay to the eager bits; on the prototype's trajectory recipe the final
vertex RMS to the true mesh and the final E_s2m must each be at most twice the float64 fit's (Adam's normalised step amplifies sign differences
of near-zero gradients: the silhouette fit's notes show final energies of single bodies differing by up to 10 % between two correct loops) and
inside the float64 fit's own conditions, 0.1 of the start (tests/test_scan_cases_cpu.py).
Measured on MI355X: see DESIGN.md, "Test-time fitting to a 3-D scan"."""
import ctypes as C

import pytest
import torch

import fit_cases as FC
import scan_cases as S
import straps_amd
from smpl_cases import cpu_threads
from straps_amd import hipabi
from straps_amd.fit import ScanFitter, fit_adam_raw, fit_keypoints_raw, scan_energy_raw

pytestmark = pytest.mark.gpu
BLOCKS = ((0, 3), (3, 147), (147, 157))
T = S.TRAJ


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    torch.set_num_threads(cpu_threads())
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def smpl(dev):
    return straps_amd.SMPL(FC.MODEL, batch_size=1).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def split(est):
    return est[:, :3].contiguous(), est[:, 3:147].contiguous(), est[:, 147:].contiguous()


def eval_inputs(B):
    """the three-body case's scans (B <= 3 of them) with a perturbed start, a translation included; the last point of body 0 is invalid"""
    c = S.three_body_case()
    est = c['est'][:B] + torch.from_numpy(FC.det_uniform((B, 157), 8250, -0.03, 0.03))
    pts = c['points'][:B].clone()
    pts[0, -1, 1] = float('nan')
    return est, pts


def fitter_for(smpl, iters, **kw):
    a = dict(sigma=0.1, w_s2m=T['w_s2m'], w_m2s=70.0, lr=(0.01, 0.02, 0.005))
    a.update(kw)
    return ScanFitter(smpl, iters=iters, **a)


@pytest.mark.parametrize('B', [1, 3])
def test_evaluate_vs_float64(dev, smpl, B):
    est, pts = eval_inputs(B)
    f = fitter_for(smpl, 0)
    E, g, terms = f.evaluate(*split(est.to(dev)), pts.to(dev))
    at = f(*split(est.to(dev)), pts.to(dev))      # iters = 0: one evaluation at the same parameters -- the partners the GPU chose
    assert same_bits(at['energy'], E) and same_bits(at['energy_terms'], terms)
    nv, npt = at['nearest_vertex'].cpu().long(), at['nearest_point'].cpu().long()
    assert int(nv[0, -1]) == -1 and bool((nv[0, :-1] >= 0).all()) and bool((nv[1:] >= 0).all()) and bool((npt >= 0).all())
    x = est.double()
    Ew, gw, tw = S.objective_grad(x, x.clone(), pts.double(), f.sigma, f.w_s2m, f.w_m2s, near_v=nv, near_p=npt)
    # the partners are nearest ones of the float64 mesh as well, but for near-ties that the rounding of an fp32 mesh decides: about 1.5 e of the queries
    # have a second-best squared distance within e relative of the best (scan_cases' independent draws), so 1e-3 allows for e = 6e-4 -- a thousand
    # times what fp32 rounding moves a squared distance by
    _, _, nv64, np64 = S.objective(x, x.clone(), pts.double(), f.sigma, f.w_s2m, f.w_m2s)
    assert float((nv != nv64).double().mean()) < 1e-3 and float((npt != np64).double().mean()) < 1e-3
    e_en = float(((E.cpu().double() - Ew).abs() / Ew.abs()).max())
    wt = torch.tensor([1.0, f.w_s2m, f.w_m2s], dtype=torch.float64)
    e_t = float((((terms.cpu().double() - tw).abs() * wt).max(dim=1).values / Ew.abs()).max())
    e_g = [float((g.cpu()[:, a:b].double() - gw[:, a:b]).abs().max() / gw[:, a:b].abs().max()) for a, b in BLOCKS]
    print('evaluate B=%d: energy rel %.2e, weighted terms rel-to-energy %.2e, grad rel-to-max (transl, pose, shape) %.2e %.2e %.2e' % (B, e_en, e_t, *e_g))
    assert e_en < 1e-5 and e_t < 1e-5 and max(e_g) < 1e-4, (e_en, e_t, e_g)
    assert float(terms[:, 0].max()) == 0.0      # (the priors are centred on the start)


def by_hand(dev, smpl, f, est, pts, iters):
    """the loop of ScanFitter.__call__ as its seven entry points"""
    L, st = hipabi.lib(), hipabi.stream_ptr()
    B, P = est.shape[0], pts.shape[1]
    est, est0 = est.clone(), est.clone()
    e = lambda *s: torch.empty(*s, device=dev)
    R, betas, verts, dverts, dtrans, e2, drot, dbetas, dx6, e_kp, g_kp = (e(B, 24, 3, 3), e(B, 10), e(B, 6890, 3), e(B, 6890, 3), e(B, 3), e(B, 2), e(B, 24, 3, 3),
                                                                           e(B, 10), e(B, 144), e(B, 1), e(B, 157))
    nv, npt = torch.empty(B, P, device=dev, dtype=torch.int32), torch.empty(B, 6890, device=dev, dtype=torch.int32)
    ws = torch.empty(L.straps_scan_energy_workspace_bytes(B, 6890, P) // 16 + 1, 2, device=dev, dtype=torch.float64)
    ws2 = e(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)
    m, v = torch.zeros(B, 157, device=dev), torch.zeros(B, 157, device=dev)
    energy, best, best_e = e(B, iters + 1), e(B, 157), e(B)
    targets, conf = torch.zeros(B, f.n_kp, 2, device=dev), torch.zeros(B, f.n_kp, device=dev)
    x6 = C.c_void_p(est.data_ptr() + 12)
    for i in range(iters + 1):
        hipabi.check(L.straps_rot6d_fwd(x6, 157, 24, hipabi.ptr(R), B, st), 'straps_rot6d_fwd')
        betas.copy_(est[:, 147:])
        smpl.forward_arrays(betas, R, want_joints=False, out_verts=verts)
        scan_energy_raw(verts, est, 157, pts, f.scan_opts(), e2, dverts, dtrans, nv, npt, ws)
        hipabi.check(L.straps_smpl_bwd(C.byref(smpl._model_struct()), hipabi.ptr(betas), hipabi.ptr(R), hipabi.ptr(dverts), None, hipabi.ptr(dbetas),
                                       hipabi.ptr(drot), hipabi.ptr(ws2), B, 0, st), 'straps_smpl_bwd')
        hipabi.check(L.straps_rot6d_bwd(x6, 157, 24, hipabi.ptr(drot), hipabi.ptr(dx6), 144, B, st), 'straps_rot6d_bwd')
        est_kp = est.clone()
        est_kp[:, :3] = torch.tensor([1.0, 0.0, 0.0], device=dev)
        fit_keypoints_raw(f._struct, f.opts(0), est_kp, est0, targets, conf, None, None, e_kp, g_kp, None, None, None)
        fit_adam_raw(f.opts(), est, g_kp, dtrans, dx6, dbetas, e_kp, e2, f.w_s2m, f.w_m2s, m, v, energy, i, None, best, best_e, i, i == 0, i < iters)
    return {'est': est, 'm': m, 'v': v, 'energy': energy, 'best': best, 'best_e': best_e, 'terms': torch.cat([e_kp, e2], dim=1), 'R': R,
            'verts': verts + est[:, None, :3], 'nv': nv, 'np': npt}


KEYS = {'transl', 'pose', 'shape', 'pose_rotmats', 'verts', 'energy0', 'energy', 'best', 'energy_terms', 'nearest_vertex', 'nearest_point', 'state', 'trace'}


@pytest.mark.parametrize('B', [1, 3])
def test_call_equals_the_seven_entry_points_and_a_split_call_equals_the_whole(dev, smpl, B):
    est, pts = eval_inputs(B)
    est, pts = est.to(dev), pts.to(dev)
    keep = [t.clone() for t in (est, pts)]
    f = fitter_for(smpl, 2)
    out = f(*split(est), pts, trace=True)
    hand = by_hand(dev, smpl, f, est, pts, 2)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip((est, pts), keep)), 'the inputs are not modified'
    got = torch.cat([out['transl'], out['pose'], out['shape']], dim=1)
    assert same_bits(got, hand['est']) and not same_bits(got, est) and bool((got[:, :3] != est[:, :3]).all()), 'the translation moves as well'
    assert same_bits(out['trace'], hand['energy']) and same_bits(out['energy0'], hand['energy'][:, 0]) and same_bits(out['energy'], hand['energy'][:, 2])
    assert same_bits(out['state']['exp_avg'], hand['m']) and same_bits(out['state']['exp_avg_sq'], hand['v']) and out['state']['step'] == 2
    assert same_bits(torch.cat([out['best'][k] for k in ('transl', 'pose', 'shape')], dim=1), hand['best']) and same_bits(out['best']['energy'], hand['best_e'])
    assert same_bits(out['energy_terms'], hand['terms']) and same_bits(out['pose_rotmats'], hand['R']) and same_bits(out['verts'], hand['verts'])
    assert torch.equal(out['nearest_vertex'], hand['nv']) and torch.equal(out['nearest_point'], hand['np'])
    assert set(out) == KEYS and set(out['best']) == {'transl', 'pose', 'shape', 'energy'} and set(f(*split(est), pts)) == KEYS - {'trace'}
    assert bool((out['energy'] < out['energy0']).all())
    # two calls of one iteration each, the state and the prior centre carried over
    g = fitter_for(smpl, 1)
    one = g(*split(est), pts)
    two = g(one['transl'].contiguous(), one['pose'].contiguous(), one['shape'].contiguous(), pts, prior=split(est), state=one['state'])
    for k in ('transl', 'pose', 'shape', 'energy', 'energy_terms', 'verts', 'pose_rotmats'):
        assert same_bits(two[k], out[k]), k
    assert torch.equal(two['nearest_vertex'], out['nearest_vertex']) and torch.equal(two['nearest_point'], out['nearest_point'])
    assert same_bits(two['state']['exp_avg'], out['state']['exp_avg']) and same_bits(two['state']['exp_avg_sq'], out['state']['exp_avg_sq']) and two['state']['step'] == 2
    with pytest.raises(RuntimeError, match='points'):
        f(*split(est), pts[:, :, :2])


@pytest.mark.parametrize('B', [1, 3])
def test_call_is_capturable(dev, smpl, B):
    est, pts = eval_inputs(B)
    est, pts = est.to(dev), pts.to(dev)
    f = fitter_for(smpl, 2)
    args = split(est) + (pts,)
    eager = f(*args, trace=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = f(*args, trace=True)
    graph.replay()
    torch.cuda.synchronize()
    for k in ('transl', 'pose', 'shape', 'pose_rotmats', 'verts', 'energy0', 'energy', 'trace', 'energy_terms'):
        assert same_bits(cap[k], eager[k]), k
    assert same_bits(cap['best']['pose'], eager['best']['pose']) and torch.equal(cap['nearest_vertex'], eager['nearest_vertex'])


def test_start_translation_is_the_difference_of_the_centroids(dev, smpl):
    est, pts = eval_inputs(3)
    est, pts = est.to(dev), pts.to(dev) + torch.tensor([0.3, -0.2, 1.5], device=dev)
    pts[1] = float('nan')      # a body without a valid point starts at zero and stays where it is
    f = fitter_for(smpl, 0)
    out = f(None, est[:, 3:147].contiguous(), est[:, 147:].contiguous(), pts)
    zero = f(torch.zeros(3, 3, device=dev), est[:, 3:147].contiguous(), est[:, 147:].contiguous(), pts)
    valid = torch.isfinite(pts).all(dim=2, keepdim=True)
    want = torch.where(valid, pts, torch.zeros_like(pts)).sum(dim=1) / valid.sum(dim=1).clamp(min=1) - zero['verts'].mean(dim=1)
    want[1] = 0.0
    assert float((out['transl'] - want).abs().max()) < 1e-5 and not bool(out['transl'][1].any())
    assert not bool(out['energy_terms'][1].any()) and bool((out['nearest_vertex'][1] == -1).all()) and bool((out['nearest_point'][1] == -1).all())
    assert bool((out['energy'][[0, 2]] < zero['energy'][[0, 2]]).all())


def test_trajectory_recipe(dev, smpl):
    c, ref = S.trajectory_case(), S.trajectory_reference()
    est, pts = c['est'].to(dev), c['points'].to(dev)
    f = ScanFitter(smpl, iters=T['iters'], lr=T['lr'], sigma=T['sigma'], w_s2m=T['w_s2m'], w_m2s=T['w_m2s'], lambda_pose=T['lambda_pose'],
                   lambda_shape=T['lambda_shape'])
    _, _, t0 = f.evaluate(*split(est), pts)
    out = f(*split(est), pts)
    final = torch.cat([out['transl'], out['pose'], out['shape']], dim=1).cpu()
    rms0, rms = ref['rms0'], S.vertex_rms(final, c['true_verts'])
    s0, s1 = t0[:, 1].cpu().double(), out['energy_terms'][:, 1].cpu().double()
    print('trajectory recipe: vertex RMS %s -> %s (float64 fit: %s); E_s2m %s -> %s (float64 fit: %s -> %s); E_m2s %s (float64 fit: %s)'
          % (rms0.tolist(), rms.tolist(), ref['rms'].tolist(), s0.tolist(), s1.tolist(), ref['terms'][0, :, 1].tolist(), ref['terms'][-1, :, 1].tolist(),
             out['energy_terms'][:, 2].tolist(), ref['terms'][-1, :, 2].tolist()))
    assert bool((rms <= 2.0 * ref['rms']).all()) and bool((s1 <= 2.0 * ref['terms'][-1, :, 1]).all()), 'at most twice the float64 fit'
    assert bool((rms <= 0.1 * rms0).all()) and bool((s1 <= 0.1 * s0).all()), "inside the float64 fit's own conditions"
    assert bool((out['energy'] < out['energy0']).all()) and bool((out['best']['energy'] <= out['energy']).all())
    # the mesh it reports is the mesh of the parameters it reports
    assert float((out['verts'].cpu().double() - S.mesh(final.double())).abs().max()) < 1e-4
