"""GPU: straps_fit_adam and fit.SilhouetteFitter (csrc/silfit.hip, fit.py) on the full synthetic model, batches of 1 and 3.

The update kernel must reproduce straps_fit_keypoints' own update bit for bit, at 1, 3, 4, 5 and 9 bodies (it places four bodies in a workgroup:
part of one, one whole, a ragged second, a ragged third), and is compared with a float64 Adam of the test's own at 4, 5 and 9 bodies (moments
within 2 ulp, est within half an ulp plus seven roundings of a step size; measured 0.93 and 1.31 ulp and 0.80 of the bound), where a body of
the batch of nine must equal the body run alone; SilhouetteFitter.evaluate is compared with the float64 composed
objective of tests/silfit_cases.py (energy 1e-5 relative, gradient 1e-4 of the largest magnitude per block: the keypoint fit's bars); the loop
must equal the seven entry points written out by hand, a split call must equal the whole, a captured graph must replay to the eager bits; the
standard trajectory case must end with its silhouette energy below half of its start (the float64 fit reaches a quarter:
tests/test_silfit_cases_cpu.py; the factor two is the margin for the fp32 path taking other branches at the kinks of the objective).
Measured on MI355X: evaluate -- energy 1.7e-7, gradient per block 2.6e-6, 5.4e-7, 2.5e-6 (a term's OWN relative error reached 1.5e-5 at B = 3, on
an E_out of 9.4e-7 beside an E_in of 1.1e-3: the terms are therefore judged weighted, against the energy's bar); trajectory ratios 0.117 and 0.141
(float64: 0.117 and 0.142).  DESIGN.md has the same figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import fit_cases as FC
import predict_cases as PC
import silfit_cases as SC
import straps_amd
from redzone import Zone
from smpl_cases import cpu_threads
from straps_amd import hipabi
from straps_amd.fit import KeypointFitter, SilhouetteFitter, distance_field, fit_adam_raw, fit_keypoints_raw, pack_fit_model, silhouette_energy_raw

pytestmark = pytest.mark.gpu
BLOCKS = ((0, 3), (3, 147), (147, 157))
T = SC.TRAJ


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    torch.set_num_threads(cpu_threads())
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def smpl(dev):
    return straps_amd.SMPL(FC.MODEL, batch_size=1).to(dev)


_TABLES = {}


def tables(dev):
    """-> (FitModelStruct, n_kp) of the synthetic model for the COCO keypoints, uploaded once"""
    if 'coco' not in _TABLES:
        p = pack_fit_model(FC.MODEL, None)
        t = {k: torch.from_numpy(np.ascontiguousarray(p[k])).to(dev) for k in ('j_template', 'j_shapedirs', 'parents', 'vert_dirs', 'vert_w', 'kp_src')}
        s = hipabi.FitModelStruct()
        for k, v in t.items():
            setattr(s, k, v.data_ptr() if v.numel() else None)
        s.n_verts, s.n_kp = p['n_verts'], p['n_kp']
        _TABLES['coco'] = (s, t, p['n_kp'])
    return _TABLES['coco'][0], _TABLES['coco'][2]


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def opts(iters=0, step0=0, lr=(0.01, 0.02, 0.005)):
    return hipabi.FitOptsStruct(iters, step0, lr[0], lr[1], lr[2], 0.9, 0.999, 1e-8, 0.0, 1e-3, 1e-3, FC.IMG_WH)


# ---------------------------------------------------------------- the update kernel ----------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 4, 5, 9])      # four bodies to a workgroup: part of one, one whole, one and a ragged second, two and a ragged third
@pytest.mark.parametrize('step0', [0, 5])
def test_update_kernel_is_the_keypoint_fit_update(dev, B, step0):
    case = {k: v[:B] for k, v in FC.standard_case(B=3 if B <= 3 else 9).items()}
    ms, nk = tables(dev)
    est0, tg, cf = (case[k].to(dev) for k in ('est', 'targets', 'conf'))
    if step0:
        m0 = torch.from_numpy(FC.det_uniform((B, 157), 77, -0.1, 0.1)).to(dev)
        v0 = torch.from_numpy(FC.det_uniform((B, 157), 78, 0.0, 0.01)).to(dev)
    else:
        m0, v0 = torch.zeros(B, 157, device=dev), torch.zeros(B, 157, device=dev)
    # the reference: one iteration inside straps_fit_keypoints
    e1, m1, v1 = est0.clone(), m0.clone(), v0.clone()
    en1, best1, beste1 = torch.empty(B, 2, device=dev), torch.empty(B, 157, device=dev), torch.empty(B, device=dev)
    fit_keypoints_raw(ms, opts(1, step0), e1, None, tg, cf, m1, v1, en1, None, best1, beste1, None)
    # its evaluation, then the update as a launch of its own
    ev, en0, g0 = est0.clone(), torch.empty(B, 1, device=dev), torch.empty(B, 157, device=dev)
    fit_keypoints_raw(ms, opts(0), ev, None, tg, cf, None, None, en0, g0, None, None, None)
    z = Zone(dev)
    e2, m2, v2 = z.guarded((B, 157), name='est'), z.guarded((B, 157), name='exp_avg'), z.guarded((B, 157), name='exp_avg_sq')
    e2.copy_(est0), m2.copy_(m0), v2.copy_(v0)
    trace, grad = z.guarded((B, 4), name='energy'), z.guarded((B, 157), name='grad')
    best, best_e = z.guarded((B, 157), name='best_est'), z.guarded((B,), name='best_energy')
    fit_adam_raw(opts(0), e2, z.at_end(g0), None, None, None, z.at_end(en0), None, 100.0, 100.0, m2, v2, trace, 2, grad, best, best_e, step0, True, True)
    z.check()
    assert same_bits(e2, e1) and same_bits(m2, m1) and same_bits(v2, v1), 'the update differs from the one inside straps_fit_keypoints'
    assert not same_bits(e2, est0)
    assert same_bits(trace[:, 2], en0[:, 0]) and same_bits(trace[:, 2], en1[:, 0]) and bool(torch.isnan(trace[:, [0, 1, 3]]).all())
    assert same_bits(grad, g0) and same_bits(best, est0) and same_bits(best_e, en0[:, 0])
    # evaluate only: est and the moments stay, the energy and the best pair are written; a larger or NaN energy does not replace what is held
    keep = [t.clone() for t in (e2, m2, v2)]
    higher = en0 * 2 + 1
    fit_adam_raw(opts(0), e2, g0, None, None, None, higher, None, 100.0, 100.0, m2, v2, trace, 3, None, best, best_e, step0 + 1, False, False)
    fit_adam_raw(opts(0), e2, g0, None, None, None, higher * float('nan'), None, 100.0, 100.0, m2, v2, trace, 0, None, best, best_e, step0 + 1, False, False)
    z.check()
    assert all(same_bits(a, b) for a, b in zip((e2, m2, v2), keep))
    assert same_bits(trace[:, 3], higher[:, 0]) and same_bits(best, est0) and same_bits(best_e, en0[:, 0])
    lower = en0 * 0.5
    fit_adam_raw(opts(0), e2, g0, None, None, None, lower, None, 100.0, 100.0, None, None, None, 0, None, best, best_e, step0 + 1, False, False)
    z.check()
    # (the body without keypoints, row 4 of the B = 9 case, has E = 0 exactly: half of it is not lower, and an equal energy does not replace)
    strict = (lower < en0)[:, 0]
    assert strict.tolist() == [b != 4 for b in range(B)]
    assert same_bits(best[strict], e2[strict]) and same_bits(best[~strict], est0[~strict]) and same_bits(best_e, lower[:, 0])


def test_update_kernel_adds_the_silhouette_terms(dev):
    for B in (3, 5):      # part of a workgroup of four bodies; one whole and a ragged second
        u = lambda shape, k: torch.from_numpy(FC.det_uniform(shape, 8100 + k, -1.0, 1.0)).to(dev)
        est, g_kp, dcam, dx6, dbetas, e_kp, e2 = u((B, 157), 0), u((B, 157), 1), u((B, 3), 2), u((B, 144), 3), u((B, 10), 4), u((B, 1), 5).abs(), u((B, 2), 6).abs()
        z = Zone(dev)
        grad, en = z.guarded((B, 157), name='grad'), z.guarded((B, 1), name='energy')
        fit_adam_raw(opts(0), est, g_kp, dcam, dx6, dbetas, e_kp, e2, 3.0, 0.25, None, None, en, 0, grad, None, None, 0, True, False)
        z.check()
        assert same_bits(grad, g_kp + torch.cat([dcam, dx6, dbetas], dim=1))
        want = e_kp[:, 0].double() + 3.0 * e2[:, 0].double() + 0.25 * e2[:, 1].double()
        assert float(((en[:, 0].double() - want).abs() / want).max()) < 3e-7
        fit_adam_raw(opts(0), est, None, None, dx6, None, None, e2, 3.0, 0.25, None, None, en, 0, grad, None, None, 0, True, False)
        z.check()
        assert same_bits(grad[:, 3:147], dx6) and not bool(grad[:, :3].any()) and not bool(grad[:, 147:].any())


LR = (0.01, 0.02, 0.005)      # opts()' learning rates: one per column group, all different
_ADAM = {}


def adam_case(step):
    """nine bodies of det_uniform inputs for one update at `step` (a smaller batch takes the first rows), with the float64 result.
    -> dict of CPU tensors: fp32 'est', 'g_kp', 'dcam', 'dx6', 'dbetas', 'e_kp', 'e2', 'm0', 'v0', 'g' (the fp32 sum of the four gradients: one
    IEEE addition per element, which the test demands of the kernel bit for bit), float64 'est1', 'm1', 'v1', 'E', 'step_size' [157].

    The float64 Adam is include/straps_hip.h's statement of straps_adam_step, m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) with t = step + 1, on the fp32 values of lr, b1, b2 and eps that the options hold.
    The inputs meet two conditions, asserted here, under which the test's bounds follow from fp32's precision:
      no cancellation in m: a moment at step 5 has the sign of its gradient (0.01 .. 0.1 in magnitude), so the two roundings of m are each at
        most half an ulp of m; v is a sum of positive terms, v0 in 0.002 .. 0.01 so that (1 - b2) g^2 <= 0.004 is at most two thirds of v: three
        roundings, at most 1.83 ulp of v;
      |m| / (sqrt(v) / sqrt(1 - b2^t) + eps) <= 0.7: the quotient carries about ten roundings in the worst case (two in m, 1.83 through the root
        of v, the root, the two casts of the bias corrections, the products, the fma of the denominator, the division); with the update at most
        0.7 step sizes they stay below seven roundings of one step size."""
    if step not in _ADAM:
        B = 9
        u = lambda shape, k, lo=-1.0, hi=1.0: torch.from_numpy(FC.det_uniform(shape, 8400 + 20 * step + k, lo, hi))
        c = {'est': u((B, 157), 0), 'g_kp': u((B, 157), 1), 'dcam': u((B, 3), 2), 'dx6': u((B, 144), 3), 'dbetas': u((B, 10), 4), 'e_kp': u((B, 1), 5).abs(),
             'e2': u((B, 2), 6).abs()}
        g = c['g_kp'] + torch.cat([c['dcam'], c['dx6'], c['dbetas']], dim=1)
        assert g.dtype == torch.float32 and bool((g != 0).all())
        if step:
            c['m0'], c['v0'] = torch.sign(g) * u((B, 157), 7, 0.01, 0.1), u((B, 157), 8, 0.002, 0.01)
        else:
            c['m0'], c['v0'] = torch.zeros(B, 157), torch.zeros(B, 157)
        f32 = lambda x: float(np.float32(x))
        b1, b2, eps, t = f32(0.9), f32(0.999), f32(1e-8), step + 1
        g64, m0, v0 = g.double(), c['m0'].double(), c['v0'].double()
        m1 = b1 * m0 + (1.0 - b1) * g64
        v1 = b2 * v0 + (1.0 - b2) * g64 * g64
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        ss = torch.tensor([f32(LR[0])] * 3 + [f32(LR[1])] * 144 + [f32(LR[2])] * 10, dtype=torch.float64) / bc1
        quot = m1 / (v1.sqrt() / bc2 ** 0.5 + eps)
        assert bool((m0 * g64 >= 0).all()) and float(quot.abs().max()) <= 0.7 and float(((1.0 - b2) * g64 * g64 / v1).max()) <= (1.0 if step == 0 else 2.0 / 3.0)
        c.update(g=g, m1=m1, v1=v1, est1=c['est'].double() - ss * quot, step_size=ss,
                 E=c['e_kp'][:, 0].double() + 3.0 * c['e2'][:, 0].double() + 0.25 * c['e2'][:, 1].double())
        _ADAM[step] = c
    return _ADAM[step]


def ulp32(x):
    """float64 tensor -> the spacing of fp32 at |x|"""
    return torch.from_numpy(np.spacing(x.abs().numpy().astype(np.float32)).astype(np.float64))


def run_adam(dev, c, rows, step):
    """one updating straps_fit_adam call on the bodies `rows` of an adam_case, all outputs guarded -> dict of CPU tensors"""
    B = rows.stop - rows.start
    z = Zone(dev)
    est, m, v = z.guarded((B, 157), name='est'), z.guarded((B, 157), name='exp_avg'), z.guarded((B, 157), name='exp_avg_sq')
    est.copy_(c['est'][rows]), m.copy_(c['m0'][rows]), v.copy_(c['v0'][rows])
    trace, grad = z.guarded((B, 4), name='energy'), z.guarded((B, 157), name='grad')
    best, best_e = z.guarded((B, 157), name='best_est'), z.guarded((B,), name='best_energy')
    ins = [z.at_end(c[k][rows]) for k in ('g_kp', 'dcam', 'dx6', 'dbetas', 'e_kp', 'e2')]
    fit_adam_raw(opts(0), est, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], 3.0, 0.25, m, v, trace, 2, grad, best, best_e, step, True, True)
    z.check()
    return {k: t.cpu() for k, t in (('est', est), ('m', m), ('v', v), ('trace', trace), ('grad', grad), ('best', best), ('best_e', best_e))}


@pytest.mark.parametrize('B', [4, 5, 9])      # four bodies to a workgroup: one whole; one and a ragged second; two and a ragged third
@pytest.mark.parametrize('step', [0, 5])
def test_update_kernel_vs_float64_adam(dev, B, step):
    """straps_fit_adam's update beside an Adam of its own, float64, written out in adam_case from the header's formula -- no model, no other kernel.
    Bounds (adam_case states the input conditions they rest on): the moments 2 ulp of their own value (one or two fp32 operations each, three for v
    at step 5); est half an fp32 ulp of |est| for the final subtraction, plus the element's step size lr / (1 - b1^t) times 2^-24 for each of the
    seven fp32 roundings of the chain.  A row of the B = 9 call must equal the same body run alone, bit for bit: the wave's place in its
    workgroup and the workgroup's index do not matter.
    Measured on MI355X, worst over the six cases: exp_avg 0.93 ulp, exp_avg_sq 1.31 ulp (step 0, where it is the twice-rounded (1 - b2) g^2
    itself; 1.01 at step 5), est 0.80 of its bound (step 5; 0.23 at step 0), energy 6.8e-8 relative."""
    c = adam_case(step)
    got = run_adam(dev, c, slice(0, B), step)
    assert same_bits(got['grad'], c['g'][:B]), 'the gradient is the fp32 sum of its four parts'
    e_m = float(((got['m'].double() - c['m1'][:B]).abs() / ulp32(c['m1'][:B])).max())
    e_v = float(((got['v'].double() - c['v1'][:B]).abs() / ulp32(c['v1'][:B])).max())
    bound = 0.5 * ulp32(c['est1'][:B]) + c['step_size'] * 7.0 * 2.0 ** -24
    e_est = float(((got['est'].double() - c['est1'][:B]).abs() / bound).max())
    e_E = float(((got['trace'][:, 2].double() - c['E'][:B]).abs() / c['E'][:B]).max())
    print('B=%d step %d: exp_avg %.2f ulp, exp_avg_sq %.2f ulp, est %.3f of its bound, energy rel %.2e' % (B, step, e_m, e_v, e_est, e_E))
    assert e_m <= 2.0 and e_v <= 2.0 and e_est <= 1.0 and e_E < 3e-7, (e_m, e_v, e_est, e_E)
    assert not same_bits(got['est'], c['est'][:B]) and bool(((got['est'] - c['est'][:B]).abs() > 0).all()), 'every element moves'
    # the unused energy columns stay (the margins of every buffer: run_adam), the best pair is the evaluated iterate
    assert bool(torch.isnan(got['trace'][:, [0, 1, 3]]).all())
    assert same_bits(got['best'], c['est'][:B]) and same_bits(got['best_e'], got['trace'][:, 2])
    if B == 9:
        for b in range(B):
            alone = run_adam(dev, c, slice(b, b + 1), step)
            assert all(same_bits(alone[k], got[k][b:b + 1]) for k in got), (b, 'a body alone differs from the body in its batch')


# ---------------------------------------------------------------- evaluate ----------------------------------------------------------------
def eval_inputs(dev, B):
    """the three-body case's targets (B <= 3 of them) with a perturbed start and keypoint targets of the true bodies"""
    c = SC.three_body_case()
    true = c['true'][:B]
    est = c['est'][:B] + torch.from_numpy(FC.det_uniform((B, 157), 8200, -0.03, 0.03))
    with torch.no_grad():
        p = SC.O.orthographic_project(FC.keypoints3d(true.double(), FC.COCO), true.double()[:, :3])
    targets = ((p + 1.0) * (T['wh'] / 2.0)).float()
    conf = torch.from_numpy(FC.det_uniform((B, 17), 8300, 0.3, 1.0))
    return est, targets, conf, c['masks'][:B], c['d2'][:B]


def split(est):
    return est[:, :3].contiguous(), est[:, 3:147].contiguous(), est[:, 147:].contiguous()


def fitter_for(smpl, iters, **kw):
    return SilhouetteFitter(smpl, iters=iters, lattice=T['lattice'], tau=T['tau'], w_in=T['w_in'], w_out=T['w_out'], img_wh=T['wh'], **kw)


@pytest.mark.parametrize('B', [1, 3])
def test_evaluate_vs_float64(dev, smpl, B):
    est, targets, conf, masks, d2 = eval_inputs(dev, B)
    f = fitter_for(smpl, 0)
    sil = torch.from_numpy(masks).to(dev)
    assert torch.equal(distance_field(sil).cpu(), torch.from_numpy(d2))
    E, g, terms = f.evaluate(*split(est.to(dev)), sil, targets.to(dev), conf=conf.to(dev))
    Ew, gw, tw = SC.objective_grad(est.double(), est.double(), masks, d2, targets.double(), conf.double(), T['lattice'], T['tau'], T['w_in'], T['w_out'])
    e_en = float(((E.cpu().double() - Ew).abs() / Ew.abs()).max())
    # the terms, each weighted as it enters E, against the bar of E itself: a term's own relative error is no measure -- E_out of a body the model
    # nearly covers is a thousandth of E_in (9.4e-7 for the third body here), and in float64 a shift of the projection by 1e-5 px, the size of
    # fp32's rounding of a grid coordinate at wh = 64, already moves it by 1.05e-5 relative
    wt = torch.tensor([1.0, T['w_in'], T['w_out']], dtype=torch.float64)
    e_t = float((((terms.cpu().double() - tw).abs() * wt).max(dim=1).values / Ew.abs()).max())
    e_g = [float((g.cpu()[:, a:b].double() - gw[:, a:b]).abs().max() / gw[:, a:b].abs().max()) for a, b in BLOCKS]
    print('evaluate B=%d: energy rel %.2e, weighted terms rel-to-energy %.2e, grad rel-to-max (cam, pose, shape) %.2e %.2e %.2e' % (B, e_en, e_t, *e_g))
    assert e_en < 1e-5 and e_t < 1e-5 and max(e_g) < 1e-4, (e_en, e_t, e_g)
    # without keypoints: all-zero confidences, bit for bit
    a = f.evaluate(*split(est.to(dev)), sil)
    b = f.evaluate(*split(est.to(dev)), sil, targets.to(dev), conf=torch.zeros(B, 17, device=dev))
    assert all(same_bits(x, y) for x, y in zip(a, b))
    assert float(a[2][:, 0].max()) == 0.0      # (the priors are centred on the start)


# ---------------------------------------------------------------- the loop ----------------------------------------------------------------
def by_hand(dev, smpl, f, est, targets, conf, sil, iters):
    """the loop of SilhouetteFitter.__call__ as its seven entry points"""
    L, st = hipabi.lib(), hipabi.stream_ptr()
    B = est.shape[0]
    est, est0 = est.clone(), est.clone()
    mask = (sil != 0).to(torch.uint8)
    d2 = torch.empty(mask.shape, device=dev, dtype=torch.int32)
    hipabi.check(L.straps_distance_field(hipabi.ptr(mask), hipabi.ptr(d2), B, mask.shape[1], st), 'straps_distance_field')
    e = lambda *s: torch.empty(*s, device=dev)
    R, betas, verts, dverts, dcam, e2, drot, dbetas, dx6, e_kp, g_kp = (e(B, 24, 3, 3), e(B, 10), e(B, 6890, 3), e(B, 6890, 3), e(B, 3), e(B, 2), e(B, 24, 3, 3),
                                                                         e(B, 10), e(B, 144), e(B, 1), e(B, 157))
    ws = torch.empty(L.straps_silhouette_energy_workspace_bytes(B, 6890, f.wh, f.lattice) // 8, device=dev, dtype=torch.float64)
    ws2 = e(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)
    m, v = torch.zeros(B, 157, device=dev), torch.zeros(B, 157, device=dev)
    energy, best, best_e = e(B, iters + 1), e(B, 157), e(B)
    x6 = C.c_void_p(est.data_ptr() + 12)
    for i in range(iters + 1):
        hipabi.check(L.straps_rot6d_fwd(x6, 157, 24, hipabi.ptr(R), B, st), 'straps_rot6d_fwd')
        betas.copy_(est[:, 147:])
        smpl.forward_arrays(betas, R, want_joints=False, out_verts=verts)
        silhouette_energy_raw(verts, est, 157, mask, d2, f.sil_opts(), e2, dverts, dcam, None, ws)
        hipabi.check(L.straps_smpl_bwd(C.byref(smpl._model_struct()), hipabi.ptr(betas), hipabi.ptr(R), hipabi.ptr(dverts), None, hipabi.ptr(dbetas),
                                       hipabi.ptr(drot), hipabi.ptr(ws2), B, 0, st), 'straps_smpl_bwd')
        hipabi.check(L.straps_rot6d_bwd(x6, 157, 24, hipabi.ptr(drot), hipabi.ptr(dx6), 144, B, st), 'straps_rot6d_bwd')
        fit_keypoints_raw(f._struct, f.opts(0), est.clone(), est0, targets, conf, None, None, e_kp, g_kp, None, None, None)
        fit_adam_raw(f.opts(), est, g_kp, dcam, dx6, dbetas, e_kp, e2, f.w_in, f.w_out, m, v, energy, i, None, best, best_e, i, i == 0, i < iters)
    return {'est': est, 'm': m, 'v': v, 'energy': energy, 'best': best, 'best_e': best_e, 'terms': torch.cat([e_kp, e2], dim=1), 'R': R}


@pytest.mark.parametrize('B', [1, 3])
def test_call_equals_the_seven_entry_points_and_a_split_call_equals_the_whole(dev, smpl, B):
    est, targets, conf, masks, _ = eval_inputs(dev, B)
    est, targets, conf, sil = est.to(dev), targets.to(dev), conf.to(dev), torch.from_numpy(masks).to(dev)
    keep = [t.clone() for t in (est, targets, conf, sil)]
    f = fitter_for(smpl, 3)
    out = f(*split(est), sil, targets, conf=conf, trace=True)
    hand = by_hand(dev, smpl, f, est, targets, conf, sil, 3)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((est, targets, conf, sil), keep)), 'the inputs are not modified'
    got = torch.cat([out['cam_wp'], out['pose'], out['shape']], dim=1)
    assert same_bits(got, hand['est']) and not same_bits(got, est)
    assert same_bits(out['trace'], hand['energy']) and same_bits(out['energy0'], hand['energy'][:, 0]) and same_bits(out['energy'], hand['energy'][:, 3])
    assert same_bits(out['state']['exp_avg'], hand['m']) and same_bits(out['state']['exp_avg_sq'], hand['v']) and out['state']['step'] == 3
    assert same_bits(torch.cat([out['best'][k] for k in ('cam_wp', 'pose', 'shape')], dim=1), hand['best']) and same_bits(out['best']['energy'], hand['best_e'])
    assert same_bits(out['energy_terms'], hand['terms']) and same_bits(out['pose_rotmats'], hand['R'])
    assert set(out) == {'cam_wp', 'pose', 'shape', 'pose_rotmats', 'energy0', 'energy', 'best', 'joints2D', 'state', 'trace', 'energy_terms'}
    assert same_bits(out['pose_rotmats'], straps_amd.rot6d_to_rotmat(out['pose'].contiguous()).view(B, 24, 3, 3))
    # bool and float silhouettes are the uint8 ones
    assert same_bits(f(*split(est), sil != 0, targets, conf=conf)['pose'], out['pose']) and same_bits(f(*split(est), sil.float() * 0.5, targets, conf=conf)['pose'], out['pose'])
    # two calls of one and two iterations, the state and the prior centre carried over
    one = fitter_for(smpl, 1)(*split(est), sil, targets, conf=conf)
    two = fitter_for(smpl, 2)(one['cam_wp'].contiguous(), one['pose'].contiguous(), one['shape'].contiguous(), sil, targets, conf=conf, prior=split(est), state=one['state'])
    for k in ('cam_wp', 'pose', 'shape', 'energy', 'energy_terms', 'joints2D'):
        assert same_bits(two[k], out[k]), k
    assert same_bits(two['state']['exp_avg'], out['state']['exp_avg']) and same_bits(two['state']['exp_avg_sq'], out['state']['exp_avg_sq']) and two['state']['step'] == 3
    with pytest.raises(RuntimeError, match='silhouettes'):
        f(*split(est), sil[:, :32], targets, conf=conf)


@pytest.mark.parametrize('B', [1, 3])
def test_call_is_capturable(dev, smpl, B):
    est, targets, conf, masks, _ = eval_inputs(dev, B)
    est, targets, conf, sil = est.to(dev), targets.to(dev), conf.to(dev), torch.from_numpy(masks).to(dev)
    f = fitter_for(smpl, 2)
    args = split(est) + (sil, targets)
    eager = f(*args, conf=conf, trace=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = f(*args, conf=conf, trace=True)
    graph.replay()
    torch.cuda.synchronize()
    for k in ('cam_wp', 'pose', 'shape', 'pose_rotmats', 'energy0', 'energy', 'joints2D', 'trace', 'energy_terms'):
        assert same_bits(cap[k], eager[k]), k
    assert same_bits(cap['best']['pose'], eager['best']['pose'])


# ---------------------------------------------------------------- the standard trajectory case ----------------------------------------------------------------
def test_standard_trajectory_case(dev, smpl):
    c = SC.trajectory_case()
    est, sil = c['est'].to(dev), torch.from_numpy(c['masks']).to(dev)
    f = fitter_for(smpl, T['iters'], lr=T['lr'], lambda_pose=T['lambda_pose'], lambda_shape=T['lambda_shape'])
    _, _, t0 = f.evaluate(*split(est), sil)
    out = f(*split(est), sil)
    start, end = (t0[:, 1] + t0[:, 2]).cpu(), (out['energy_terms'][:, 1] + out['energy_terms'][:, 2]).cpu()
    ratio = end / start
    print('standard trajectory case: silhouette energy %s -> %s, ratio %s' % (start.tolist(), end.tolist(), ratio.tolist()))
    assert bool((ratio < 0.5).all()), ratio
    assert bool((out['energy'] < out['energy0']).all()) and bool((out['best']['energy'] <= out['energy']).all())


# ---------------------------------------------------------------- Predictor.refine ----------------------------------------------------------------
def test_predictor_refine_with_a_silhouette_fitter(dev, smpl):
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=straps_amd.synthetic_mean_params(0)).to(dev).eval()
    sil, joints = PC.inputs('a')
    sil, joints = torch.from_numpy(sil[:3].copy()).to(dev), torch.from_numpy(joints[:3]).to(dev)
    sil[2] = 0                                                    # an empty silhouette: invalid, passes through
    pred = straps_amd.Predictor(reg, smpl)
    out = pred(sil, joints)
    f = SilhouetteFitter(smpl, iters=4)
    ref = pred.refine(out, f)
    torch.cuda.synchronize()
    assert set(ref) == set(out) | {'energy0', 'energy', 'energy_terms'}
    assert out['valid'].tolist() == [True, True, False]
    for k in ('cam_wp', 'pose', 'shape'):
        assert same_bits(ref[k][2], out[k][2]) and not same_bits(ref[k][0], out[k][0]), k
    assert float(ref['energy0'][2]) == 0.0 and not bool(ref['energy_terms'][2].any())
    assert bool((ref['energy'][:2] < ref['energy0'][:2]).all())
    # the same as the fitter called by hand on the regressor's silhouette channel
    valid = out['valid']
    target = (out['proxy_rep'][:, 0] != 0) & valid[:, None, None]
    conf = torch.ones(3, 17, device=dev) * valid[:, None].float()
    hand = f(out['cam_wp'].contiguous(), out['pose'].contiguous(), out['shape'].contiguous(), target, out['joints2D_cropped'], conf=conf)
    for k in ('cam_wp', 'pose', 'shape'):
        assert same_bits(ref[k], hand[k]), k
    assert same_bits(ref['energy_terms'], hand['energy_terms'])
    with pytest.raises(ValueError, match='img_wh'):
        pred.refine(out, SilhouetteFitter(smpl, iters=1, img_wh=224))
    # a KeypointFitter: what it returned before -- the fitter called by hand, through the same tail
    kf = KeypointFitter(smpl, iters=5)
    a = pred.refine(out, kf)
    b = kf(out['cam_wp'].contiguous(), out['pose'].contiguous(), out['shape'].contiguous(), out['joints2D_cropped'], conf=conf)
    assert set(a) == set(out) | {'energy0', 'energy'}
    for k in ('cam_wp', 'pose', 'shape', 'energy0', 'energy'):
        assert same_bits(a[k], b[k]), k
    verts, jts = smpl.forward_arrays(a['shape'].contiguous(), a['pose_rotmats'].contiguous())
    assert torch.equal(a['vertices'], verts) and torch.equal(a['joints'], jts)
