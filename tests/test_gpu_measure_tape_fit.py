"""GPU: BodyMeasurer(tape_gradients=True), fit.MeasurementFitter with tape specs and Predictor.refine_shape on the full synthetic model
(csrc/measure_tape_bwd.hip, measure.py, fit.py, predict.py).

The measurer holds the seven tape_measurements() plus the height: tape columns 0..6 (straps_measure_tape / straps_measure_tape_bwd), mesh
column 7 (straps_measure_mesh / straps_measure_mesh_bwd).  evaluate is compared with float64 autograd through the oracle's SMPL forward and
the restatements of tests/tape_grad_cases.py and tests/measure_grad_cases.py, at the bars of test_gpu_measure_fit.py (energy 1e-5 relative,
gradient 1e-4 of its largest entry); the loop must equal its entry points written out by hand, a split call must equal the whole, a captured
graph must replay to the eager bits.  The trajectory test runs the float64 prototype of the fit on the CPU and asks the GPU fit for at least
half of the prototype's relative decrease: the hull of a triangle soup's loose segments makes the trajectory non-smooth (body 1 of the
prototype moves between 0.0082 and 0.0113 over its last 50 iterations).  The measured figures are printed; DESIGN.md section 1 records them."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import measure_cases as MC
import measure_grad_cases as GC
import predict_cases as PC
import straps_amd
import straps_oracle as O
import tape_grad_cases as TG
from smpl_cases import cpu_threads
from straps_amd import hipabi, measure
from straps_amd.fit import NE, MeasurementFitter, fit_adam_raw

pytestmark = pytest.mark.gpu
MODEL = straps_amd.synthetic_smpl_model(0)
MP = straps_amd.synthetic_mean_params(0)
LAMBDA = 1e-3
SPECS = collections.OrderedDict(list(measure.tape_measurements().items()) + [('height', measure.extent((0.0, 1.0, 0.0)))])
M, T = len(SPECS), 7


def _tape_dicts(specs):
    arr, _ = measure.tape_structs(specs, 6890)
    return [{'kind': q.kind, 'anchor': list(q.anchor), 'dir': list(q.dir), 'part_mask': q.part_mask} for q in arr]


MEAS_TAPE = _tape_dicts(list(SPECS.values())[:T])
MEAS_MESH = MC.from_specs(list(SPECS.values())[T:], 6890)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    torch.set_num_threads(cpu_threads())
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def smpl(dev):
    return straps_amd.SMPL(MODEL, batch_size=1).to(dev)


@pytest.fixture(scope='module')
def measurer(dev, smpl):
    return straps_amd.BodyMeasurer.from_smpl(smpl, SPECS, tape_gradients=True).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- float64 references ----------------------------------------------------------------------------------------------------------------
def tpose64(betas):
    t = lambda k: torch.from_numpy(np.asarray(MODEL[k], np.float64))
    v = t('v_template')[None] + torch.einsum('bl,mkl->bmk', betas, t('shapedirs'))
    return v, torch.einsum('bik,ji->bjk', v, t('J_regressor'))


def energy64(betas, betas0, targets, weights, forward=tpose64):
    """the objective of straps_measure_residual in float64 torch on the fp64 mesh -> (energy [B], values [B,M])"""
    verts, joints = forward(betas)
    rows = []
    for b in range(betas.shape[0]):
        rows.append(torch.stack(TG.values_torch(verts[b], joints[b, :24], MODEL['faces'], MODEL['face_parts'], MEAS_TAPE)
                                + GC.values_torch(verts[b], joints[b, :24], MODEL['faces'], MODEL['face_parts'], MEAS_MESH)))
    vals = torch.stack(rows)
    t, w = torch.from_numpy(targets.astype(np.float64)), torch.from_numpy(weights.astype(np.float64))
    known = torch.isfinite(t) & (t != 0) & torch.isfinite(w) & (w > 0)
    r = torch.where(known, vals / torch.where(known, t, torch.ones_like(t)) - 1.0, torch.zeros_like(vals))
    e = (torch.where(known, w, torch.zeros_like(w)) * r * r).sum(1) + LAMBDA * ((betas - betas0) ** 2).sum(1)
    return e, vals


def case(B, seed=0):
    """betas, prior centre, targets (the measurements of other bodies, one tape column unknown everywhere, one in body 0) and weights"""
    rng = np.random.RandomState(700 + seed)
    betas = rng.uniform(-1.5, 1.5, (B, 10)).astype(np.float32)
    prior = (betas + rng.uniform(-0.5, 0.5, (B, 10))).astype(np.float32)
    with torch.no_grad():
        _, vals = energy64(torch.from_numpy(rng.uniform(-2, 2, (B, 10))), torch.zeros(B, 10, dtype=torch.float64), np.ones((B, M)), np.ones((B, M)))
    targets = vals.numpy().astype(np.float32)
    targets[:, 4] = np.nan
    targets[0, 1] = 0.0
    weights = rng.uniform(0.5, 2.0, (B, M)).astype(np.float32)
    weights[:, 5] = 0.0
    return betas, prior, targets, weights


# ---- the autograd surface ---------------------------------------------------------------------------------------------------------------
def test_body_measurer_with_tape_gradients(dev, smpl, measurer):
    b = MC.bodies(betas_seed=1)
    v = torch.from_numpy(b['verts']).to(dev).requires_grad_(True)
    j = torch.zeros(3, 90, 3, device=dev)
    j[:, :24] = torch.from_numpy(b['joints']).to(dev)
    j.requires_grad_(True)
    plain = measurer(v, j)
    assert not plain['values'].requires_grad
    res = measurer(v, j, differentiable=True)
    assert res['values'].requires_grad and same_bits(res['values'], plain['values']) and list(res) == list(plain) == ['values'] + list(SPECS)
    dvalues = torch.from_numpy(GC.random_dout(3, M, 8)).to(dev)
    (res['values'] * dvalues).sum().backward()
    dv, dj = measurer.measure_grad(v, j, dvalues)
    assert same_bits(v.grad, dv) and same_bits(j.grad, dj) and dj.shape == (3, 90, 3) and not dj[:, 24:].any() and dj[:, :24].any()
    # against the oracle: the tape columns' and the height's gradients, added
    d = dvalues.cpu().numpy()
    _, want_v, want_p, S_v, S_p = TG.oracle_grad(b['verts'], b['joints'], b['faces'], b['face_parts'], MEAS_TAPE, d[:, :T])
    mv, mp, Sm_v, Sm_p = GC.oracle_grad(b['verts'], b['joints'], b['faces'], b['face_parts'], MEAS_MESH, d[:, T:])
    # two roundings to float (straps_measure_mesh_bwd's output, then the sum)
    for got, tape_part, mesh_part, S in ((dv.cpu().numpy(), want_v, mv, S_v + Sm_v), (dj[:, :24].cpu().numpy(), want_p, mp, S_p + Sm_p)):
        assert (np.abs(got - (tape_part + mesh_part)) <= 2.0 ** -23 * (np.abs(tape_part + mesh_part) + np.abs(mesh_part)) + 1e-10 * S).all()
    # each column's own gradient: a mixed measurer against measurers of one sort
    tape_only = straps_amd.BodyMeasurer.from_smpl(smpl, list(SPECS.items())[:T], tape_gradients=True).to(dev)
    mesh_only = straps_amd.BodyMeasurer.from_smpl(smpl, list(SPECS.items())[T:]).to(dev)
    only_tape, only_mesh = dvalues.clone(), dvalues.clone()
    only_tape[:, T:] = 0
    only_mesh[:, :T] = 0
    a, aj = measurer.measure_grad(v, j, only_tape)
    t, tj = tape_only.measure_grad(v, j, dvalues[:, :T].contiguous())
    assert torch.equal(a, t) and torch.equal(aj, tj) and bool(t.any())
    a, aj = measurer.measure_grad(v, j, only_mesh)
    m, mj = mesh_only.measure_grad(v, j, dvalues[:, T:].contiguous())
    assert torch.equal(a, m) and mj is not None and torch.equal(aj, mj) and int((m != 0).sum()) == 2 * int((dvalues[:, T] != 0).sum()) > 0
    v.grad = None
    measurer(v, j, differentiable=True)['waist_tape_girth'].sum().backward()
    one = torch.zeros(3, T, device=dev)
    one[:, 1] = 1.0
    assert same_bits(v.grad, tape_only.measure_grad(v, j, one)[0]) and 3 * 6 <= int((v.grad != 0).any(2).sum()) <= 3 * 60      # sparse: a few dozen vertices per body
    # without the flag every refusal is the one it was
    closed = straps_amd.BodyMeasurer.from_smpl(smpl, SPECS).to(dev)
    with pytest.raises(RuntimeError, match='tape'):
        closed(v, j, differentiable=True)
    with pytest.raises(RuntimeError, match='tape'):
        closed.measure_grad(v, j, dvalues)
    with pytest.raises(ValueError, match='tape'):
        MeasurementFitter(smpl, closed)


# ---- evaluate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
def test_evaluate_vs_float64(dev, smpl, measurer, B):
    betas, prior, targets, weights = case(B)
    eye = torch.eye(3, dtype=torch.float64).expand(B, 24, 3, 3)

    def oracle_forward(b):
        v, j = O.smpl_forward(MODEL, b, rotmats=eye, dtype=torch.float64)
        return v, j[:, :24]
    b64 = torch.from_numpy(betas.astype(np.float64)).requires_grad_(True)
    want_e, want_vals = energy64(b64, torch.from_numpy(prior.astype(np.float64)), targets, weights, forward=oracle_forward)
    (want_g,) = torch.autograd.grad(want_e.sum(), b64)
    fitter = MeasurementFitter(smpl, measurer, lambda_shape=LAMBDA)
    to = lambda a: torch.from_numpy(a).to(dev)
    e, g, vals = fitter.evaluate(to(betas), to(targets), to(weights), to(prior))
    assert e.shape == (B,) and g.shape == (B, 10) and vals.shape == (B, M)
    e, g, vals = e.cpu().double(), g.cpu().double(), vals.cpu().double()
    err_e = float(((e - want_e.detach()).abs() / want_e.detach()).max())
    err_g = float(((g - want_g).abs().max(1).values / want_g.abs().max(1).values).max())
    err_v = float(((vals - want_vals.detach()).abs() / want_vals.detach().abs()).max())
    print('B %d: energy %.3g relative, gradient %.3g of the largest entry, values %.3g relative' % (B, err_e, err_g, err_v))
    assert err_e <= 1e-5 and err_g <= 1e-4


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
def _by_hand(dev, smpl, measurer, betas, targets, weights, prior, iters, lr):
    """the entry points of every iteration, called one by one on buffers of the test"""
    L, st, B = hipabi.lib(), hipabi.stream_ptr(), betas.shape[0]
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    zeros = torch.zeros(B, 147, device=dev)
    est, est0 = torch.cat([zeros, betas], 1).contiguous(), torch.cat([zeros, prior], 1).contiguous()
    R = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    P = measurer.needs_joints
    b, verts, joints, points = f(B, 10), f(B, 6890, 3), f(B, 90, 3), f(B, P, 3)
    values, dvalues, e, g, dverts, djoints = f(B, M), f(B, M), f(B), f(B, NE), f(B, 6890, 3), torch.zeros(B, 90, 3, device=dev)
    mesh_values, tape_values = f(B, M - T), f(B, T)
    dbetas, drot = f(B, 10), f(B, 24, 3, 3)
    ws = torch.empty(L.straps_measure_workspace_bytes(B, 6890, 13776, M - T) // 8, device=dev, dtype=torch.float64)
    wsg = torch.empty(L.straps_measure_bwd_workspace_bytes(B, 6890, 13776, M - T) // 8, device=dev, dtype=torch.float64)
    wst = torch.empty(L.straps_measure_tape_workspace_bytes(B, 13776, T, 0) // 8, device=dev, dtype=torch.float64)
    wstg = torch.empty(L.straps_measure_tape_bwd_workspace_bytes(B, 6890, 13776, T, 0) // 8, device=dev, dtype=torch.float64)
    ws2 = f(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)
    m, v = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev)
    energy, best, best_e = f(B, iters + 1), f(B, NE), f(B)
    opts = hipabi.FitOptsStruct(iters, 0, lr, lr, lr, 0.9, 0.999, 1e-8, 0.0, 0.0, LAMBDA, 0.0)
    arr = measure.measure_structs(list(SPECS.values())[T:], 6890)[0]
    tarr = measure.tape_structs(list(SPECS.values())[:T], 6890)[0]
    p = hipabi.ptr
    for i in range(iters + 1):
        b.copy_(est[:, 147:])
        smpl.forward_arrays(b, R, out_verts=verts, out_joints=joints)
        points.copy_(joints[:, :P])
        hipabi.check(L.straps_measure_mesh(p(verts), p(points), p(measurer.faces), p(measurer.face_parts), arr, p(mesh_values), p(ws), B, 6890, P, 13776, M - T, st),
                     'straps_measure_mesh')
        hipabi.check(L.straps_measure_tape(p(verts), p(points), p(measurer.faces), p(measurer.face_parts), tarr, p(tape_values), None, p(wst), B, 6890, P, 13776, T, 0, st),
                     'straps_measure_tape')
        values[:, :T], values[:, T:] = tape_values, mesh_values
        hipabi.check(L.straps_measure_residual(p(values), p(targets), p(weights), p(est), p(est0), LAMBDA, p(e), p(dvalues), p(g), B, M, st), 'straps_measure_residual')
        d_mesh, d_tape = dvalues[:, T:].contiguous(), dvalues[:, :T].contiguous()
        hipabi.check(L.straps_measure_mesh_bwd(p(verts), p(points), p(measurer.faces), p(measurer.face_parts), p(measurer.vf_offsets), p(measurer.vf_faces), arr,
                                               p(d_mesh), p(dverts), p(djoints), p(wsg), B, 6890, P, 90, 13776, M - T, st), 'straps_measure_mesh_bwd')
        hipabi.check(L.straps_measure_tape_bwd(p(verts), p(points), p(measurer.faces), p(measurer.face_parts), p(measurer.vf_offsets), p(measurer.vf_faces), tarr,
                                               p(d_tape), p(dverts), p(djoints), None, None, p(wstg), B, 6890, P, 90, 13776, T, 0, 1, st), 'straps_measure_tape_bwd')
        hipabi.check(L.straps_smpl_bwd(C.byref(smpl._model_struct()), p(b), p(R), p(dverts), p(djoints), p(dbetas), p(drot), p(ws2), B, 0, st), 'straps_smpl_bwd')
        fit_adam_raw(opts, est, g, None, None, dbetas, e, None, 0.0, 0.0, m, v, energy, i, None, best, best_e, i, i == 0, i < iters)
    return est, values, energy, best, best_e, m, v, djoints


def test_call_equals_the_entry_points_by_hand_and_splits(dev, smpl, measurer):
    B, iters, lr = 3, 4, 0.05
    betas, prior, targets, weights = (torch.from_numpy(a).to(dev) for a in case(B, seed=1))
    keep = [t.clone() for t in (betas, prior, targets, weights)]
    fitter = MeasurementFitter(smpl, measurer, iters=iters, lr=lr, lambda_shape=LAMBDA)
    out = fitter(betas, targets, weights, prior, trace=True)
    assert list(out) == ['shape', 'values', 'energy0', 'energy', 'best', 'state', 'trace']
    assert all(same_bits(a, b) for a, b in zip((betas, prior, targets, weights), keep)), 'an input was modified'
    est, values, energy, best, best_e, m, v, djoints = _by_hand(dev, smpl, measurer, betas, targets, weights, prior, iters, lr)
    assert same_bits(out['shape'], est[:, 147:]) and same_bits(out['values'], values) and same_bits(out['trace'], energy)
    assert same_bits(out['energy0'], energy[:, 0]) and same_bits(out['energy'], energy[:, iters])
    assert same_bits(out['best']['shape'], best[:, 147:]) and same_bits(out['best']['energy'], best_e)
    assert same_bits(out['state']['exp_avg'][:, 147:], m[:, 147:]) and same_bits(out['state']['exp_avg_sq'][:, 147:], v[:, 147:]) and out['state']['step'] == iters
    assert not djoints[:, measurer.needs_joints:].any() and djoints[:, :measurer.needs_joints].any()
    assert bool((out['best']['energy'] <= out['energy']).all()) and bool((out['energy'] < out['energy0']).any()) and not same_bits(out['shape'], betas)
    # a call split in two, state and prior carried over
    half = MeasurementFitter(smpl, measurer, iters=iters // 2, lr=lr, lambda_shape=LAMBDA)
    first = half(betas, targets, weights, prior)
    second = half(first['shape'], targets, weights, prior, state=first['state'])
    assert same_bits(second['shape'], out['shape']) and same_bits(second['energy'], out['energy']) and same_bits(first['energy0'], out['energy0'])
    assert same_bits(second['state']['exp_avg'], out['state']['exp_avg']) and second['state']['step'] == iters
    # targets by name; a measurer of tape specs alone (no straps_measure_mesh call at all)
    named = fitter(betas, {'waist_tape_girth': targets[:, 1], 'height': 1.7}, prior=prior)
    t2 = torch.full_like(targets, float('nan'))
    t2[:, 1], t2[:, 7] = targets[:, 1], 1.7
    assert same_bits(named['shape'], fitter(betas, t2, prior=prior)['shape'])
    tape_only = straps_amd.BodyMeasurer.from_smpl(smpl, measure.tape_measurements(), tape_gradients=True).to(dev)
    alone = MeasurementFitter(smpl, tape_only, iters=iters, lr=lr, lambda_shape=LAMBDA)(betas, targets[:, :T].contiguous(), weights[:, :T].contiguous(), prior)
    t3 = targets.clone()
    t3[:, T:] = float('nan')
    assert same_bits(alone['shape'], fitter(betas, t3, weights, prior)['shape']) and bool((alone['energy'] < alone['energy0']).any())


def test_call_is_capturable(dev, smpl, measurer):
    B = 2
    betas, prior, targets, weights = (torch.from_numpy(a).to(dev) for a in case(B, seed=2))
    fitter = MeasurementFitter(smpl, measurer, iters=3, lambda_shape=LAMBDA)
    eager = fitter(betas, targets, weights, prior)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fitter(betas, targets, weights, prior)
    for _ in range(2):
        for t in (out['shape'], out['values'], out['energy'], out['best']['shape']):
            t.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert all(same_bits(out[k], eager[k]) for k in ('shape', 'values', 'energy0', 'energy')) and same_bits(out['best']['shape'], eager['best']['shape'])


# ---- trajectory ------------------------------------------------------------------------------------------------------------------------
def test_trajectory_against_the_float64_prototype(dev, smpl, measurer):
    """targets: the seven tape girths and the height of two bodies with betas from RandomState(5).uniform(-2, 2); start at zero; lr 0.05,
    lambda 1e-3, 100 iterations"""
    B, iters, lr = 2, 100, 0.05
    true = torch.from_numpy(np.random.RandomState(5).uniform(-2, 2, (B, 10)))
    ones = np.ones((B, M))
    with torch.no_grad():
        _, tv = energy64(true, true, ones, ones)
    targets = tv.numpy().astype(np.float32)
    zero = torch.zeros(B, 10, dtype=torch.float64)
    b64 = zero.clone().requires_grad_(True)
    opt = torch.optim.Adam([b64], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    trace = []
    for i in range(iters + 1):
        opt.zero_grad()
        e, _ = energy64(b64, zero, targets, ones)
        trace.append(e.detach().clone())
        if i < iters:
            e.sum().backward()
            opt.step()
    r = (trace[-1] / trace[0]).numpy()
    fitter = MeasurementFitter(smpl, measurer, iters=iters, lr=lr, lambda_shape=LAMBDA)
    out = fitter(torch.zeros(B, 10, device=dev), torch.from_numpy(targets).to(dev))
    e0, e1, best = out['energy0'].cpu().double().numpy(), out['energy'].cpu().double().numpy(), out['best']['energy'].cpu().double().numpy()
    print('float64 prototype: E_0 %s, E_end / E_0 %s; GPU: E_0 %s, E_end / E_0 %s, best / E_0 %s' % (trace[0].numpy(), r, e0, e1 / e0, best / e0))
    assert (r < 1).all(), 'the prototype itself does not descend'
    assert (np.abs(e0 - trace[0].numpy()) <= 1e-5 * trace[0].numpy()).all()
    assert (e1 / e0 <= (1 + r) / 2).all()
    assert (best <= e1).all()


# ---- Predictor.refine_shape -------------------------------------------------------------------------------------------------------------
def test_predictor_refine_shape_with_tape_targets(dev, smpl, measurer):
    B = 3
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP).to(dev).eval()
    sil, joints = PC.inputs('a')
    pred = straps_amd.Predictor(reg, smpl)
    sil, joints = torch.from_numpy(sil[:B].copy()).to(dev), torch.from_numpy(joints[:B].copy()).to(dev)
    sil[1] = 0                                                   # an invalid sample
    out = pred(sil, joints)
    assert out['valid'].tolist() == [True, False, True]
    kept = {k: v.clone() for k, v in out.items()}
    fitter = MeasurementFitter(smpl, measurer, iters=5, lambda_shape=LAMBDA)
    targets = pred.measure(out, measurer)['values'] * 1.1
    weights = torch.ones(B, M, device=dev)
    weights[:, 5:] = 0.5
    res = pred.refine_shape(out, fitter, targets, weights)
    assert set(res) == set(out) | {'energy0', 'energy', 'measurements'}
    assert all(same_bits(out[k].float(), kept[k].float()) for k in kept), '`out` was changed'
    w = weights.clone()
    w[1] = 0
    fit = fitter(out['shape'].contiguous(), targets, weights=w)
    assert same_bits(res['shape'], fit['shape']) and same_bits(res['energy'], fit['energy']) and same_bits(res['energy0'], fit['energy0'])
    assert same_bits(res['measurements'], fit['values'])
    assert same_bits(res['shape'][1], out['shape'][1]) and float(res['energy0'][1]) == 0 and float(res['energy'][1]) == 0      # the invalid row comes back as it went in
    assert not same_bits(res['shape'][0], out['shape'][0]) and bool((res['energy'][[0, 2]] < res['energy0'][[0, 2]]).all())
    eye = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    tverts, _ = smpl.forward_arrays(res['shape'].contiguous(), eye)
    assert same_bits(res['reposed_vertices'], tverts) and same_bits(pred.measure(res, measurer)['values'], res['measurements'])
    named = pred.refine_shape(out, fitter, {'chest_tape_girth': 1.0, 'height': 1.8})
    assert bool((named['energy'][[0, 2]] < named['energy0'][[0, 2]]).all()) and same_bits(named['shape'][1], out['shape'][1])
