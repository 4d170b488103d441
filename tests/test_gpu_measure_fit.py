"""GPU: straps_measure_residual, fit.MeasurementFitter, BodyMeasurer.forward(differentiable=True) and Predictor.refine_shape on the full synthetic
model (csrc/measure_bwd.hip, fit.py, measure.py, predict.py).

The residual head is compared with a float64 restatement (2^-22 of the sum of magnitudes: fp32 sums of at most 43 terms); evaluate with float64
autograd through the oracle's SMPL forward and the measurement restatement of tests/measure_grad_cases.py, at the bars of
test_gpu_fit_silhouette.py::test_evaluate_vs_float64 for the same SMPL-backward chain (energy 1e-5 relative, gradient 1e-4 of its largest
entry); the loop must equal the six entry points written out by hand, a split call must equal the whole, a captured graph must replay to the
eager bits.  The trajectory test runs the float64 prototype of the fit on the CPU (Adam on the same objective) and asks the GPU fit for at
least half of the prototype's relative decrease: the section girths of a triangle soup make the trajectory non-smooth.
Measured on MI355X: evaluate -- energy 7.3e-6 relative, gradient 5.3e-5 of the largest entry (the values 2.0e-6 relative); trajectory ratios
0.0647 and 0.1980 (float64 prototype: 0.0645 and 0.1980, E_0 0.2892 and 0.3632).  DESIGN.md section 1 has the same figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import measure_cases as MC
import measure_grad_cases as GC
import predict_cases as PC
import straps_amd
import straps_oracle as O
from redzone import Zone
from smpl_cases import cpu_threads
from straps_amd import hipabi, measure
from straps_amd.fit import NE, MeasurementFitter, fit_adam_raw

pytestmark = pytest.mark.gpu
MODEL = straps_amd.synthetic_smpl_model(0)
MP = straps_amd.synthetic_mean_params(0)
LAMBDA = 1e-3


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
    return straps_amd.BodyMeasurer.from_smpl(smpl).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


MEAS = MC.from_specs(list(measure.default_measurements().values()), 6890)
M = len(MEAS)


# ---- float64 references ----------------------------------------------------------------------------------------------------------------
def tpose64(betas):
    """betas [B,10] float64 torch -> (verts [B,6890,3], joints [B,24,3]): with identity rotations the pose blend vanishes and every skinning
    transform is the identity, so the mesh is the shaped template to the rounding of the fp32 weights (asserted against the oracle's SMPL forward in test_evaluate_vs_float64)"""
    t = lambda k: torch.from_numpy(np.asarray(MODEL[k], np.float64))
    v = t('v_template')[None] + torch.einsum('bl,mkl->bmk', betas, t('shapedirs'))
    return v, torch.einsum('bik,ji->bjk', v, t('J_regressor'))


def energy64(betas, betas0, targets, weights, forward=tpose64):
    """the objective of straps_measure_residual in float64 torch on the fp64 mesh -> (energy [B], values [B,M])"""
    verts, joints = forward(betas)
    vals = torch.stack([torch.stack(GC.values_torch(verts[b], joints[b, :24], MODEL['faces'], MODEL['face_parts'], MEAS)) for b in range(betas.shape[0])])
    t, w = torch.from_numpy(targets.astype(np.float64)), torch.from_numpy(weights.astype(np.float64))
    known = torch.isfinite(t) & (t != 0) & torch.isfinite(w) & (w > 0)
    r = torch.where(known, vals / torch.where(known, t, torch.ones_like(t)) - 1.0, torch.zeros_like(vals))
    e = (torch.where(known, w, torch.zeros_like(w)) * r * r).sum(1) + LAMBDA * ((betas - betas0) ** 2).sum(1)
    return e, vals


def case(B, seed=0):
    """betas, prior centre, targets (the measurements of other bodies, two columns unknown) and weights"""
    rng = np.random.RandomState(600 + seed)
    betas = rng.uniform(-1.5, 1.5, (B, 10)).astype(np.float32)
    prior = (betas + rng.uniform(-0.5, 0.5, (B, 10))).astype(np.float32)
    with torch.no_grad():
        _, vals = energy64(torch.from_numpy(rng.uniform(-2, 2, (B, 10))), torch.zeros(B, 10, dtype=torch.float64), np.ones((B, M)), np.ones((B, M)))
    targets = vals.numpy().astype(np.float32)
    targets[:, 4] = np.nan
    targets[0, 7] = 0.0
    weights = rng.uniform(0.5, 2.0, (B, M)).astype(np.float32)
    weights[:, 11] = 0.0
    return betas, prior, targets, weights


# ---- straps_measure_residual -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 257])
@pytest.mark.parametrize('with_weights', [True, False])
def test_residual_head_vs_float64(dev, B, with_weights):
    rng = np.random.RandomState(B)
    n_meas = 1 if B == 1 else (32 if B == 3 else 15)
    values = rng.uniform(0.2, 2.0, (B, n_meas)).astype(np.float32)
    targets = (values * rng.uniform(0.8, 1.25, (B, n_meas))).astype(np.float32)
    weights = rng.uniform(0.1, 3.0, (B, n_meas)).astype(np.float32)
    est, est0 = rng.uniform(-2, 2, (B, NE)).astype(np.float32), rng.uniform(-2, 2, (B, NE)).astype(np.float32)
    unknown = np.zeros((B, n_meas), bool)
    if n_meas > 1:
        targets[:, 1], targets[-1, 2], targets[0, 3], targets[-1, 4] = np.nan, 0.0, np.inf, -0.0
        weights[:, 5], weights[0, 6], weights[-1, 7], weights[0, 8] = 0.0, -1.0, np.nan, np.inf
        unknown[:, 1], unknown[-1, 2], unknown[0, 3], unknown[-1, 4] = True, True, True, True
        if with_weights:
            unknown[:, 5], unknown[0, 6], unknown[-1, 7], unknown[0, 8] = True, True, True, True
        values[unknown] = np.nan                                 # the value of an unknown column is not evaluated
    z = Zone(dev)
    e, dv, g = z.guarded((B,), name='energy'), z.guarded((B, n_meas), name='dvalues'), z.guarded((B, NE), name='g')
    put = lambda a: z.at_end(torch.from_numpy(a))
    hipabi.check(hipabi.lib().straps_measure_residual(hipabi.ptr(put(values)), hipabi.ptr(put(targets)), hipabi.ptr(put(weights)) if with_weights else None,
                                                      hipabi.ptr(put(est)), hipabi.ptr(put(est0)), LAMBDA, hipabi.ptr(e), hipabi.ptr(dv), hipabi.ptr(g), B, n_meas,
                                                      hipabi.stream_ptr()), 'straps_measure_residual')
    z.check()
    e, dv, g = e.cpu().numpy(), dv.cpu().numpy(), g.cpu().numpy()
    w = np.where(unknown, 0.0, weights.astype(np.float64) if with_weights else 1.0)
    t = np.where(unknown, 1.0, targets.astype(np.float64))
    r = np.where(unknown, 0.0, np.where(unknown, 1.0, values.astype(np.float64)) / t - 1.0)
    d = est[:, 147:].astype(np.float64) - est0[:, 147:].astype(np.float64)
    want_e = (w * r * r).sum(1) + LAMBDA * (d * d).sum(1)
    # the sum of magnitudes: r = value / target - 1 cancels, so a term w r^2 carries the rounding of w (|value / target| + 1)^2; likewise the prior
    mag_e = (w * (np.abs(r + 1.0) + 1.0) ** 2).sum(1) + LAMBDA * ((np.abs(est[:, 147:]) + np.abs(est0[:, 147:])).astype(np.float64) ** 2).sum(1)
    assert (np.abs(e - want_e) <= 2.0 ** -22 * mag_e).all() and (want_e > 0).all()
    want_dv = 2 * w * r / t
    # one value: the magnitudes are |value / target| and 1 (the subtraction cancels), times 2 w / |target|
    assert (np.abs(dv - want_dv) <= 2.0 ** -22 * (2 * w / np.abs(t)) * (np.abs(r + 1.0) + 1.0)).all()
    assert not dv[unknown].any() and not np.signbit(dv[unknown]).any() and (dv[~unknown] != 0).any()
    assert not g[:, :147].any() and not np.signbit(g[:, :147]).any()
    assert (np.abs(g[:, 147:] - 2 * LAMBDA * d) <= 2.0 ** -22 * 2 * LAMBDA * (np.abs(est[:, 147:]) + np.abs(est0[:, 147:]))).all()


def test_residual_argument_errors():
    L = hipabi.load()
    P = C.c_void_p(4096)

    def call(values=P, targets=P, est=P, est0=P, lam=1e-3, e=P, dv=P, g=P, batch=2, n_meas=3):
        return L.straps_measure_residual(values, targets, None, est, est0, lam, e, dv, g, batch, n_meas, None), L.straps_last_error().decode()
    for kw, word in ((dict(values=None), '`values`'), (dict(targets=None), '`targets`'), (dict(est=None), '`est`'), (dict(est0=None), '`est0`'), (dict(e=None), '`energy`'),
                     (dict(dv=None), '`dvalues`'), (dict(g=None), '`g`'), (dict(batch=0), '`batch`'), (dict(n_meas=0), '`n_meas`'), (dict(n_meas=33), '`n_meas`'),
                     (dict(lam=-1.0), '`lambda_shape`'), (dict(lam=float('nan')), '`lambda_shape`')):
        rc, err = call(**kw)
        assert rc == 1 and word in err and 'straps_measure_residual' in err, (kw, rc, err)


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
    with torch.no_grad():
        v_lin, j_lin = tpose64(b64)
        v_orc, j_orc = oracle_forward(b64)
        # the T-pose is the shaped template, up to the sum of a vertex's fp32 skinning weights (1 within their rounding), which scales it
        assert float((v_lin - v_orc).abs().max()) < 1e-6 and float((j_lin - j_orc).abs().max()) < 1e-12
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
def _by_hand(dev, smpl, measurer, betas, targets, weights, prior, iters, lr, camp):
    """the six entry points of every iteration, called one by one on buffers of the test; cam and pose columns hold `camp`"""
    L, st, B = hipabi.lib(), hipabi.stream_ptr(), betas.shape[0]
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    est = torch.cat([camp, betas], 1).contiguous()
    est0 = torch.cat([camp, prior], 1).contiguous()
    R = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    b, verts, joints, points = f(B, 10), f(B, 6890, 3), f(B, 90, 3), f(B, measurer.needs_joints, 3)
    values, dvalues, e, g, dverts, djoints = f(B, M), f(B, M), f(B), f(B, NE), f(B, 6890, 3), torch.zeros(B, 90, 3, device=dev)
    dbetas, drot = f(B, 10), f(B, 24, 3, 3)
    ws = torch.empty(L.straps_measure_workspace_bytes(B, 6890, 13776, M) // 8, device=dev, dtype=torch.float64)
    wsg = torch.empty(L.straps_measure_bwd_workspace_bytes(B, 6890, 13776, M) // 8, device=dev, dtype=torch.float64)
    ws2 = f(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)
    m, v = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev)
    energy, best, best_e = f(B, iters + 1), f(B, NE), f(B)
    opts = hipabi.FitOptsStruct(iters, 0, lr, lr, lr, 0.9, 0.999, 1e-8, 0.0, 0.0, LAMBDA, 0.0)
    arr = measure.measure_structs(list(measurer.specs), 6890)[0]
    p = hipabi.ptr
    for i in range(iters + 1):
        b.copy_(est[:, 147:])
        smpl.forward_arrays(b, R, out_verts=verts, out_joints=joints)
        points.copy_(joints[:, :measurer.needs_joints])
        hipabi.check(L.straps_measure_mesh(p(verts), p(points), p(measurer.faces), p(measurer.face_parts), arr, p(values), p(ws), B, 6890, measurer.needs_joints, 13776, M,
                                           st), 'straps_measure_mesh')
        hipabi.check(L.straps_measure_residual(p(values), p(targets), p(weights), p(est), p(est0), LAMBDA, p(e), p(dvalues), p(g), B, M, st), 'straps_measure_residual')
        hipabi.check(L.straps_measure_mesh_bwd(p(verts), p(points), p(measurer.faces), p(measurer.face_parts), p(measurer.vf_offsets), p(measurer.vf_faces), arr,
                                               p(dvalues), p(dverts), p(djoints), p(wsg), B, 6890, measurer.needs_joints, 90, 13776, M, st), 'straps_measure_mesh_bwd')
        hipabi.check(L.straps_smpl_bwd(C.byref(smpl._model_struct()), p(b), p(R), p(dverts), p(djoints), p(dbetas), p(drot), p(ws2), B, 0, st), 'straps_smpl_bwd')
        fit_adam_raw(opts, est, g, None, None, dbetas, e, None, 0.0, 0.0, m, v, energy, i, None, best, best_e, i, i == 0, i < iters)
    return est, values, energy, best, best_e, m, v, djoints


def test_call_equals_the_entry_points_by_hand_and_splits(dev, smpl, measurer):
    B, iters, lr = 3, 4, 0.05
    betas, prior, targets, weights = (torch.from_numpy(a).to(dev) for a in case(B, seed=1))
    keep = [t.clone() for t in (betas, prior, targets, weights)]
    fitter = MeasurementFitter(smpl, measurer, iters=iters, lr=lr, lambda_shape=LAMBDA)
    out = fitter(betas, targets, weights, prior, trace=True)
    assert list(out) == ['shape', 'values', 'energy0', 'energy', 'best', 'state', 'trace'] and 'trace' not in fitter(betas, targets, weights, prior)
    assert all(same_bits(a, b) for a, b in zip((betas, prior, targets, weights), keep)), 'an input was modified'
    # by hand, with zeros in the cam and pose columns (what the fitter holds there) and with arbitrary values: the shape trajectory is the same bits
    # and the cam and pose columns come back as they went in
    for camp in (torch.zeros(B, 147, device=dev), torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (B, 147)).astype(np.float32)).to(dev)):
        est, values, energy, best, best_e, m, v, djoints = _by_hand(dev, smpl, measurer, betas, targets, weights, prior, iters, lr, camp)
        assert same_bits(est[:, :147], camp) and same_bits(best[:, :147], camp), 'cam and pose columns changed'
        assert not m[:, :147].any() and not v[:, :147].any()
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
    # targets by name: absent names are unknown
    named = fitter(betas, {'height': targets[:, 0], 'chest_girth': 1.0}, prior=prior)
    t2 = torch.full_like(targets, float('nan'))
    t2[:, 0], t2[:, 3] = targets[:, 0], 1.0
    assert same_bits(named['shape'], fitter(betas, t2, prior=prior)['shape'])
    with pytest.raises(ValueError, match='no measurement'):
        fitter(betas, {'hat_size': 1.0})
    with pytest.raises(ValueError, match='tape'):
        MeasurementFitter(smpl, straps_amd.BodyMeasurer.from_smpl(smpl, measure.tape_measurements()).to(dev))


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
    """targets: the measurements of two bodies with betas from RandomState(5).uniform(-2, 2); start at zero; lr 0.05, lambda 1e-3, 100 iterations"""
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


# ---- the autograd surface ---------------------------------------------------------------------------------------------------------------
def test_body_measurer_differentiable(dev, smpl, measurer):
    b = MC.bodies(betas_seed=1)
    v = torch.from_numpy(b['verts']).to(dev).requires_grad_(True)
    j = torch.zeros(3, 90, 3, device=dev)
    j[:, :24] = torch.from_numpy(b['joints']).to(dev)
    j.requires_grad_(True)
    plain = measurer(v, j)
    assert not plain['values'].requires_grad
    res = measurer(v, j, differentiable=True)
    assert res['values'].requires_grad and same_bits(res['values'], plain['values']) and list(res) == list(plain)
    dvalues = torch.from_numpy(GC.random_dout(3, M, 8)).to(dev)
    (res['values'] * dvalues).sum().backward()
    dv, dj = measurer.measure_grad(v, j, dvalues)
    assert same_bits(v.grad, dv) and same_bits(j.grad, dj) and dj.shape == (3, 90, 3) and not dj[:, 24:].any() and dj[:, :24].any()
    # a named column carries its own gradient; vertex anchors only need no joints
    v.grad = None
    measurer(v, j, differentiable=True)['height'].sum().backward()
    assert int((v.grad != 0).sum()) == 2 * 3      # the top and the bottom vertex of every body, their y
    own = straps_amd.BodyMeasurer(b['faces'], None, {'vol': measure.volume(about=5), 'ring': measure.girth(4000, (0, 1, 0))}, num_vertices=6890).to(dev)
    dv, dj = own.measure_grad(v, None, torch.ones(3, 2, device=dev))
    assert dj is None and dv.shape == (3, 6890, 3) and bool(dv.any())
    # tape specs have no gradient
    tape = straps_amd.BodyMeasurer.from_smpl(smpl, dict(measure.tape_measurements(), height=measure.extent((0, 1, 0)))).to(dev)
    with pytest.raises(RuntimeError, match='tape'):
        tape(v, j, differentiable=True)
    dvalues = torch.zeros(3, 8, device=dev)
    dvalues[:, 7] = 1.0
    dv, _ = tape.measure_grad(v, j, dvalues)
    assert int((dv != 0).sum()) == 6
    dvalues[1, 2] = 0.5
    with pytest.raises(RuntimeError, match='tape'):
        tape.measure_grad(v, j, dvalues)
    with pytest.raises(RuntimeError, match='built for'):
        straps_amd.BodyMeasurer(b['faces'], b['face_parts'], num_vertices=7000).to(dev).measure_grad(v, j, torch.zeros(3, 15, device=dev))


# ---- Predictor.refine_shape -------------------------------------------------------------------------------------------------------------
def test_predictor_refine_shape(dev, smpl, measurer):
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
    assert same_bits(res['shape'][1], out['shape'][1]) and float(res['energy0'][1]) == 0 and float(res['energy'][1]) == 0
    assert not same_bits(res['shape'][0], out['shape'][0]) and bool((res['energy'][[0, 2]] < res['energy0'][[0, 2]]).all())
    for k in ('cam_wp', 'pose', 'pose_rotmats', 'proxy_rep', 'boxes', 'joints2D_cropped'):
        assert same_bits(res[k].float(), out[k].float()), k
    eye = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    tverts, _ = smpl.forward_arrays(res['shape'].contiguous(), eye)
    assert same_bits(res['reposed_vertices'], tverts) and same_bits(pred.measure(res, measurer)['values'], res['measurements'])
    # targets by name
    named = pred.refine_shape(out, fitter, {'height': 1.8})
    assert bool((named['energy'][[0, 2]] < named['energy0'][[0, 2]]).all()) and same_bits(named['shape'][1], out['shape'][1])
