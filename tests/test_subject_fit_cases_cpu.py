"""CPU: the float64 restatement of the tied-shape fit (tests/subject_fit_cases.py) agrees with the per-frame restatements where the two must agree,
its tied gradient is the gradient of the summed energy, and the inputs of the GPU tests meet the conditions their bars rely on."""
import torch

import fit_cases as FC
import silfit_cases as SC
import subject_fit_cases as SF

F64 = torch.float64


# ---------------------------------------------------------------- (a) one frame per subject is the per-frame fit ----------------------------------------------------------------
def test_singleton_subjects_reproduce_the_keypoint_fit():
    case, traj, en, kw = FC.reference_fit('sigma0')
    est = case['est'].double()
    got, sub_e, frame_e, _ = SF.subject_adam_fit(est, (1,) * 6, SF.keypoint_energy_fn(case, est.clone(), sigma=kw['sigma']), 100, lr=kw['lr'])
    assert float((got - traj).abs().max()) < 1e-12
    assert float((sub_e - en).abs().max()) < 1e-12 and torch.equal(sub_e, frame_e)


def test_singleton_subjects_reproduce_the_silhouette_fit():
    c = SC.trajectory_case()
    T = SC.TRAJ
    est = c['est'].double()
    iters = 4
    want, terms = SC.adam_fit(est, est.clone(), c['masks'], c['d2'], None, None, iters, T['lattice'], T['tau'], T['w_in'], T['w_out'], lr=T['lr'],
                              lambda_pose=T['lambda_pose'], lambda_shape=T['lambda_shape'])
    got, _, _, last = SF.subject_adam_fit(est, (1, 1), SF.silhouette_energy_fn(c, est.clone()), iters, lr=T['lr'])
    assert float((got[-1] - want).abs().max()) < 1e-12 and float((last - terms[-1]).abs().max()) < 1e-12
    assert float((got[-1] - est).abs().max()) > 1e-3


# ---------------------------------------------------------------- (b) the tied gradient ----------------------------------------------------------------
def test_tied_gradient_is_the_gradient_of_the_summed_energy():
    case = FC.standard_case()
    fps = SF.KP_FPS
    off = SF.offsets_of(fps)
    est = case['est'].double()
    est0 = est.clone()
    est[:, 147:] = SF.mean_rows(est[:, 147:], off, None)[0][SF.subject_of(fps)]
    fn = SF.keypoint_energy_fn(case, est0)
    E, want = SF.tied_gradient(est, fps, fn)
    # per frame by autograd, tied by the restatement of the kernel
    _, g, _ = FC.energy_grad(est, est0, case['targets'].double(), case['conf'].double())
    z = torch.zeros(6, 157, dtype=F64)
    got = SF.subject_update(est, off, None, g, None, None, None, E.reshape(6, 1), None, 0.0, 0.0, z, z, z[:2, :10], z[:2, :10], 0, (0.01,) * 3, update=False)
    assert float((got['g'] - want).abs().max()) < 1e-12 * float(want.abs().max())
    assert float((got['E_s'] - torch.stack([E[:3].sum(), E[3:].sum()])).abs().max()) < 1e-12
    assert float((got['g'][0, 147:] - g[0, 147:]).abs().max()) > 1e-6      # (tying changes the shape gradient)
    # a masked frame leaves the sums: the subject's gradient is that of the other two frames
    mask = torch.tensor([1, 0, 1, 1, 1, 1], dtype=torch.uint8)
    got = SF.subject_update(est, off, mask, g, None, None, None, E.reshape(6, 1), None, 0.0, 0.0, z, z, z[:2, :10], z[:2, :10], 0, (0.01,) * 3, update=False)
    assert float((got['g'][1, 147:] - (g[0, 147:] + g[2, 147:])).abs().max()) < 1e-15 and int(got['n'][0]) == 2


def test_subject_update_with_singletons_is_the_per_frame_update():
    c = SF.update_case((1, 1, 1), signed=False)
    a = {k: c[k] for k in ('g_kp', 'dcam', 'dx6', 'dbetas', 'e_kp', 'energy2')}
    sm, sv = c['m'][:, 147:], c['v'][:, 147:]
    got = SF.subject_update(c['est'], c['offsets'], None, a['g_kp'], a['dcam'], a['dx6'], a['dbetas'], a['e_kp'], a['energy2'], 3.0, 0.25, c['m'], c['v'], sm, sv, 5,
                            (0.01, 0.02, 0.005))
    g, E = SF.frame_terms(3, a['g_kp'], a['dcam'], a['dx6'], a['dbetas'], a['e_kp'], a['energy2'], 3.0, 0.25)
    e1, m1, v1 = FC.adam_update(c['est'].double(), g, c['m'].double(), c['v'].double(), 6, FC.lr_columns((0.01, 0.02, 0.005)))
    assert torch.equal(got['est'], e1) and torch.equal(got['g'], g) and torch.equal(got['E_s'], E)
    assert torch.equal(got['m'][:, :147], m1[:, :147]) and torch.equal(got['sm'], m1[:, 147:]) and torch.equal(got['sv'], v1[:, 147:])
    assert torch.equal(got['m'][:, 147:], c['m'][:, 147:].double())      # the shape columns of the per-frame moments are not touched


# ---------------------------------------------------------------- (c) the conditions the GPU bars rely on ----------------------------------------------------------------
def test_update_case_meets_the_condition_of_the_adam_step_comparison():
    c = SF.update_case()
    assert c['est'].shape[0] == 464 and tuple(c['fps']) == SF.SIZES
    r = SF.subject_update(c['est'], c['offsets'], c['mask'], c['g_kp'], c['dcam'], c['dx6'], c['dbetas'], c['e_kp'], c['energy2'], 100.0, 100.0, c['m'], c['v'],
                          c['sm'], c['sv'], 5, (0.01,) * 3, update=False)
    n = r['n']
    off = c['offsets']
    assert n.tolist() == [1, 2, 2, 4, 4, 63, 0, 65, 257]
    assert int(c['mask'][off[2]]) == 0 and int(c['mask'][off[5] - 1]) == 0 and not bool(c['mask'][off[6]:off[7]].any())
    used = n > 0
    bound = SF.rounding_bound(n, r['abs_g'])
    margin = (r['g_s'].abs()[used] / bound[used]).min()
    print('update case: smallest |g_s| / rounding bound = %.3g' % float(margin))
    assert float(margin) > 1e4
    rows = torch.cat([c['est'][off[s]:off[s + 1], 147:] for s in range(len(n))])
    assert all(torch.equal(c['est'][off[s], 147:].expand(off[s + 1] - off[s], 10), c['est'][off[s]:off[s + 1], 147:]) for s in range(len(n))) and rows.shape[0] == 464


def test_silhouette_subject_case_meets_the_condition_of_the_trajectory_test():
    t0, t1 = SF.silhouette_reference()
    start, end = float((t0[:, 1] + t0[:, 2]).sum()), float((t1[:, 1] + t1[:, 2]).sum())
    per_frame = ((t1[:, 1] + t1[:, 2]) / (t0[:, 1] + t0[:, 2])).tolist()
    print('silhouette subject case (float64): E_in + E_out of the subject %.4g -> %.4g, ratio %.3f; per frame %s' % (start, end, end / start, per_frame))
    assert end / start <= 0.25
