"""GPU: straps_fit_adam_subjects, straps_subject_mean_rows (csrc/fit_subjects.hip), fit.SubjectFitter and Predictor.refine(subjects=...) /
measure_subjects.

With one frame per subject the grouped update must be straps_fit_adam bit for bit.  On a batch of subjects of 1, 2, 3, 4, 5, 63, 64, 65 and 257 frames
(B = 464, masks that knock out a first frame, a last frame and a whole subject) the summed shape gradient and subject energy lie within
n * 2^-23 * sum |terms| of the float64 sum of the same fp32 terms, the shape step within the single-step bar of tests/test_gpu_fit_keypoints.py (5e-7 at lr
0.01; the inputs meet the condition of tests/test_subject_fit_cases_cpu.py), and the cam / pose columns are straps_fit_adam's bits.  Structure is
checked bit-wise: one shape in all rows of a subject, per-frame shape moments untouched, rows outside every subject untouched, a subject's bits
independent of position, neighbours (NaN ones included) and run; a NaN in a masked frame stays there.  SubjectFitter must equal its entry points
written out by hand, a split call the whole, a graph replay the eager call, singleton subjects SilhouetteFitter.  Trajectories: the standard keypoint
case read as two subjects of three frames stays within 2e-5 (parameters) and 1e-4 relative (subject energies) of the float64 tied fit over 100
iterations; the four-frame silhouette subject ends with E_in + E_out at no more than half of its start (float64: 0.161).
All buffers a kernel writes sit behind redzones (tests/redzone.py), on the NaN-poisoned allocator of conftest.py.
Measured on MI355X: sums at 0.25 (g_s) and 0.18 (E_s) of their bar, shape step 5.1e-8, shape moments 3.6e-7 and 1.3e-5 relative (bars 3.1e-5 and
6.2e-5); tied keypoint trajectory 1.1e-6 and 1.0e-6; silhouette subject ratio 0.160.  DESIGN.md has the same figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import fit_cases as FC
import predict_cases as PC
import silfit_cases as SC
import straps_amd
import subject_fit_cases as SF
from redzone import Zone
from smpl_cases import cpu_threads
from straps_amd import hipabi
from straps_amd.fit import (SilhouetteFitter, SubjectFitter, fit_adam_raw, fit_adam_subjects_raw, fit_keypoints_raw, silhouette_energy_raw,
                            subject_mean_rows_raw)

pytestmark = pytest.mark.gpu
T = SC.TRAJ
W_IN, W_OUT = 3.0, 0.25
TERMS = ('g_kp', 'dcam', 'dx6', 'dbetas', 'e_kp', 'energy2')


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
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def opts(lr=(0.01, 0.02, 0.005)):
    return hipabi.FitOptsStruct(0, 0, lr[0], lr[1], lr[2], 0.9, 0.999, 1e-8, 0.0, 1e-3, 1e-3, FC.IMG_WH)


def run_subjects(dev, c, step=5, first=True, update=True, mask=None, lr=(0.01, 0.02, 0.005), null=(), held=None, offsets=None, zero_moments=False, col=1):
    """one straps_fit_adam_subjects call on guarded buffers -> dict of CPU tensors.  c: a case of subject_fit_cases.update_case (CPU tensors); null: names of
    TERMS passed as NULL; held: (best_est, best_energy) before the call (default: NaN prefill)."""
    off = torch.from_numpy(np.asarray(c['offsets'] if offsets is None else offsets, np.int32)).to(dev)
    G, B = off.numel() - 1, c['est'].shape[0]
    z = Zone(dev)
    out = {k: z.guarded((B, 157), name=k) for k in ('est', 'm', 'v', 'grad', 'best')}
    out.update(sm=z.guarded((G, 10), name='shape_avg'), sv=z.guarded((G, 10), name='shape_avg_sq'), energy=z.guarded((B, 3), name='energy'),
               sub=z.guarded((G, 2), name='subject_energy'), best_e=z.guarded((G,), name='best_energy'))
    for k in ('est', 'm', 'v'):
        out[k].copy_(c[k])
    out['sm'].copy_(c['sm']), out['sv'].copy_(c['sv'])
    if zero_moments:
        for k in ('m', 'v', 'sm', 'sv'):
            out[k].zero_()
    if held is not None:
        out['best'].copy_(held[0]), out['best_e'].copy_(held[1])
    t = {k: (None if k in null else z.at_end(c[k])) for k in TERMS}
    fm = None if mask is None else z.at_end(mask)
    fit_adam_subjects_raw(opts(lr), out['est'], off, fm, t['g_kp'], t['dcam'], t['dx6'], t['dbetas'], t['e_kp'], t['energy2'], W_IN, W_OUT, out['m'], out['v'],
                          out['sm'], out['sv'], out['energy'], col, out['sub'], out['grad'], out['best'], out['best_e'], step, first, update, G)
    z.check()
    return {k: v.cpu() for k, v in out.items()}


def run_frames(dev, c, step=5, first=True, update=True, lr=(0.01, 0.02, 0.005), null=(), held=None, zero_moments=False, col=1):
    """the same inputs through straps_fit_adam, one body per frame"""
    B = c['est'].shape[0]
    z = Zone(dev)
    out = {k: z.guarded((B, 157), name=k) for k in ('est', 'm', 'v', 'grad', 'best')}
    out.update(energy=z.guarded((B, 3), name='energy'), best_e=z.guarded((B,), name='best_energy'))
    for k in ('est', 'm', 'v'):
        out[k].copy_(c[k])
    if zero_moments:
        out['m'].zero_(), out['v'].zero_()
    if held is not None:
        out['best'].copy_(held[0]), out['best_e'].copy_(held[1])
    t = {k: (None if k in null else z.at_end(c[k])) for k in TERMS}
    fit_adam_raw(opts(lr), out['est'], t['g_kp'], t['dcam'], t['dx6'], t['dbetas'], t['e_kp'], t['energy2'], W_IN, W_OUT, out['m'], out['v'], out['energy'], col,
                 out['grad'], out['best'], out['best_e'], step, first, update)
    z.check()
    return {k: v.cpu() for k, v in out.items()}


# ---------------------------------------------------------------- 1. singletons are straps_fit_adam ----------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 5])
@pytest.mark.parametrize('step', [0, 5])
def test_singleton_subjects_equal_fit_adam_bit_for_bit(dev, B, step):
    c = SF.update_case((1,) * B, seed=9200 + B, signed=False)
    c['g_kp'][0, 150] = -0.0      # a -0 term stays a -0 (nothing is added to it when dbetas is NULL)
    c['sm'], c['sv'] = c['m'][:, 147:].clone(), c['v'][:, 147:].clone()
    E = (c['e_kp'][:, 0].double() + W_IN * c['energy2'][:, 0].double() + W_OUT * c['energy2'][:, 1].double()).float()
    held = (torch.from_numpy(FC.det_uniform((B, 157), 9300, -1.0, 1.0)), E * torch.tensor([0.5, 2.0, 1.0, 0.5, 2.0])[:B])      # some held energies lower, some higher
    runs = [dict(null=(k,)) for k in TERMS] + [dict(first=f, update=u) for f in (True, False) for u in (True, False)] + [dict(null=('dbetas', 'dcam'))]
    for zero in (False, True):
        for kw in runs:
            kw = dict(kw, step=step, zero_moments=zero, held=None if kw.get('first', True) else held)
            a, b = run_subjects(dev, c, **kw), run_frames(dev, c, **kw)
            tag = (B, step, zero, kw)
            for k in ('est', 'energy', 'grad', 'best', 'best_e'):
                assert same_bits(a[k], b[k]), (k, tag)
            assert same_bits(a['m'][:, :147], b['m'][:, :147]) and same_bits(a['v'][:, :147], b['v'][:, :147]), tag
            assert same_bits(a['sm'], b['m'][:, 147:]) and same_bits(a['sv'], b['v'][:, 147:]), tag
            m0 = torch.zeros(B, 10) if zero else c['m'][:, 147:]
            assert same_bits(a['m'][:, 147:], m0), tag      # the per-frame shape moments are not touched
            assert same_bits(a['sub'][:, 1], a['energy'][:, 1]) and bool(torch.isnan(a['sub'][:, 0]).all()), tag
            if kw.get('update', True):
                assert not same_bits(a['est'], c['est'])
            else:
                assert same_bits(a['est'], c['est']) and same_bits(a['sm'], torch.zeros(B, 10) if zero else c['sm'])
    a = run_subjects(dev, c, null=('dbetas',), update=False)
    assert int(_bits(a['grad'])[0, 150]) == int(_bits(torch.tensor([-0.0]))[0])


# ---------------------------------------------------------------- 2. against float64 ----------------------------------------------------------------
@pytest.fixture(scope='module')
def big(dev):
    """the B = 464 case: the grouped call, straps_fit_adam on the same rows, the float64 restatement; computed once"""
    c = SF.update_case()
    lr = (0.01, 0.01, 0.01)
    got = run_subjects(dev, c, mask=c['mask'], lr=lr)
    frames = run_frames(dev, c, lr=lr)
    want = SF.subject_update(c['est'], c['offsets'], c['mask'], c['g_kp'], c['dcam'], c['dx6'], c['dbetas'], c['e_kp'], c['energy2'], W_IN, W_OUT, c['m'], c['v'],
                             c['sm'], c['sv'], 5, lr)
    return c, got, frames, want


def test_sums_and_shape_step_vs_float64(big):
    c, got, frames, want = big
    off, mask = c['offsets'], c['mask']
    G = len(off) - 1
    # the terms the kernel adds are fp32 values: straps_fit_adam's shape gradient and energy of every frame
    t_g, t_e = frames['grad'][:, 147:].double(), frames['energy'][:, 1].double()
    worst_g = worst_e = 0.0
    for s in range(G):
        rows = SF.counting(off[s], off[s + 1], mask)
        g_s, E_s = got['grad'][off[s], 147:].double(), got['sub'][s, 1].double()
        if not rows:
            assert not bool(g_s.any()) and float(E_s) == 0.0
            continue
        n = len(rows)
        bg, be = n * SF.EPS32 * t_g[rows].abs().sum(dim=0), n * SF.EPS32 * t_e[rows].abs().sum()
        eg, ee = (g_s - t_g[rows].sum(dim=0)).abs(), (E_s - t_e[rows].sum()).abs()
        worst_g, worst_e = max(worst_g, float((eg / bg).max())), max(worst_e, float(ee / be))
        assert bool((eg <= bg).all()) and bool(ee <= be), (s, n, eg, bg, ee, be)
        if n == 1:
            assert float(eg.max()) == 0.0 and float(ee) == 0.0
    # the restatement's sums (of the float64 terms) agree to the same bar
    used = want['n'] > 0
    assert bool(((got['grad'][off[:-1].astype(np.int64), 147:].double() - want['g_s']).abs()[used] <= 2 * SF.rounding_bound(want['n'], want['abs_g'])[used]).all())
    e_shape = float((got['est'][:, 147:].double() - want['est'][:, 147:]).abs().max())
    # the moments: the sum's bar (relative to a sum of like-signed terms: n * 2^-23, n = 257) and the update's own fp32 roundings; twice that for g_s^2
    e_sm = float((got['sm'].double() - want['sm']).abs().max() / want['sm'].abs().max())
    e_sv = float((got['sv'].double() - want['sv']).abs().max() / want['sv'].abs().max())
    bar_m = (257 + 4) * SF.EPS32
    print('B = 464: sum errors / bound: g_s %.3f, E_s %.3f; |shape - float64| = %.2e (bound 5e-7); shape moments relative %.2e %.2e' % (worst_g, worst_e, e_shape, e_sm, e_sv))
    assert e_shape < 5e-7 and e_sm < bar_m and e_sv < 2 * bar_m
    assert float((got['est'][:, 147:] - c['est'][:, 147:]).abs().max()) > 1e-3


def test_cam_and_pose_columns_are_fit_adam_bits(big):
    c, got, frames, _ = big
    for k in ('est', 'm', 'v', 'grad', 'best'):
        assert same_bits(got[k][:, :147], frames[k][:, :147]), k
    assert same_bits(got['energy'], frames['energy']) and bool(torch.isnan(got['energy'][:, [0, 2]]).all())
    assert same_bits(got['best'], c['est'])


@pytest.mark.parametrize('cols', [1, 10, 64])
def test_subject_mean_rows_vs_float64(dev, cols):
    c = SF.update_case()
    B, off = 464, c['offsets']
    rows = torch.from_numpy(FC.det_uniform((B, 67), 9400 + cols, -1.0, 1.0))
    rows[0, 3] = -0.0
    z = Zone(dev)
    offd = torch.from_numpy(off).to(dev)
    for mask in (None, c['mask']):
        out = z.guarded((len(off) - 1, cols), name='out')
        src = z.at_end(rows)
        subject_mean_rows_raw(src.data_ptr() + 12, 67, cols, offd, None if mask is None else z.at_end(mask), out, B, len(off) - 1)
        z.check()
        want, mag, n = SF.mean_rows(rows[:, 3:3 + cols], off, mask)
        err = (out.cpu().double() - want).abs()
        bar = SF.rounding_bound(n, mag) / n.double()[:, None]
        assert bool((err <= bar).all()), (cols, mask is None, float((err / bar).max()))
        assert same_bits(out.cpu()[0], rows[0, 3:3 + cols])      # one row: the row itself, a -0 included
    # an empty subject gives zeros; rows past the last offset are not read as a subject
    out = z.guarded((3, cols), name='out')
    subject_mean_rows_raw(src.data_ptr() + 12, 67, cols, torch.tensor([0, 2, 2, 5], dtype=torch.int32, device=dev), None, out, B, 3)
    z.check()
    assert not bool(out[1].any()) and bool(torch.isfinite(out).all())


# ---------------------------------------------------------------- 3. structure ----------------------------------------------------------------
def test_one_shape_per_subject_and_untouched_moments(big):
    c, got, _, _ = big
    off = c['offsets']
    for s in range(len(off) - 1):
        block = got['est'][off[s]:off[s + 1], 147:]
        assert same_bits(block, block[:1].expand_as(block).contiguous()), s
        gblock = got['grad'][off[s]:off[s + 1], 147:]
        assert same_bits(gblock, gblock[:1].expand_as(gblock).contiguous()), s
    assert same_bits(got['m'][:, 147:], c['m'][:, 147:]) and same_bits(got['v'][:, 147:], c['v'][:, 147:])
    # the subject without a counting frame: shape and shape moments as they were; its frames' cam and pose moved
    assert same_bits(got['est'][off[6]:off[7], 147:], c['est'][off[6]:off[7], 147:]) and same_bits(got['sm'][6], c['sm'][6]) and same_bits(got['sv'][6], c['sv'][6])
    assert not same_bits(got['est'][off[6]:off[7], :147], c['est'][off[6]:off[7], :147])
    assert not same_bits(got['sm'][5], c['sm'][5])


def sub_case(c, subjects):
    """the named subjects of a case as a batch of their own"""
    off = c['offsets']
    rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in subjects])
    out = {k: c[k][rows].clone() for k in ('est', 'm', 'v', 'mask') + TERMS}
    out['sm'], out['sv'] = c['sm'][list(subjects)].clone(), c['sv'][list(subjects)].clone()
    out['fps'] = tuple(int(off[s + 1] - off[s]) for s in subjects)
    out['offsets'] = SF.offsets_of(out['fps'])
    return out


def subject_bits(r, off, s):
    return [r[k][off[s]:off[s + 1]] for k in ('est', 'm', 'v', 'grad', 'best', 'energy')] + [r[k][s] for k in ('sm', 'sv', 'sub', 'best_e')]


def test_a_subject_depends_on_nothing_but_its_own_inputs(dev, big):
    c, got, _, _ = big
    lr = (0.01, 0.01, 0.01)
    for s in (4, 7, 8):      # 5 frames (the last masked), 65 frames, 257 frames
        ref = subject_bits(got, c['offsets'], s)
        alone = sub_case(c, (s,))
        a = run_subjects(dev, alone, mask=alone['mask'], lr=lr)
        assert all(same_bits(x, y) for x, y in zip(subject_bits(a, alone['offsets'], 0), ref)), s
        again = run_subjects(dev, alone, mask=alone['mask'], lr=lr)
        assert all(same_bits(x, y) for x, y in zip(subject_bits(again, alone['offsets'], 0), ref)), s
        # second in another batch, beside a subject whose inputs are all NaN
        pair = sub_case(c, (2, s))
        for k in TERMS + ('est', 'm', 'v'):
            pair[k][:3] = float('nan')
        pair['sm'][0], pair['sv'][0] = float('nan'), float('nan')
        b = run_subjects(dev, pair, mask=pair['mask'], lr=lr)
        assert all(same_bits(x, y) for x, y in zip(subject_bits(b, pair['offsets'], 1), ref)), s
        assert bool(torch.isnan(b['est'][:3]).all())


def test_a_nan_in_a_masked_frame_stays_there(dev, big):
    c, got, _, _ = big
    poisoned = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    dead = (c['mask'] == 0).nonzero()[:, 0]
    for k in ('g_kp', 'dbetas', 'e_kp', 'energy2', 'dcam', 'dx6'):
        poisoned[k][dead] = float('nan')
    r = run_subjects(dev, poisoned, mask=c['mask'], lr=(0.01, 0.01, 0.01))
    assert same_bits(r['est'][:, 147:], got['est'][:, 147:]) and same_bits(r['sub'][:, 1], got['sub'][:, 1]) and same_bits(r['grad'][:, 147:], got['grad'][:, 147:])
    assert same_bits(r['sm'], got['sm']) and same_bits(r['sv'], got['sv']) and same_bits(r['best_e'], got['best_e'])
    assert bool(torch.isfinite(r['est'][:, 147:]).all()) and bool(torch.isfinite(r['sub'][:, 1]).all())
    live = (c['mask'] != 0).nonzero()[:, 0]
    assert same_bits(r['est'][live], got['est'][live]) and bool(torch.isnan(r['energy'][dead, 1]).all())


def test_rows_outside_every_subject_and_empty_subjects_are_untouched(dev):
    c = SF.update_case((2, 3, 2), seed=9500, signed=False)
    off = np.array([0, 2, 2, 5], np.int32)      # subject 1 is empty, rows 5 and 6 belong to nobody
    r = run_subjects(dev, c, offsets=off)
    assert same_bits(r['est'][5:], c['est'][5:]) and same_bits(r['m'][5:], c['m'][5:]) and same_bits(r['v'][5:], c['v'][5:])
    assert bool(torch.isnan(r['grad'][5:]).all()) and bool(torch.isnan(r['best'][5:]).all()) and bool(torch.isnan(r['energy'][5:]).all())
    assert float(r['sub'][1, 1]) == 0.0 and bool(torch.isnan(r['best_e'][1])) and same_bits(r['sm'][1], c['sm'][1]) and same_bits(r['sv'][1], c['sv'][1])
    assert bool(torch.isfinite(r['sub'][[0, 2], 1]).all()) and not same_bits(r['est'][:5], c['est'][:5])
    # the two real subjects are what they are alone (subject 2 of this call owns rows 2..4)
    lone = {k: (c[k][2:5].clone() if k in ('est', 'm', 'v') + TERMS else c[k]) for k in c}
    lone['sm'], lone['sv'], lone['offsets'] = c['sm'][2:3], c['sv'][2:3], np.array([0, 3], np.int32)
    a = run_subjects(dev, lone)
    assert same_bits(a['est'], r['est'][2:5]) and same_bits(a['sm'][0], r['sm'][2]) and same_bits(a['sub'][0], r['sub'][2])
    # offsets past the batch are clamped: the last subject ends at B
    big_off = np.array([0, 2, 5, 1000], np.int32)
    b = run_subjects(dev, c, offsets=big_off)
    whole = run_subjects(dev, c, offsets=np.array([0, 2, 5, 7], np.int32))
    assert all(same_bits(b[k], whole[k]) for k in b)


def test_update_0_changes_nothing(dev):
    c = SF.update_case((3, 1, 4), seed=9600)
    r = run_subjects(dev, c, update=False)
    for k in ('est', 'm', 'v', 'sm', 'sv'):
        assert same_bits(r[k], c[k]), k
    u = run_subjects(dev, c, update=True)
    for k in ('grad', 'energy', 'sub', 'best', 'best_e'):
        assert same_bits(r[k], u[k]), k      # what an evaluation writes is what the updating call writes
    assert same_bits(r['best'], c['est'])


def test_best_iterate_per_subject(dev):
    """two subjects of 2 + 1 frames through a hand-made sequence of subject energies: down, up, NaN, equal"""
    fps = (2, 1)
    off = torch.from_numpy(SF.offsets_of(fps)).to(dev)
    z = Zone(dev)
    best, best_e, sub = z.guarded((3, 157), name='best'), z.guarded((2,), name='best_energy'), z.guarded((2, 6), name='subject_energy')
    nan = float('nan')
    # per-frame energies of call k; subject 0 sums two frames (all sums exact in fp32)
    seq = [((3.0, 1.0), 4.0), ((1.5, 0.5), 3.0), ((2.0, 1.0), 3.5), ((nan, 0.25), nan), ((1.25, 0.75), 3.0), ((0.5, 0.25), 5.0)]
    want_call = ([0, 1, 1, 1, 1, 5], [0, 1, 1, 1, 1, 1])      # the call whose est each subject holds afterwards
    want_e = ([4.0, 2.0, 2.0, 2.0, 2.0, 0.75], [4.0, 3.0, 3.0, 3.0, 3.0, 3.0])
    for k, ((a, b), e1) in enumerate(seq):
        est = torch.full((3, 157), float(k), device=dev)
        e_kp = torch.tensor([[a], [b], [e1]], device=dev)
        fit_adam_subjects_raw(opts(), est, off, None, None, None, None, None, e_kp, None, 1.0, 1.0, None, None, None, None, None, k, sub, None, best, best_e, k, k == 0,
                              False, 2)
        z.check()
        for s, rows in ((0, slice(0, 2)), (1, slice(2, 3))):
            assert float(best_e[s]) == want_e[s][k], (k, s, best_e.tolist())
            assert bool((best[rows] == float(want_call[s][k])).all()), (k, s)
    assert torch.isnan(sub[0, 3]) and float(sub[0, 4]) == 2.0 and float(sub[1, 4]) == 3.0


# ---------------------------------------------------------------- 4. SubjectFitter ----------------------------------------------------------------
FPS3 = (2, 1)


def inputs3(dev):
    """three frames at wh = 64 read as subjects of 2 + 1 frames: silfit_cases' three targets, a perturbed start, keypoint targets of the true bodies"""
    c = SC.three_body_case()
    true = c['true']
    est = c['est'] + torch.from_numpy(FC.det_uniform((3, 157), 8200, -0.03, 0.03))
    with torch.no_grad():
        p = SC.O.orthographic_project(FC.keypoints3d(true.double(), FC.COCO), true.double()[:, :3])
    targets = ((p + 1.0) * (T['wh'] / 2.0)).float()
    conf = torch.from_numpy(FC.det_uniform((3, 17), 8300, 0.3, 1.0))
    return est.to(dev), targets.to(dev), conf.to(dev), torch.from_numpy(c['masks']).to(dev)


def split(est):
    return est[:, :3].contiguous(), est[:, 3:147].contiguous(), est[:, 147:].contiguous()


def fitter_for(smpl, iters, cls=SubjectFitter, **kw):
    return cls(smpl, iters=iters, lattice=T['lattice'], tau=T['tau'], w_in=T['w_in'], w_out=T['w_out'], img_wh=T['wh'], **kw)


def by_hand(dev, smpl, f, est, targets, conf, sil, iters, fps):
    """SubjectFitter.__call__ as its entry points; sil None: keypoints only (two launches per iteration)"""
    L, st = hipabi.lib(), hipabi.stream_ptr()
    B, G = est.shape[0], len(fps)
    off = torch.from_numpy(SF.offsets_of(fps)).to(dev)
    est, est0 = est.clone(), est.clone()
    mean = torch.empty(G, 10, device=dev)
    subject_mean_rows_raw(est.data_ptr() + 147 * 4, 157, 10, off, None, mean, B, G)
    est[:, 147:] = mean[SF.subject_of(fps).to(dev)]
    e = lambda *s: torch.empty(*s, device=dev)
    e_kp, g_kp, kp2d = e(B, 1), e(B, 157), e(B, 17, 2)
    dcam = dx6 = dbetas = e2 = R = None
    if sil is not None:
        mask = (sil != 0).to(torch.uint8)
        d2 = torch.empty(mask.shape, device=dev, dtype=torch.int32)
        hipabi.check(L.straps_distance_field(hipabi.ptr(mask), hipabi.ptr(d2), B, mask.shape[1], st), 'straps_distance_field')
        R, betas, verts, dverts, dcam, e2, drot, dbetas, dx6 = e(B, 24, 3, 3), e(B, 10), e(B, 6890, 3), e(B, 6890, 3), e(B, 3), e(B, 2), e(B, 24, 3, 3), e(B, 10), e(B, 144)
        ws = torch.empty(L.straps_silhouette_energy_workspace_bytes(B, 6890, f.wh, f.lattice) // 8, device=dev, dtype=torch.float64)
        ws2 = e(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)
    m, v, sm, sv = torch.zeros(B, 157, device=dev), torch.zeros(B, 157, device=dev), torch.zeros(G, 10, device=dev), torch.zeros(G, 10, device=dev)
    energy, sub, best, best_e = e(B, iters + 1), e(G, iters + 1), e(B, 157), e(G)
    x6 = C.c_void_p(est.data_ptr() + 12)
    for i in range(iters + 1):
        if sil is not None:
            hipabi.check(L.straps_rot6d_fwd(x6, 157, 24, hipabi.ptr(R), B, st), 'straps_rot6d_fwd')
            betas.copy_(est[:, 147:])
            smpl.forward_arrays(betas, R, want_joints=False, out_verts=verts)
            silhouette_energy_raw(verts, est, 157, mask, d2, f.sil_opts(), e2, dverts, dcam, None, ws)
            hipabi.check(L.straps_smpl_bwd(C.byref(smpl._model_struct()), hipabi.ptr(betas), hipabi.ptr(R), hipabi.ptr(dverts), None, hipabi.ptr(dbetas),
                                           hipabi.ptr(drot), hipabi.ptr(ws2), B, 0, st), 'straps_smpl_bwd')
            hipabi.check(L.straps_rot6d_bwd(x6, 157, 24, hipabi.ptr(drot), hipabi.ptr(dx6), 144, B, st), 'straps_rot6d_bwd')
        fit_keypoints_raw(f._struct, f.opts(0), est.clone(), est0, targets, conf, None, None, e_kp, g_kp, None, None, kp2d)
        fit_adam_subjects_raw(f.opts(), est, off, None, g_kp, dcam, dx6, dbetas, e_kp, e2, f.w_in, f.w_out, m, v, sm, sv, energy, i, sub, None, best, best_e, i,
                              i == 0, i < iters, G)
    return {'est': est, 'm': m, 'v': v, 'sm': sm, 'sv': sv, 'energy': energy, 'sub': sub, 'best': best, 'best_e': best_e, 'R': R,
            'terms': None if sil is None else torch.cat([e_kp, e2], dim=1)}


@pytest.mark.parametrize('with_sil', [False, True])
def test_call_equals_its_entry_points_and_a_split_call_equals_the_whole(dev, smpl, with_sil):
    est, targets, conf, sil = inputs3(dev)
    keep = [t.clone() for t in (est, targets, conf, sil)]
    f = fitter_for(smpl, 3)
    kw = dict(silhouettes=sil if with_sil else None, joints2D=targets, conf=conf)
    out = f(*split(est), FPS3, trace=True, **kw)
    hand = by_hand(dev, smpl, f, est, targets, conf, sil if with_sil else None, 3, FPS3)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((est, targets, conf, sil), keep)), 'the inputs are not modified'
    got = torch.cat([out['cam_wp'], out['pose'], out['shape']], dim=1)
    assert same_bits(got, hand['est']) and not same_bits(got, est)
    assert same_bits(out['trace'], hand['sub']) and same_bits(out['subject_energy0'], hand['sub'][:, 0]) and same_bits(out['subject_energy'], hand['sub'][:, 3])
    assert same_bits(out['energy0'], hand['energy'][:, 0]) and same_bits(out['energy'], hand['energy'][:, 3])
    st = out['state']
    assert all(same_bits(st[k], hand[h]) for k, h in (('exp_avg', 'm'), ('exp_avg_sq', 'v'), ('shape_avg', 'sm'), ('shape_avg_sq', 'sv'))) and st['step'] == 3
    assert same_bits(torch.cat([out['best'][k] for k in ('cam_wp', 'pose', 'shape')], dim=1), hand['best']) and same_bits(out['best']['energy'], hand['best_e'])
    assert same_bits(out['subject_shape'], hand['est'][[0, 2], 147:]) and same_bits(out['shape'][1], out['shape'][0]) and tuple(out['trace'].shape) == (2, 4)
    keys = {'cam_wp', 'pose', 'shape', 'pose_rotmats', 'energy0', 'energy', 'best', 'joints2D', 'state', 'trace', 'subject_shape', 'subject_energy0', 'subject_energy'}
    assert set(out) == (keys | {'energy_terms'} if with_sil else keys)
    if with_sil:
        assert same_bits(out['energy_terms'], hand['terms']) and same_bits(out['pose_rotmats'], hand['R'])
    assert same_bits(out['pose_rotmats'], straps_amd.rot6d_to_rotmat(out['pose'].contiguous()).view(3, 24, 3, 3))
    # two calls of one and two iterations, the state and the prior centre carried over (the shapes of a subject are equal by then: their mean is that shape)
    one = fitter_for(smpl, 1)(*split(est), FPS3, **kw)
    two = fitter_for(smpl, 2)(one['cam_wp'].contiguous(), one['pose'].contiguous(), one['shape'].contiguous(), FPS3, prior=split(est), state=one['state'], **kw)
    for k in ('cam_wp', 'pose', 'shape', 'energy', 'subject_energy', 'subject_shape', 'joints2D') + (('energy_terms',) if with_sil else ()):
        assert same_bits(two[k], out[k]), k
    assert all(same_bits(two['state'][k], st[k]) for k in ('exp_avg', 'exp_avg_sq', 'shape_avg', 'shape_avg_sq')) and two['state']['step'] == 3
    # evaluate: the first evaluation of the loop
    E_s, g, E_f = f.evaluate(*split(est), FPS3, **kw)
    assert same_bits(E_s, hand['sub'][:, 0]) and same_bits(E_f, hand['energy'][:, 0]) and same_bits(g[0, 147:], g[1, 147:]) and tuple(g.shape) == (3, 157)


def test_call_refuses_what_it_cannot_fit(dev, smpl):
    est, targets, conf, sil = inputs3(dev)
    f = fitter_for(smpl, 1)
    with pytest.raises(ValueError, match='silhouettes, joints2D or both'):
        f(*split(est), FPS3)
    for bad in ((2, 2), (3, 0), (1.5, 1.5), ()):
        with pytest.raises(ValueError, match='frames_per_subject'):
            f(*split(est), bad, joints2D=targets)
    with pytest.raises(RuntimeError, match='frame_mask'):
        f(*split(est), FPS3, joints2D=targets, frame_mask=torch.ones(2, device=dev))
    with pytest.raises(RuntimeError, match='shape_avg'):
        f(*split(est), FPS3, joints2D=targets, state={'exp_avg': torch.zeros(3, 157, device=dev), 'exp_avg_sq': torch.zeros(3, 157, device=dev), 'step': 0})


@pytest.mark.parametrize('with_sil', [False, True])
def test_call_is_capturable(dev, smpl, with_sil):
    est, targets, conf, sil = inputs3(dev)
    f = fitter_for(smpl, 2)
    fm = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    kw = dict(silhouettes=sil if with_sil else None, joints2D=targets, conf=conf, frame_mask=fm, trace=True)
    eager = f(*split(est), FPS3, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    args = split(est)
    with torch.cuda.graph(graph):
        cap = f(*args, FPS3, **kw)
    graph.replay()
    torch.cuda.synchronize()
    for k in ('cam_wp', 'pose', 'shape', 'pose_rotmats', 'energy0', 'energy', 'joints2D', 'trace', 'subject_shape', 'subject_energy') + (('energy_terms',) if with_sil else ()):
        assert same_bits(cap[k], eager[k]), k
    assert same_bits(cap['best']['pose'], eager['best']['pose'])
    # the masked frame received the shape of the frame that counts
    assert same_bits(eager['shape'][1], eager['shape'][0]) and same_bits(eager['subject_shape'][0], eager['shape'][0])


def test_singleton_subjects_are_the_silhouette_fitter(dev, smpl):
    est, targets, conf, sil = inputs3(dev)
    a = fitter_for(smpl, 3)(*split(est), (1, 1, 1), silhouettes=sil, joints2D=targets, conf=conf, trace=True)
    b = fitter_for(smpl, 3, cls=SilhouetteFitter)(*split(est), sil, targets, conf=conf, trace=True)
    for k in ('cam_wp', 'pose', 'shape', 'pose_rotmats', 'energy0', 'energy', 'energy_terms', 'joints2D', 'trace'):
        assert same_bits(a[k], b[k]), k
    assert same_bits(a['subject_energy'], b['energy']) and same_bits(a['subject_shape'], b['shape'])
    assert same_bits(a['state']['exp_avg'][:, :147], b['state']['exp_avg'][:, :147]) and same_bits(a['state']['shape_avg'], b['state']['exp_avg'][:, 147:])
    assert all(same_bits(a['best'][k], b['best'][k]) for k in ('cam_wp', 'pose', 'shape', 'energy'))


# ---------------------------------------------------------------- 5. trajectories ----------------------------------------------------------------
def test_keypoint_trajectory_vs_float64(dev, smpl):
    case, traj, sub_e, _ = SF.keypoint_reference()
    f = SubjectFitter(smpl, iters=100, lr=0.01, img_wh=FC.IMG_WH)
    est = case['est'].to(dev)
    out = f(*split(est), SF.KP_FPS, joints2D=case['targets'].to(dev), conf=case['conf'].to(dev), trace=True)
    got = torch.cat([out['cam_wp'], out['pose'], out['shape']], dim=1).cpu().double()
    e_est = float((got - traj[-1]).abs().max())
    e_en = float(((out['trace'].cpu().double() - sub_e).abs() / sub_e.abs()).max())
    print('tied keypoint trajectory: |est_100 - float64| = %.2e (bound 2e-5), subject energy trace relative %.2e (bound 1e-4)' % (e_est, e_en))
    assert e_est < 2e-5 and e_en < 1e-4, (e_est, e_en)
    assert same_bits(out['shape'][0], out['shape'][2]) and same_bits(out['shape'][3], out['shape'][5]) and not same_bits(out['shape'][0], out['shape'][3])
    assert bool((out['subject_energy'] < out['subject_energy0']).all())


def test_silhouette_subject_trajectory(dev, smpl):
    c = SF.silhouette_subject_case()
    est, sil = c['est'].to(dev), torch.from_numpy(c['masks']).to(dev)
    f = fitter_for(smpl, T['iters'], lr=T['lr'], lambda_pose=T['lambda_pose'], lambda_shape=T['lambda_shape'])
    t0 = SilhouetteFitter.evaluate(f, *split(est), sil)[2]      # (the start shapes are equal: the tied start is the start)
    out = f(*split(est), c['fps'], silhouettes=sil)
    start, end = float((t0[:, 1] + t0[:, 2]).sum()), float((out['energy_terms'][:, 1] + out['energy_terms'][:, 2]).sum())
    print('silhouette subject of %d frames: E_in + E_out %.4g -> %.4g, ratio %.3f (float64: 0.161); per frame %s'
          % (est.shape[0], start, end, end / start, ((out['energy_terms'][:, 1] + out['energy_terms'][:, 2]) / (t0[:, 1] + t0[:, 2])).tolist()))
    assert end / start <= 0.5
    assert float(out['subject_energy'][0]) < float(out['subject_energy0'][0]) and float(out['best']['energy'][0]) <= float(out['subject_energy'][0])
    assert all(same_bits(out['shape'][k], out['shape'][0]) for k in range(1, est.shape[0]))


# ---------------------------------------------------------------- 6. Predictor ----------------------------------------------------------------
def test_predictor_refine_with_subjects_and_measure_subjects(dev, smpl):
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=straps_amd.synthetic_mean_params(0)).to(dev).eval()
    sil, joints = PC.inputs('a')
    sil, joints = torch.from_numpy(sil[:4].copy()).to(dev), torch.from_numpy(joints[:4]).to(dev)
    sil[1] = 0                                                    # an empty silhouette: invalid
    pred = straps_amd.Predictor(reg, smpl)
    out = pred(sil, joints)
    assert out['valid'].tolist() == [True, False, True, True]
    f = SubjectFitter(smpl, iters=3)
    subjects = [2, 2]
    ref = pred.refine(out, f, subjects=subjects)
    torch.cuda.synchronize()
    assert set(ref) == set(out) | {'energy0', 'energy', 'energy_terms', 'subject_shape', 'subject_energy0', 'subject_energy', 'subjects'} and ref['subjects'] == subjects
    for k in ('cam_wp', 'pose'):
        assert same_bits(ref[k][1], out[k][1]) and not same_bits(ref[k][0], out[k][0]), k
    assert tuple(ref['subject_shape'].shape) == (2, 10)
    for b, s in ((0, 0), (1, 0), (2, 1), (3, 1)):
        assert same_bits(ref['shape'][b], ref['subject_shape'][s]), b
    # the invalid frame pulled nothing: subject 0 is what frame 0 alone gives
    alone = {k: (v[[0, 2, 3]] if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    ref3 = pred.refine(alone, f, subjects=[1, 2])
    assert same_bits(ref3['subject_shape'], ref['subject_shape']) and same_bits(ref3['subject_energy'], ref['subject_energy'])
    assert same_bits(ref3['cam_wp'][0], ref['cam_wp'][0]) and same_bits(ref3['pose'][1:], ref['pose'][2:])
    # measurements per subject: those of any of its frames
    measurer = straps_amd.BodyMeasurer.from_smpl(smpl).to(dev)
    per_frame, per_subject = pred.measure(ref, measurer), pred.measure_subjects(ref, measurer)
    assert list(per_subject) == list(per_frame) and tuple(per_subject['values'].shape) == (2, per_frame['values'].shape[1])
    for k in per_subject:
        assert same_bits(per_subject[k][0], per_frame[k][1]) and same_bits(per_subject[k][1], per_frame[k][2]), k
    with pytest.raises(ValueError, match='subjects'):
        pred.refine(out, f)
    with pytest.raises(ValueError, match='subjects'):
        pred.refine(out, SilhouetteFitter(smpl, iters=1), subjects=subjects)
    with pytest.raises(ValueError, match='subjects'):
        pred.refine(out, straps_amd.KeypointFitter(smpl, iters=1), subjects=subjects)
    with pytest.raises(ValueError, match='subject_shape'):
        pred.measure_subjects(out, measurer)
