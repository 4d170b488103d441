"""GPU: metrics.EvalMetricsTracker on the inputs of tests/golden/eval_metrics_golden.npz against what the reference's tracker computed from
float64 copies of them: final metrics, per-frame arrays (NaN where the reference has NaN), file names, returned keys and points; the
metric the reference cannot run ('pve-ts_pa') against the float64 restatement; accumulation over two calls; mask dtypes."""
import os

import numpy as np
import pytest
import torch

import eval_cases as EC
import straps_amd
from straps_amd import hipabi
from straps_amd.metrics import EvalMetricsTracker

pytestmark = pytest.mark.gpu
RTOL = 5e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    return np.load(EC.GOLD)


@pytest.fixture(scope='module')
def batches(dev):
    to = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    return [(to(p), to(t), n) for p, t, n in EC.tracker_batches()]


def _tracker(metrics, **kw):
    t = EvalMetricsTracker(list(metrics), **kw)
    t.initialise_metric_sums()
    t.initialise_per_frame_metric_lists()
    return t


@pytest.fixture(scope='module')
def full_run(batches, tmp_path_factory):
    """all thirteen metrics over both batches, per-frame files saved: shared by the tests below"""
    tmp = str(tmp_path_factory.mktemp('eval_frames'))
    t = _tracker(EC.ALL_METRICS, img_wh=EC.TRACKER_SIL_WH, save_path=tmp, save_per_frame_metrics=True)
    returned = [t.update_per_batch(p, q, n, return_transformed_points=True) for p, q, n in batches]
    sums_on_device = all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float64 for v in t.metric_sums.values())
    return t, returned, t.compute_final_metrics(), tmp, sums_on_device


def test_final_metrics_match_the_reference(full_run, gold):
    t, _, final, _, sums_on_device = full_run
    assert sums_on_device, 'running sums must be float64 device tensors'
    assert sorted(final) == sorted(EC.ALL_METRICS) and t.total_samples == 5
    for m in EC.REFERENCE_METRICS:
        print('%-16s got %.9g reference %.9g' % (m, final[m], float(gold['final_%s' % m])))
        assert final[m] == pytest.approx(float(gold['final_%s' % m]), rel=RTOL), m
    # integer counts: exact
    for k in EvalMetricsTracker.COUNT_KEYS:
        assert float(t.metric_sums[k]) == float(gold['sum_%s' % k]), k


def test_per_frame_files_match_the_reference(full_run, gold):
    _, _, _, tmp, _ = full_run
    files = sorted(os.listdir(tmp))
    assert files == sorted(gold['frame_files'].tolist() + ['pve-ts_pa_per_frame.npy'])
    for m in EC.PER_FRAME_METRICS:
        got, want = np.load(os.path.join(tmp, '%s_per_frame.npy' % m)), gold['frame_%s' % m]
        assert got.shape == want.shape == (5,)
        assert np.array_equal(np.isnan(got), np.isnan(want)), m
        np.testing.assert_allclose(got, want, rtol=RTOL, equal_nan=True, err_msg=m)
    assert np.isnan(np.load(os.path.join(tmp, 'silhouette_ious_per_frame.npy'))[1])


def test_returned_points_carry_the_references_keys_and_values(full_run, gold):
    _, returned, _, _, _ = full_run
    first = returned[0]
    assert sorted(set(first) - {'pred_reposed_vertices_pa'}) == gold['returned_keys'].tolist() and 'pred_reposed_vertices_pa' in first
    src = {'vertices': 'verts', 'reposed_vertices': 'reposed_verts', 'joints3D_h36mlsp': 'joints3D'}
    pred, target, _ = EC.tracker_batches()[0]
    for k in gold['returned_keys'].tolist():
        want = gold['returned_%s' % k]              # the reference's points (every GOLD_STRIDE-th of a 6890-point set)
        got = first[k]
        assert got.is_cuda and got.dtype == torch.float32
        got = got.cpu().numpy().astype(np.float64)
        got = got[:, ::EC.GOLD_STRIDE] if got.shape[1] > 1000 else got
        key = src[k[len('pred_'):-3]]
        whole = EC.aligned_points64(pred[key], target[key])[1 if k.endswith('_sc') else 2]      # for the frame's largest coordinate
        assert (np.abs(got - want).reshape(len(want), -1).max(1) <= EC.ulp32_of_largest(whole)).all(), k


def test_pve_ts_pa_equals_the_float64_restatement(full_run):
    _, returned, final, tmp, _ = full_run
    sums, frames, pts = 0.0, [], []
    for p, t, n in EC.tracker_batches():
        s, _, pa = EC.aligned_points64(p['reposed_verts'], t['reposed_verts'])
        sums += s[:, 2].sum()
        frames.append(s[:, 2] / 6890)
        pts.append(pa)
    assert final['pve-ts_pa'] == pytest.approx(sums / (5 * 6890), rel=RTOL)
    np.testing.assert_allclose(np.load(os.path.join(tmp, 'pve-ts_pa_per_frame.npy')), np.concatenate(frames), rtol=RTOL)
    for got, want in zip(returned, pts):
        g = got['pred_reposed_vertices_pa'].cpu().numpy().astype(np.float64)
        assert (np.abs(g - want).reshape(len(want), -1).max(1) <= EC.ulp32_of_largest(want)).all()


def test_two_calls_accumulate(batches, full_run):
    _, _, final, _, _ = full_run
    metrics = [m for m in EC.ALL_METRICS]
    singles = []
    for p, q, n in batches:
        t = _tracker(metrics)
        assert t.update_per_batch(p, q, n) is None
        singles.append((t.compute_final_metrics(), n, {k: float(v) for k, v in t.metric_sums.items()}))
    for m in metrics:
        if m == 'silhouette_ious':
            tp, fp, fn = (sum(s[2][k] for s in singles) for k in ('num_true_positives', 'num_false_positives', 'num_false_negatives'))
            assert final[m] == tp / (tp + fp + fn)
        else:
            assert final[m] == pytest.approx(sum(s[0][m] * s[1] for s in singles) / 5, rel=1e-12), m


def test_mask_dtypes_give_equal_counts(batches):
    p, q, n = batches[0]
    got = []
    for conv in (lambda m: m, lambda m: m != 0, lambda m: m.float() * 3.0):
        t = _tracker(['silhouette_ious'])
        t.update_per_batch({'silhouettes': conv(p['silhouettes'])}, {'silhouettes': conv(q['silhouettes'])}, n)
        got.append([float(t.metric_sums[k]) for k in EvalMetricsTracker.COUNT_KEYS] + [t.compute_final_metrics()['silhouette_ious']])
    assert got[0] == got[1] == got[2] and sum(got[0][:4]) == 3 * EC.TRACKER_SIL_WH ** 2


def test_mse_only_tracker_writes_no_file(batches, tmp_path):
    p, q, n = batches[1]
    t = _tracker(['pose_mses', 'shape_mses'], save_path=str(tmp_path), save_per_frame_metrics=True)
    t.update_per_batch(p, q, n)
    f = t.compute_final_metrics()
    assert os.listdir(str(tmp_path)) == [] and f['pose_mses'] > 0 and f['shape_mses'] > 0
    with pytest.raises(ValueError):
        EvalMetricsTracker(['pve_ts_pa'])
