"""Writes tests/golden/eval_metrics_golden.npz: what the REFERENCE's evaluation code computes for the cases of tests/eval_cases.py.

    python tools/make_eval_metrics_golden.py --reference /path/to/the/reference/checkout

CPU only.  The reference's own `EvalMetricsTracker` (metrics/eval_metrics_tracker.py) is imported and run; nothing of its text is restated
here.  It is fed float64 copies of the float32 inputs, so its numbers are the float64 truth of exactly the inputs the GPU gets.

The file holds data only:
  * per point case c of eval_cases.POINT_CASES: c_sums [B,3] (the reference's per-frame means times N: raw, scale+translation corrected,
    Procrustes aligned), c_sc / c_pa [B,n,3] float64 (its returned transformed points; every eval_cases.GOLD_STRIDE-th point of a 6890-point
    case, all points otherwise) and c_idx (the indices kept).  A point case is run through the tracker as 'joints3D' (the family the
    tracker does not tie to a vertex count);
  * the tracker run on eval_cases.tracker_batches() (two update_per_batch calls): final_<metric> for the twelve metrics the reference can
    run (its metric_sums over total_samples and the divisor), frame_<metric> (the <metric>_per_frame.npy files it saves), frame_files (their names),
    returned_keys (the keys of its return_transformed_points dict, first call), returned_<key> of the first batch (strided like above),
    and the summed silhouette counts."""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def f64(d):
    return {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in d.items()}


def final_metrics(t, EC):
    """the reference's final numbers from its tracker's own attributes: compute_final_metrics only prints them.  metric_sums and
    total_samples are what it divides; the divisors are the ones of eval_cases.DIVISORS (6890, 14, 17, 10, 216)."""
    s, out = t.metric_sums, {}
    for m in t.metrics_to_track:
        if m == 'silhouette_ious':
            out[m] = float(s['num_true_positives']) / float(s['num_true_positives'] + s['num_false_negatives'] + s['num_false_positives'])
        else:
            per_sample, = [v for k, v in EC.DIVISORS.items() if k in m]
            out[m] = float(s[m]) / (t.total_samples * per_sample)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', default=os.environ.get('STRAPS_REFERENCE'), help='checkout of the reference project (or $STRAPS_REFERENCE)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'eval_metrics_golden.npz'))
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, 'metrics', 'eval_metrics_tracker.py')):
        ap.error('--reference must name a checkout of the reference project')
    sys.path.insert(0, args.reference)
    with contextlib.redirect_stdout(io.StringIO()):
        from metrics.eval_metrics_tracker import EvalMetricsTracker
    import eval_cases as EC

    def tracker(metrics, **kw):
        with contextlib.redirect_stdout(io.StringIO()):
            t = EvalMetricsTracker(list(metrics), **kw)
        t.initialise_metric_sums()
        t.initialise_per_frame_metric_lists()
        return t

    data = {}
    # ---- point cases, through the tracker's joints3D family -------------------------------------------------------------------
    for name in EC.POINT_CASES:
        EC.check_point_case(name)
        pred, target = EC.point_case(name)
        B, N = pred.shape[0], pred.shape[1]
        t = tracker(('mpjpes', 'mpjpes_sc', 'mpjpes_pa'))
        ret = t.update_per_batch({'joints3D': pred.astype(np.float64)}, {'joints3D': target.astype(np.float64)}, B, return_transformed_points=True)
        frames = np.stack([np.concatenate(t.per_frame_metrics[m]) for m in ('mpjpes', 'mpjpes_sc', 'mpjpes_pa')], axis=1)
        idx = np.arange(0, N, EC.GOLD_STRIDE if N > 1000 else 1)
        data['%s_sums' % name] = frames * N
        data['%s_idx' % name] = idx.astype(np.int32)
        data['%s_sc' % name] = ret['pred_joints3D_h36mlsp_sc'][:, idx]
        data['%s_pa' % name] = ret['pred_joints3D_h36mlsp_pa'][:, idx]
        assert data['%s_sc' % name].dtype == np.float64
    # ---- the whole tracker -------------------------------------------------------------------------------------------------------
    batches = EC.tracker_batches()
    t = tracker(EC.REFERENCE_METRICS, img_wh=EC.TRACKER_SIL_WH)
    first = None
    for pred, target, n in batches:
        with np.errstate(invalid='ignore'):
            ret = t.update_per_batch(f64(pred), f64(target), n, return_transformed_points=True)
        first = ret if first is None else first
    with np.errstate(invalid='ignore'), contextlib.redirect_stdout(io.StringIO()):
        t.compute_final_metrics()          # (must run through; it prints)
    final = final_metrics(t, EC)
    assert sorted(final) == sorted(EC.REFERENCE_METRICS)
    for k, v in final.items():
        data['final_%s' % k] = np.float64(v)
    for k in ('num_true_positives', 'num_false_positives', 'num_true_negatives', 'num_false_negatives'):
        data['sum_%s' % k] = np.float64(t.metric_sums[k])
    data['returned_keys'] = np.array(sorted(first))
    for k, v in first.items():
        data['returned_%s' % k] = v[:, ::EC.GOLD_STRIDE] if v.shape[1] > 1000 else v
    with tempfile.TemporaryDirectory() as tmp:
        t = tracker(EC.PER_FRAME_METRICS, img_wh=EC.TRACKER_SIL_WH, save_path=tmp, save_per_frame_metrics=True)
        for pred, target, n in batches:
            with np.errstate(invalid='ignore'):
                t.update_per_batch(f64(pred), f64(target), n)
        with np.errstate(invalid='ignore'), contextlib.redirect_stdout(io.StringIO()):
            t.compute_final_metrics()
        files = sorted(os.listdir(tmp))
        data['frame_files'] = np.array(files)
        for fn in files:
            data['frame_%s' % fn[:-len('_per_frame.npy')]] = np.load(os.path.join(tmp, fn))
    # the two behaviours of the reference the port decides differently: it must really show them
    for metrics, kw, exc in ((('pve-ts_pa',), {}, KeyError), (('pose_mses', 'shape_mses'), {'save_per_frame_metrics': True, 'save_path': '.'}, ValueError)):
        t = tracker(metrics, **kw)
        try:
            pred, target, n = batches[1]
            t.update_per_batch(f64(pred), f64(target), n)
            with contextlib.redirect_stdout(io.StringIO()):
                t.compute_final_metrics()
        except exc as e:
            print('reference raises on %s: %s: %s' % ('+'.join(metrics), type(e).__name__, e))
        else:
            raise SystemExit('the reference completed %s: the port\'s decision no longer describes it' % '+'.join(metrics))
    np.savez_compressed(args.out, **data)
    print('wrote %s: %d arrays, %d bytes' % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
