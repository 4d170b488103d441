"""Timing of the on-device evaluation on the GPU, beside the host numpy path it replaces; writes profiles/eval_metrics_b64.json.

    python tools/eval_profile.py [--batch 64] [--iters 50] [--host-iters 1] [--out profiles/eval_metrics_b64.json]

Measured, at B = 64, 6890 vertices, 14 joints, 256 x 256 masks:
  * one EvalMetricsTracker.update_per_batch with all thirteen metrics, inputs resident on the device, return_transformed_points off and on:
    device events around `iters` back-to-back calls after a warm-up (nothing in update_per_batch synchronises);
  * one WeakPerspectiveSilhouetteRenderer call (synthetic SMPL mesh, 13 776 faces, posed by the template) the same way;
  * the three library entries alone (straps_point_align on the vertices, straps_silhouette_counts, straps_wp_silhouette);
  * the host path: the same quantities with numpy -- oracle/straps_oracle.py's point_metrics helpers (scale_and_translation_transform,
    similarity_transform with one SVD per sample) on float64 copies, the confusion counts with np.logical_and -- under a host clock,
    with the number of threads numpy's BLAS may use stated (the device-to-host copy of the inputs is timed separately).
No speed bar is set anywhere: the file is where the measured numbers go."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import straps_amd                      # noqa: E402
import straps_oracle as O              # noqa: E402
from detgen import det_metrics_case, det_uniform      # noqa: E402
from straps_amd import hipabi          # noqa: E402

ALL = list(straps_amd.EvalMetricsTracker.METRICS)


def device_us(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def inputs(B, wh):
    pv, tv = det_metrics_case(6890, 70, batch=B)
    pr, tr = det_metrics_case(6890, 74, batch=B)
    pj, tj = det_metrics_case(14, 72, batch=B)
    rr, cc = np.mgrid[0:wh, 0:wh]
    ps = np.stack([(((rr - 120 - b % 7) / 90.0) ** 2 + ((cc - 128) / 40.0) ** 2 <= 1.0) for b in range(B)]).astype(np.uint8)
    ts = np.stack([(((rr - 126) / 95.0) ** 2 + ((cc - 124 - b % 5) / 42.0) ** 2 <= 1.0) for b in range(B)]).astype(np.uint8)
    pred = {'verts': pv, 'reposed_verts': pr, 'joints3D': pj, 'joints2D': det_uniform((B, 17, 2), 1), 'shape_params': det_uniform((B, 10), 2),
            'pose_params_rot_matrices': det_uniform((B, 24, 3, 3), 3), 'silhouettes': ps}
    target = {'verts': tv, 'reposed_verts': tr, 'joints3D': tj, 'joints2D': det_uniform((B, 17, 2), 4), 'shape_params': det_uniform((B, 10), 5),
              'pose_params_rot_matrices': det_uniform((B, 24, 3, 3), 6), 'silhouettes': ts}
    return pred, target


def host_update(pred, target):
    """the numpy path for all thirteen metrics on float64 copies -> a few sums (so that nothing is optimised away)"""
    out = []
    for key in ('verts', 'reposed_verts', 'joints3D'):
        out.append(O.point_metrics(pred[key], target[key]).sum(0))
    out.append(((pred['pose_params_rot_matrices'].astype(np.float64) - target['pose_params_rot_matrices']) ** 2).sum())
    out.append(((pred['shape_params'].astype(np.float64) - target['shape_params']) ** 2).sum())
    out.append(np.linalg.norm(pred['joints2D'].astype(np.float64) - target['joints2D'], axis=-1).sum())
    p, t = pred['silhouettes'], target['silhouettes']
    tp = np.logical_and(p, t).sum(axis=(1, 2))
    fp = np.logical_and(p, np.logical_not(t)).sum(axis=(1, 2))
    tn = np.logical_and(np.logical_not(p), np.logical_not(t)).sum(axis=(1, 2))
    fn = np.logical_and(np.logical_not(p), t).sum(axis=(1, 2))
    out.append(np.array([tp.sum(), fp.sum(), tn.sum(), fn.sum()]))
    return out


def blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return [{'api': i.get('user_api'), 'lib': i.get('internal_api'), 'threads': i.get('num_threads')} for i in threadpool_info()]
    except ImportError:
        return {'threadpoolctl': 'not installed', 'OMP_NUM_THREADS': os.environ.get('OMP_NUM_THREADS'), 'OPENBLAS_NUM_THREADS': os.environ.get('OPENBLAS_NUM_THREADS'),
                'MKL_NUM_THREADS': os.environ.get('MKL_NUM_THREADS'), 'torch_get_num_threads': torch.get_num_threads()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_metrics_b64.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda:0')
    hipabi.load()
    B, wh = args.batch, 256
    pred, target = inputs(B, wh)
    dp = {k: torch.from_numpy(v).to(dev) for k, v in pred.items()}
    dt = {k: torch.from_numpy(v).to(dev) for k, v in target.items()}

    def tracker_call(points):
        t = straps_amd.EvalMetricsTracker(ALL)
        t.initialise_metric_sums()
        t.initialise_per_frame_metric_lists()

        def fn():
            t.per_frame_metrics = {m: [] for m in ALL}          # (the lists would grow with every timed call)
            return t.update_per_batch(dp, dt, B, return_transformed_points=points)
        return t, fn

    res = {'what': 'on-device evaluation on one MI355X beside the host numpy path: tools/eval_profile.py; one run on one box', 'batch': B,
           'shape': {'verts': 6890, 'joints3D': 14, 'mask': [wh, wh], 'faces': 13776}, 'iters': args.iters,
           'method': 'device events around back-to-back calls after 5 warm-up calls; host path under time.perf_counter'}
    try:
        res['commit'] = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        res['commit'] = os.environ.get('STRAPS_COMMIT', 'unknown (no git metadata beside the tree that was measured)')
    t, fn = tracker_call(False)
    res['update_per_batch_all_metrics_us'] = round(device_us(fn, args.iters), 1)
    t2, fn2 = tracker_call(True)
    res['update_per_batch_all_metrics_with_returned_points_us'] = round(device_us(fn2, args.iters), 1)
    final = t.compute_final_metrics()
    res['final_metrics_of_the_timed_inputs'] = {k: float(v) for k, v in final.items()}

    model = straps_amd.synthetic_smpl_model(0)
    rend = straps_amd.WeakPerspectiveSilhouetteRenderer(model['faces'], img_wh=wh).to(dev)
    verts = torch.from_numpy(np.broadcast_to(model['v_template'][None], (B, 6890, 3)).copy()).to(dev)
    cam = torch.from_numpy(np.tile(np.array([[0.9, 0.02, -0.05]], np.float32), (B, 1))).to(dev)
    mask = torch.empty(B, wh, wh, dtype=torch.uint8, device=dev)
    res['render_us'] = round(device_us(lambda: rend(verts, cam), args.iters), 1)
    res['render_covered_fraction'] = round(float(rend(verts, cam).float().mean()), 4)

    L, st = hipabi.lib(), hipabi.stream_ptr()
    out3, sc, pa = torch.empty(B, 3, device=dev), torch.empty_like(dp['verts']), torch.empty_like(dp['verts'])
    counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
    ws = torch.empty(L.straps_wp_silhouette_workspace_bytes(B, 6890) // 4, device=dev)
    res['entries_us'] = {
        'straps_point_metrics_6890': round(device_us(lambda: L.straps_point_metrics(hipabi.ptr(dp['verts']), hipabi.ptr(dt['verts']), hipabi.ptr(out3), B, 6890, st), args.iters), 1),
        'straps_point_align_6890': round(device_us(lambda: L.straps_point_align(hipabi.ptr(dp['verts']), hipabi.ptr(dt['verts']), hipabi.ptr(out3), hipabi.ptr(sc),
                                                                                hipabi.ptr(pa), B, 6890, st), args.iters), 1),
        'straps_silhouette_counts_256x256': round(device_us(lambda: L.straps_silhouette_counts(hipabi.ptr(dp['silhouettes']), hipabi.ptr(dt['silhouettes']),
                                                                                                  hipabi.ptr(counts), B, wh * wh, st), args.iters), 1),
        'straps_wp_silhouette_256': round(device_us(lambda: L.straps_wp_silhouette(hipabi.ptr(verts), hipabi.ptr(rend.faces), hipabi.ptr(cam), hipabi.ptr(mask),
                                                                                   hipabi.ptr(ws), B, 6890, 13776, wh, st), args.iters), 1)}
    res['entries_note'] = ('host-side launch cost included (ctypes calls issued back to back); silhouette_counts at 256 x 256 is a fill kernel plus the '
                           'count kernel, wp_silhouette a fill, a projection and a face kernel')

    # ---- host path ---------------------------------------------------------------------------------------------------------------
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hp = {k: v.cpu().numpy() for k, v in dp.items()}
    ht = {k: v.cpu().numpy() for k, v in dt.items()}
    copy_ms = (time.perf_counter() - t0) * 1e3
    host_update(hp, ht)
    t0 = time.perf_counter()
    for _ in range(args.host_iters):
        h = host_update(hp, ht)
    host_ms = (time.perf_counter() - t0) * 1e3 / args.host_iters
    res['host_numpy'] = {'update_all_metrics_ms': round(host_ms, 2), 'device_to_host_copy_ms': round(copy_ms, 2), 'iters': args.host_iters,
                         'threads': blas_threads(), 'cpus_available': len(os.sched_getaffinity(0)),
                         'what': "oracle/straps_oracle.py point_metrics (float64, one np.linalg.svd per sample) for verts, reposed_verts, joints3D; numpy for the rest"}
    # the two paths computed the same thing
    dev_pve = res['final_metrics_of_the_timed_inputs']['pves_pa']
    res['host_vs_device_pves_pa_rel_diff'] = abs(float(h[0][2]) / (B * 6890) - dev_pve) / dev_pve
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=2)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
