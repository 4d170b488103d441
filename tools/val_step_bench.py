#!/usr/bin/env python3
"""What a validation pass costs (validation.ValStep, straps_val_head): two measurements in ONE child process, so that every figure comes from
the same device in the same state.

  1. one ValStep.step at --batch bodies (default 64), resnet18, the synthetic SMPL model: target generation, rasteriser, crop, proxy input,
     eval-mode forward, SMPL x4, head.
  2. the head alone against the composition it replaces, on the tensors that step kept:
       fused     straps_val_head (losses + eleven metric sums + accumulator, two launches)
       composed  straps_loss_fwd_bwd + metrics.BatchMetrics.update, run from --parent-lib (libstraps_hip.so built from the parent commit, e.g.
                 git worktree add /tmp/parent HEAD~1 && (cd /tmp/parent && python -c "import __graft_entry__ as g; g.build()")); without
                 --parent-lib the composition runs from this tree's library, and the output says so.  Timed twice: with the five gradient
                 outputs (the training form) and loss-only (gradient pointers NULL).
     The two must agree: the largest relative difference of the twelve loss values and of the eleven metric sums is reported.

Timing: device events around windows of --window calls after --warmup calls, --reps (>= 5) windows per variant, the variants alternating;
medians.  The child runs under --limit seconds; nothing is started after a failure.  Writes profiles/val_step_b64.json.

    python tools/val_step_bench.py [--parent-lib PATH] [--batch 64] [--reps 7] [--window 20] [--limit 300] [--out FILE]
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    if p not in sys.path:
        sys.path.insert(0, p)


def windows(fns, warmup, window, reps):
    """{name: fn} -> {name: [us per call, one entry per window]}; the variants alternate, and swap order every repetition"""
    import torch
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for r in range(reps):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            st.record()
            for _ in range(window):
                fns[k]()
            en.record()
            en.synchronize()
            times[k].append(st.elapsed_time(en) * 1000.0 / window)
    return times


def child(a):
    import torch
    import straps_amd
    from detgen import det_uniform
    from straps_amd import hipabi
    from straps_amd.metrics import BatchMetrics
    from straps_amd.validation import ValStep
    if not torch.cuda.is_available():
        raise RuntimeError('tools/val_step_bench.py needs a GPU: a timing taken anywhere else says nothing')
    dev, B = torch.device('cuda:0'), a.batch
    new = hipabi.load()
    old = new
    if a.parent_lib:
        old = C.CDLL(a.parent_lib)
        for name, (res, args) in hipabi.SIGNATURES.items():
            if hasattr(old, name):
                getattr(old, name).restype, getattr(old, name).argtypes = res, args
        if hasattr(old, 'straps_val_head'):
            raise RuntimeError('%s exports straps_val_head: it is not the parent commit\'s library' % a.parent_lib)

    @contextlib.contextmanager
    def library(lib):
        prev, hipabi._lib = hipabi._lib, lib
        try:
            yield
        finally:
            hipabi._lib = prev

    torch.manual_seed(0)
    mp = straps_amd.synthetic_mean_params(0)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=mp).to(dev).eval()
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=B).to(dev)
    w = {'verts': 1.0, 'joints2D': 0.1, 'pose_params': 0.1, 'shape_params': 0.1, 'joints3D': 1.0}
    crit = straps_amd.HomoscedasticUncertaintyWeightedMultiTaskLoss(list(w), init_loss_weights=w).to(dev)
    vs = ValStep(reg, smpl, crit, B)
    pose = det_uniform((B, 72), 800, -0.4, 0.4)
    pose[:, :3] *= 0.25
    pose, shape = torch.from_numpy(pose).to(dev), torch.from_numpy(det_uniform((B, 10), 801, -1.5, 1.5)).to(dev)
    keep = {}
    vs.step(pose, shape, keep=keep)
    torch.cuda.synchronize()
    step_us = windows({'val_step': lambda: vs.step(pose, shape)}, a.warmup, a.window, a.reps)['val_step']

    # ---- the head alone, on the kept tensors
    p, st = hipabi.ptr, hipabi.stream_ptr()
    k = keep
    loss_f, rows, acc = torch.empty(12, device=dev), torch.empty(B, 11, device=dev), torch.zeros(24, device=dev, dtype=torch.float64)
    ws_f = torch.empty((new.straps_val_head_workspace_bytes(B) + 7) // 8, device=dev, dtype=torch.float64)

    def fused():
        hipabi.check(new.straps_val_head(p(k['pred_verts']), p(k['pred_reposed']), p(k['pred_joints']), p(k['est']), k['ld_est'], p(k['pred_rot']), p(k['verts']),
                                         p(k['reposed']), p(k['joints2d']), p(k['joints3d']), p(k['shape']), p(k['rot']), p(k['log_vars']), p(loss_f), p(rows),
                                         p(acc), p(ws_f), B, 6890, 256, st), 'straps_val_head')

    loss_c = torch.empty(12, device=dev)
    grads = [torch.empty(B, 6890, 3, device=dev), torch.empty(B, 90, 3, device=dev), torch.empty(B, k['ld_est'], device=dev),
             torch.empty(B, 24, 3, 3, device=dev), torch.empty(5, device=dev)]
    ws_c = torch.empty(old.straps_loss_workspace_bytes(B) // 4, device=dev)
    bm = BatchMetrics(dev)
    coco = torch.tensor(straps_amd.config.ALL_JOINTS_TO_COCO_MAP, device=dev)
    h36m = torch.tensor([straps_amd.config.ALL_JOINTS_TO_H36M_MAP[i] for i in straps_amd.config.H36M_TO_J14], device=dev)
    from straps_amd.cam_utils import orthographic_project_torch
    tgt = {'verts': k['verts'], 'joints3D': k['joints3d'], 'shape_params': k['shape'], 'pose_params_rot_matrices': k['rot'], 'joints2D': k['joints2d']}

    def composed(with_grads):
        g = [p(t) for t in grads] if with_grads else [None] * 5
        hipabi.check(old.straps_loss_fwd_bwd(p(k['pred_verts']), p(k['pred_joints']), p(k['est']), k['ld_est'], p(k['pred_rot']), p(k['verts']), p(k['joints2d']),
                                             p(k['joints3d']), p(k['shape']), p(k['rot']), p(k['log_vars']), p(loss_c), *g, p(ws_c), B, 256, st),
                     'straps_loss_fwd_bwd')
        with library(old):      # what TrainStep(track_metrics=True) does after its loss call (train_step.py)
            pred = {'verts': k['pred_verts'], 'joints3D': k['pred_joints'].index_select(1, h36m), 'shape_params': k['pred_shape'],
                    'pose_params_rot_matrices': k['pred_rot'], 'joints2D': orthographic_project_torch(k['pred_joints'].index_select(1, coco), k['cam'])}
            bm.update(pred, tgt, pred_reposed_vertices=k['pred_reposed'], target_reposed_vertices=k['reposed'])

    fused()
    composed(True)
    torch.cuda.synchronize()
    rel = lambda x, y: float(((x.double() - y.double()).abs() / y.double().abs().clamp_min(1e-300)).max())
    agree = dict(loss_max_rel_diff=rel(loss_f, loss_c), metric_sums_max_rel_diff=rel(acc[12:23], bm.sums))
    head_us = windows({'fused': fused, 'composed_with_gradients': lambda: composed(True), 'composed_loss_only': lambda: composed(False)},
                      a.warmup, a.window, a.reps)
    med = lambda v: round(statistics.median(v), 2)
    res = dict(tool='tools/val_step_bench.py', when=time.strftime('%Y-%m-%d %H:%M:%S'), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               batch=B, encoder='resnet18', conv_precision=getattr(reg.image_encoder, 'conv_precision', 'fp32'),
               timing='device events around windows of %d calls after %d warm-up calls, median of %d windows, variants alternating; us per call'
                      % (a.window, a.warmup, a.reps),
               composition_library='parent commit' if a.parent_lib else 'this tree',
               val_step_us=med(step_us), val_step_us_all=[round(v, 2) for v in step_us],
               head_us={n: med(v) for n, v in head_us.items()}, head_us_all={n: [round(x, 2) for x in v] for n, v in head_us.items()},
               fused_over_composed_with_gradients=round(statistics.median(head_us['fused']) / statistics.median(head_us['composed_with_gradients']), 3),
               fused_over_composed_loss_only=round(statistics.median(head_us['fused']) / statistics.median(head_us['composed_loss_only']), 3),
               agreement=agree)
    print(json.dumps({n: res[n] for n in ('val_step_us', 'head_us', 'fused_over_composed_with_gradients', 'fused_over_composed_loss_only', 'agreement')}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--limit', type=int, default=300, help='seconds the measuring process may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'val_step_b64.json'))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error('--reps must be at least 5')
    if a.parent_lib and not os.path.isfile(a.parent_lib):
        ap.error('--parent-lib %s: no such file' % a.parent_lib)
    if a.child:
        child(a)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), '--child'] + [x for x in sys.argv[1:] if x != '--child']
    return subprocess.run(cmd, timeout=a.limit).returncode      # one fresh process under its own limit


if __name__ == '__main__':
    sys.exit(main())
