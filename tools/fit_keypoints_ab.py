"""A/B of 100 iterations of keypoint fitting: the fused call (straps_fit_keypoints through KeypointFitter, one launch) vs the same loop
composed from the entry points that existed before it -- rot6d_to_rotmat, SMPL.forward under autograd (the full 6 890-vertex forward and
backward), orthographic_project_torch, torch.optim.Adam on one [B,157] tensor with E.sum().  Adam is per element, so with equal learning
rates the two walk the same trajectory; the largest difference of the final parameters is reported, not asserted (fp32 against fp32 in
another summation order).  sigma = 0, lambda 1e-3, lr 0.01, the synthetic model, seeded inputs as tests/fit_cases.standard_case makes them
(the seeded generator is oracle/detgen.py, put on sys.path here: the tool runs from a checkout, not from an installed package).

Timing: one warm-up call of each, then --reps (>= 5) timed calls of each, alternating, device events around a whole call; medians.  The
device's clock report is read before and after (read only).  Every batch size runs in a child process of its own under a time limit; the
first failure ends the run.  Writes profiles/fit_keypoints_ab.json.

    python tools/fit_keypoints_ab.py [--batches 64 4096] [--iters 100] [--reps 5] [--limit 240]
"""
import argparse
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


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks', '-d', '0'], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in r.stdout.splitlines() if 'clk' in ln.lower()][:8]
    except Exception as e:      # noqa: BLE001 (the report is a note, not a result)
        return ['unavailable: %s' % e]


def inputs(B, dev):
    import torch
    import straps_amd
    from detgen import det_uniform
    u = lambda shape, k, lo, hi: torch.from_numpy(det_uniform(shape, 4100 + k, lo, hi)).to(dev)
    x6 = lambda aa: straps_amd.batch_rodrigues(aa.reshape(-1, 3)).view(B, 24, 3, 3)[:, :, :, :2].reshape(B, 144)
    aa, betas = u((B, 72), 1, -0.4, 0.4), u((B, 10), 2, -1.5, 1.5)
    cam = torch.tensor([0.9, 0.0, 0.0], device=dev) + u((B, 3), 3, -0.1, 0.1)
    true = torch.cat([cam, x6(aa), betas], 1)
    start = torch.cat([cam + u((B, 3), 4, -0.05, 0.05), x6(aa + u((B, 72), 5, -0.25, 0.25)), betas + u((B, 10), 6, -1.0, 1.0)], 1)
    conf = u((B, 17), 7, 0.3, 1.0)
    return true.contiguous(), start.contiguous(), conf


def one_batch(B, iters, reps, out_path):
    import torch
    import straps_amd
    from straps_amd import cam_utils, config
    dev = torch.device('cuda:0')
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=1).to(dev)
    coco = list(config.ALL_JOINTS_TO_COCO_MAP)
    wh = float(config.REGRESSOR_IMG_WH)
    true, start, conf = inputs(B, dev)
    with torch.no_grad():
        R = straps_amd.rot6d_to_rotmat(true[:, 3:147].contiguous()).view(B, 24, 3, 3)
        _, joints = smpl.forward_arrays(true[:, 147:].contiguous(), R)
        targets = cam_utils.undo_keypoint_normalisation(cam_utils.orthographic_project_torch(joints[:, coco].contiguous(), true[:, :3]), wh)
    fitter = straps_amd.KeypointFitter(smpl, iters=iters, lr=0.01, lambda_pose=1e-3, lambda_shape=1e-3, img_wh=wh)
    cam0, pose0, shape0 = start[:, :3].contiguous(), start[:, 3:147].contiguous(), start[:, 147:].contiguous()
    res = {}

    def fused():
        o = fitter(cam0, pose0, shape0, targets, conf=conf)
        res['fused'] = (torch.cat([o['cam_wp'], o['pose'], o['shape']], 1), o['energy0'], o['energy'])

    w, that = conf * conf, 2.0 * targets / wh - 1.0

    def energy(est):
        R = straps_amd.rot6d_to_rotmat(est[:, 3:147]).view(B, 24, 3, 3)
        out = smpl(betas=est[:, 147:], body_pose=R[:, 1:], global_orient=R[:, :1], pose2rot=False)
        kp = cam_utils.orthographic_project_torch(out.joints[:, coco], est[:, :3])
        return (w * ((kp - that) ** 2).sum(-1)).sum(1) + 1e-3 * ((est[:, 3:147] - start[:, 3:147]) ** 2).sum(1) \
            + 1e-3 * ((est[:, 147:] - start[:, 147:]) ** 2).sum(1)

    def composed():
        est = start.clone().requires_grad_(True)
        opt = torch.optim.Adam([est], lr=0.01)
        e0 = None
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            E = energy(est)
            e0 = E.detach() if e0 is None else e0
            E.sum().backward()
            opt.step()
        with torch.no_grad():
            res['composed'] = (est.detach(), e0, energy(est))

    fns = {'fused': fused, 'composed': composed}
    before = clocks()
    for f in fns.values():      # warm-up: code objects, allocator, autograd state
        f()
    torch.cuda.synchronize()
    diff = float((res['fused'][0] - res['composed'][0]).abs().max())
    e_rel = float(((res['fused'][2] - res['composed'][2]).abs() / res['composed'][2].abs().clamp_min(1e-30)).max())
    ratio = float((res['fused'][2] / res['fused'][1]).max())
    times = {k: [] for k in fns}
    for r in range(reps):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            st.record()
            fns[k]()
            en.record()
            en.synchronize()
            times[k].append(st.elapsed_time(en))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = dict(batch=B, iters=iters, ms=med, ms_all=times, speedup=med['composed'] / med['fused'], max_abs_param_diff=diff,
               final_energy_rel_diff=e_rel, worst_final_over_start_energy=ratio, clocks_before=before, clocks_after=clocks())
    print('B=%-5d fused %9.3f ms   composed %9.3f ms   x%.1f   |est diff| %.2e   E_n/E_0 <= %.4f' % (B, med['fused'], med['composed'], row['speedup'], diff, ratio), flush=True)
    with open(out_path, 'w') as f:
        json.dump(row, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', nargs='+', type=int, default=[64, 4096])
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=240, help='seconds a batch size may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_keypoints_ab.json'))
    ap.add_argument('--child', type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error('--reps must be at least 5')
    if a.child:
        one_batch(a.child, a.iters, a.reps, a.child_out)
        return 0
    rows = []
    for B in a.batches:      # a fresh process per size, each under its own limit; nothing more is started after a failure
        tmp = '%s.%d.tmp' % (a.out, B)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(B), '--child-out', tmp, '--iters', str(a.iters), '--reps', str(a.reps)],
                           timeout=a.limit)
        if r.returncode != 0:
            print('B=%d failed with exit status %d: stopping' % (B, r.returncode))
            return 1
        rows.append(json.load(open(tmp)))
        os.remove(tmp)
    import torch
    res = dict(tool='tools/fit_keypoints_ab.py', when=time.strftime('%Y-%m-%d %H:%M:%S'), torch=torch.__version__,
               what='ms per call of %d fitting iterations (17 COCO keypoints, synthetic SMPL model): fused = straps_fit_keypoints, one launch; '
                    'composed = rot6d_to_rotmat + SMPL.forward autograd + orthographic_project_torch + torch.optim.Adam' % a.iters,
               timing='device events around a whole call, 1 warm-up, median of %d alternating repetitions' % a.reps, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
