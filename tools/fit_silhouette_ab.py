"""A/B of 20 iterations of silhouette fitting at 256 x 256: `SilhouetteFitter` (straps_distance_field once, then per iteration rot6d forward,
SMPL forward, straps_silhouette_energy, SMPL backward, rot6d backward, straps_fit_keypoints with iters = 0, straps_fit_adam) vs the same
loop written in torch ops under autograd -- rot6d_to_rotmat, SMPL.forward, gather-based bilinear sampling of sqrt(d2), torch.cdist + min for
the nearest projected vertex of every lattice point (in chunks of bodies, without a graph: only the gathered nearest vertex is differentiated,
what autograd would keep of the min anyway), the priors, torch.optim.Adam on one [B,157] tensor.  No keypoints: the silhouette and the priors
alone.  Both read the same distance field.  Lattice 4, tau 1.5, weights 100, lambda 1e-3, lr 0.01, the synthetic model; targets are
WeakPerspectiveSilhouetteRenderer masks of seeded bodies (oracle/detgen.py, put on sys.path here: the tool runs from a checkout).  The largest
difference of the final parameters and energies is reported, not asserted (the two pick the nearest vertex on differently rounded distances).

Timing: one warm-up call of each, then --reps (>= 5) timed calls of each, alternating, device events around a whole call; medians.  The
device's clock report is read before and after (read only).  Every batch size runs in a child process of its own under a time limit; the
first failure ends the run.  Writes profiles/fit_silhouette_ab.json.

    python tools/fit_silhouette_ab.py [--batches 64 1024] [--iters 20] [--reps 5] [--limit 400]

The kernels' own times come from a trace of the fitter alone, one size per run:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/fit_silhouette_ab.py --child 64 --only fitter --child-out /dev/null
and `--kernel-stats B=DIR [B=DIR ...]` merges the rows of the *kernel_stats.csv found under DIR into the JSON that exists.
"""
import argparse
import csv
import glob
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

WH, LATTICE, TAU, W_IN, W_OUT, LAM, LR = 256, 4, 1.5, 100.0, 100.0, 1e-3, 0.01


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks', '-d', '0'], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in r.stdout.splitlines() if 'clk' in ln.lower()][:8]
    except Exception as e:      # noqa: BLE001 (the report is a note, not a result)
        return ['unavailable: %s' % e]


def inputs(B, dev, smpl):
    """-> (start [B,157], target masks uint8 [B,256,256]): the mean parameters, and the silhouettes of seeded bodies near them"""
    import torch
    import straps_amd
    from detgen import det_uniform
    mp = straps_amd.synthetic_mean_params(0)
    mean = torch.cat([torch.tensor([0.9, 0.0, 0.0]), torch.from_numpy(mp['pose']), torch.from_numpy(mp['shape'])]).to(dev)
    u = lambda shape, k, lo, hi: torch.from_numpy(det_uniform(shape, 9100 + k, lo, hi)).to(dev)
    start = mean[None].repeat(B, 1).contiguous()
    true = start.clone()
    true[:, 3:147] += u((B, 144), 1, -0.08, 0.08)
    true[:, 147:] += u((B, 10), 2, -1.7, 1.7)
    with torch.no_grad():
        R = straps_amd.rot6d_to_rotmat(true[:, 3:147].contiguous()).view(B, 24, 3, 3)
        verts, _ = smpl.forward_arrays(true[:, 147:].contiguous(), R, want_joints=False)
        masks = straps_amd.WeakPerspectiveSilhouetteRenderer(smpl.faces, img_wh=WH).to(dev)(verts, true[:, :3].contiguous())
    return start, masks


def one_batch(B, iters, reps, out_path, only):
    import torch
    import straps_amd
    from straps_amd import cam_utils
    dev = torch.device('cuda:0')
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=1).to(dev)
    start, masks = inputs(B, dev, smpl)
    fitter = straps_amd.SilhouetteFitter(smpl, iters=iters, lr=LR, lattice=LATTICE, tau=TAU, w_in=W_IN, w_out=W_OUT, lambda_pose=LAM, lambda_shape=LAM, img_wh=WH)
    cam0, pose0, shape0 = start[:, :3].contiguous(), start[:, 3:147].contiguous(), start[:, 147:].contiguous()
    res = {}

    def fitter_call():
        o = fitter(cam0, pose0, shape0, masks)
        res['fitter'] = (torch.cat([o['cam_wp'], o['pose'], o['shape']], 1), o['energy0'], o['energy'])

    # ---- the torch loop
    idx = torch.arange(0, WH, LATTICE, device=dev)
    ii, jj = torch.meshgrid(idx, idx, indexing='ij')
    pts = torch.stack([jj.reshape(-1), ii.reshape(-1)], 1).float()                       # [P,2] = (column, row)
    valid = masks[:, ii.reshape(-1), jj.reshape(-1)] != 0                                 # [B,P]
    n_valid = valid.sum(1).clamp_min(1).float()
    nonempty = (masks.reshape(B, -1) != 0).any(1).float()
    chunk = max(1, min(B, 32))

    def energy(est, D):
        R = straps_amd.rot6d_to_rotmat(est[:, 3:147]).view(B, 24, 3, 3)
        out = smpl(betas=est[:, 147:], body_pose=R[:, 1:], global_orient=R[:, :1], pose2rot=False)
        g = (cam_utils.orthographic_project_torch(out.vertices, est[:, :3]) + 1.0) * (WH / 2.0) - 0.5      # [B,N,2]
        q = g.clamp(0.0, WH - 1.0)
        off = g - q
        o = (off ** 2).sum(-1).clamp_min(1e-30).sqrt() * ((off != 0).any(-1)).float()
        cell = q.detach().floor().clamp(max=WH - 2.0)
        f = q - cell
        base = (cell[..., 1] * WH + cell[..., 0]).long()
        Df = D.reshape(B, -1)
        d00, d01, d10, d11 = (Df.gather(1, base + k) for k in (0, 1, WH, WH + 1))
        fx, fy = f[..., 0], f[..., 1]
        Dv = (1 - fy) * ((1 - fx) * d00 + fx * d01) + fy * ((1 - fx) * d10 + fx * d11)
        e_in = (((Dv + o) * (2.0 / WH)) ** 2).mean(1)
        with torch.no_grad():
            near = torch.cat([torch.cdist(pts[None].expand(min(chunk, B - a), -1, -1), g[a:a + chunk]).min(2).indices for a in range(0, B, chunk)])
        gn = g.gather(1, near[:, :, None].expand(-1, -1, 2))
        r = ((gn - pts[None]) ** 2).sum(-1).clamp_min(1e-30).sqrt()
        h = (r - TAU).clamp_min(0.0) * (2.0 / WH) * valid.float()
        e_out = (h ** 2).sum(1) / n_valid
        prior = LAM * ((est[:, 3:147] - start[:, 3:147]) ** 2).sum(1) + LAM * ((est[:, 147:] - start[:, 147:]) ** 2).sum(1)
        return prior + nonempty * (W_IN * e_in + W_OUT * e_out)

    def torch_loop():
        D = straps_amd.distance_field(masks).float().sqrt()
        est = start.clone().requires_grad_(True)
        opt = torch.optim.Adam([est], lr=LR)
        e0 = None
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            E = energy(est, D)
            e0 = E.detach() if e0 is None else e0
            E.sum().backward()
            opt.step()
        with torch.no_grad():
            res['torch'] = (est.detach(), e0, energy(est, D))

    fns = {'fitter': fitter_call, 'torch': torch_loop}
    if only:
        fns = {only: fns[only]}
    before = clocks()
    for f in fns.values():      # warm-up: code objects, allocator, autograd state
        f()
    torch.cuda.synchronize()
    row = dict(batch=B, iters=iters)
    if not only:
        row['max_abs_param_diff'] = float((res['fitter'][0] - res['torch'][0]).abs().max())
        row['start_energy_rel_diff'] = float(((res['fitter'][1] - res['torch'][1]).abs() / res['torch'][1].abs().clamp_min(1e-30)).max())
        row['final_energy_rel_diff'] = float(((res['fitter'][2] - res['torch'][2]).abs() / res['torch'][2].abs().clamp_min(1e-30)).max())
        row['mean_final_over_start_energy'] = float((res['fitter'][2] / res['fitter'][1]).mean())
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
    row.update(ms=med, ms_all=times, clocks_before=before, clocks_after=clocks())
    if not only:
        row['speedup'] = med['torch'] / med['fitter']
    print('B=%-5d %s' % (B, '   '.join('%s %9.3f ms' % kv for kv in med.items())) + ('' if only else '   x%.2f   |est diff| %.2e   E_n/E_0 ~ %.3f'
                                                                                    % (row['speedup'], row['max_abs_param_diff'], row['mean_final_over_start_energy'])), flush=True)
    with open(out_path, 'w') as f:
        json.dump(row, f)


def kernel_stats(path):
    """rows of a rocprofv3 *kernel_stats.csv for the kernels of csrc/silfit.hip, csrc/fit.hip and the SMPL forward / backward"""
    files = sorted(glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True))
    if not files:
        raise SystemExit('no *kernel_stats.csv under %s' % path)
    rows = []
    for r in csv.DictReader(open(files[-1])):
        name = r.get('Name', '')
        short = name.replace('(anonymous namespace)::', '')
        short = (short[5:] if short.startswith('void ') else short).split('(')[0].split('<')[0].split('::')[-1]
        rows.append(dict(kernel=short, calls=int(r['Calls']), total_us=float(r['TotalDurationNs']) / 1e3, average_us=float(r['AverageNs']) / 1e3,
                         percent=float(r['Percentage'])))
    return sorted(rows, key=lambda r: -r['total_us'])[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', nargs='+', type=int, default=[64, 1024])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=400, help='seconds a batch size may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_silhouette_ab.json'))
    ap.add_argument('--only', choices=['fitter', 'torch'], default=None, help='time one side alone (for a kernel trace)')
    ap.add_argument('--kernel-stats', nargs='+', default=None, metavar='B=DIR', help='merge rocprofv3 kernel statistics into the existing JSON and exit')
    ap.add_argument('--child', type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out))
        for item in a.kernel_stats:
            b, d = item.split('=', 1)
            for row in res['rows']:
                if row['batch'] == int(b):
                    row['kernel_trace'] = kernel_stats(d)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print('merged kernel statistics into', a.out)
        return 0
    if a.reps < 5 and not a.only:
        ap.error('--reps must be at least 5')
    if a.child:
        one_batch(a.child, a.iters, a.reps, a.child_out, a.only)
        return 0
    rows = []
    for B in a.batches:      # a fresh process per size, each under its own limit; nothing more is started after a failure
        tmp = '%s.%d.tmp' % (a.out, B)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(B), '--child-out', tmp, '--iters', str(a.iters), '--reps', str(a.reps)]
                                + (['--only', a.only] if a.only else []), timeout=a.limit).returncode
        except subprocess.TimeoutExpired:      # (subprocess.run has killed and reaped the child)
            print('B=%d ran over its limit of %d s: stopping' % (B, a.limit))
            return 1
        if rc != 0:
            print('B=%d failed with exit status %d: stopping' % (B, rc))
            return 1
        rows.append(json.load(open(tmp)))
        os.remove(tmp)
    import torch
    res = dict(tool='tools/fit_silhouette_ab.py', when=time.strftime('%Y-%m-%d %H:%M:%S'), torch=torch.__version__,
               what='ms per call of %d silhouette-fitting iterations at %d x %d (lattice %d, synthetic SMPL model, no keypoints): fitter = SilhouetteFitter '
                    '(straps_distance_field + per iteration seven entry points); torch = rot6d_to_rotmat + SMPL.forward autograd + gather-based bilinear '
                    'sampling + torch.cdist/min + torch.optim.Adam' % (a.iters, WH, WH, LATTICE),
               timing='device events around a whole call, 1 warm-up, median of %d alternating repetitions' % a.reps, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
