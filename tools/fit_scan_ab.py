"""A/B of 20 iterations of fitting the body to a 3-D scan: `ScanFitter` (per iteration rot6d forward, SMPL forward, straps_scan_energy, SMPL
backward, rot6d backward, straps_fit_keypoints with iters = 0 for the priors, straps_fit_adam) vs the same loop written in torch ops under
autograd on the same library -- rot6d_to_rotmat, SMPL.forward, torch.cdist + min in chunks of bodies for both directions of the nearest-point
search (without a graph: only the gathered partners are differentiated, what autograd would keep of the min anyway), the priors,
torch.optim.Adam on one [B,157] tensor.  Weights 100 and 100, sigma 0, lambda 1e-3, lr 0.01, the synthetic model.  The scans are points drawn
on the faces of seeded posed bodies (a face by its index, a place on it by barycentric coordinates: oracle/detgen.py, put on sys.path here --
the tool runs from a checkout), moved by a seeded offset of up to 2 mm per axis; the start is the mean body at the scan's centroid.  The
largest difference of the final parameters and energies is reported, not asserted (the two pick partners on differently rounded distances).

Timing: one warm-up call of each, then --reps (>= 5) timed calls of each, alternating, device events around a whole call; medians.  The
device's clock report is read before and after (read only).  Every shape runs in a child process of its own under a time limit; the first
failure ends the run.  Writes profiles/fit_scan_ab.json.

    python tools/fit_scan_ab.py [--shapes 1x65536 64x16384] [--iters 20] [--reps 5] [--limit 400]

The kernels' own times come from a trace of the fitter alone, one shape per run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fit_scan_ab.py --child 64x16384 --only fitter --child-out /dev/null
and `--kernel-stats 64x16384=DIR [...]` merges the rows of the *kernel_stats.csv found under DIR into the JSON that exists, with the share of
the two search kernels and their distance evaluations per second (2 * B * points * 6890 per evaluation of the energy, over their time)
beside the fp32 vector rate of the chip.
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

W_S2M, W_M2S, SIGMA, LAM, LR, NOISE = 100.0, 100.0, 0.0, 1e-3, 0.01, 2e-3
NVERTS = 6890
FP32_VECTOR_FLOPS = 157.3e12      # MI355X: peak fp32 vector rate (one fused multiply-add = 2)
OPS_PER_DISTANCE = 8              # floating-point operations of one squared distance: three differences, one product, two fused multiply-adds


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks', '-d', '0'], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in r.stdout.splitlines() if 'clk' in ln.lower()][:8]
    except Exception as e:      # noqa: BLE001 (the report is a note, not a result)
        return ['unavailable: %s' % e]


def inputs(B, P, dev, smpl):
    """-> (start [B,157] with the translation at the scan's centroid, points [B,P,3]): scans of seeded bodies near the mean parameters"""
    import torch
    import straps_amd
    from detgen import det_uniform
    mp = straps_amd.synthetic_mean_params(0)
    mean = torch.cat([torch.zeros(3), torch.from_numpy(mp['pose']), torch.from_numpy(mp['shape'])]).to(dev)
    u = lambda shape, k, lo, hi: torch.from_numpy(det_uniform(shape, 9300 + k, lo, hi)).to(dev)
    start = mean[None].repeat(B, 1).contiguous()
    true = start.clone()
    true[:, :3] = u((B, 3), 0, -0.3, 0.3)
    true[:, 3:147] += u((B, 144), 1, -0.08, 0.08)
    true[:, 147:] += u((B, 10), 2, -1.7, 1.7)
    with torch.no_grad():
        R = straps_amd.rot6d_to_rotmat(true[:, 3:147].contiguous()).view(B, 24, 3, 3)
        verts, _ = smpl.forward_arrays(true[:, 147:].contiguous(), R, want_joints=False)
        verts = verts + true[:, None, :3]
        faces = torch.from_numpy(smpl.faces.astype('int64')).to(dev)
        pick = (u((B, P), 3, 0.0, 1.0) * faces.shape[0]).long().clamp(max=faces.shape[0] - 1)
        a, b = u((B, P, 1), 4, 0.0, 1.0), u((B, P, 1), 5, 0.0, 1.0)
        flip = (a + b) > 1.0
        a, b = torch.where(flip, 1.0 - a, a), torch.where(flip, 1.0 - b, b)
        tri = faces[pick]                                                              # [B,P,3]
        corner = lambda k: verts.gather(1, tri[:, :, k:k + 1].expand(-1, -1, 3))
        points = (corner(0) + a * (corner(1) - corner(0)) + b * (corner(2) - corner(0)) + u((B, P, 3), 6, -NOISE, NOISE)).contiguous()
        start[:, :3] = points.mean(dim=1) - (verts - true[:, None, :3]).mean(dim=1)
    return start, points


def one_shape(B, P, iters, reps, out_path, only):
    import torch
    import straps_amd
    dev = torch.device('cuda:0')
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=1).to(dev)
    start, points = inputs(B, P, dev, smpl)
    fitter = straps_amd.ScanFitter(smpl, iters=iters, lr=LR, sigma=SIGMA, w_s2m=W_S2M, w_m2s=W_M2S, lambda_pose=LAM, lambda_shape=LAM)
    t0, pose0, shape0 = start[:, :3].contiguous(), start[:, 3:147].contiguous(), start[:, 147:].contiguous()
    res = {}

    def fitter_call():
        o = fitter(t0, pose0, shape0, points)
        res['fitter'] = (torch.cat([o['transl'], o['pose'], o['shape']], 1), o['energy0'], o['energy'])

    # ---- the torch loop
    chunk = max(1, min(B, (1 << 29) // (P * NVERTS)))      # bodies per cdist: at most 2 GiB of distances at a time

    def energy(est):
        R = straps_amd.rot6d_to_rotmat(est[:, 3:147]).view(B, 24, 3, 3)
        out = smpl(betas=est[:, 147:], body_pose=R[:, 1:], global_orient=R[:, :1], pose2rot=False)
        X = out.vertices + est[:, None, :3]
        with torch.no_grad():
            nv, npt = [], []
            for a in range(0, B, chunk):
                d = torch.cdist(points[a:a + chunk], X[a:a + chunk])      # [c,P,V]
                nv.append(d.min(2).indices)
                npt.append(d.min(1).indices)
            nv, npt = torch.cat(nv), torch.cat(npt)
        e_s = ((X.gather(1, nv[:, :, None].expand(-1, -1, 3)) - points) ** 2).sum(-1).mean(1)
        e_m = ((X - points.gather(1, npt[:, :, None].expand(-1, -1, 3))) ** 2).sum(-1).mean(1)
        prior = LAM * ((est[:, 3:147] - start[:, 3:147]) ** 2).sum(1) + LAM * ((est[:, 147:] - start[:, 147:]) ** 2).sum(1)
        return prior + W_S2M * e_s + W_M2S * e_m

    def torch_loop():
        est = start.clone().requires_grad_(True)
        opt = torch.optim.Adam([est], lr=LR)
        e0 = None
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            E = energy(est)
            e0 = E.detach() if e0 is None else e0
            E.sum().backward()
            opt.step()
        with torch.no_grad():
            res['torch'] = (est.detach(), e0, energy(est))

    fns = {'fitter': fitter_call, 'torch': torch_loop}
    if only:
        fns = {only: fns[only]}
    before = clocks()
    for f in fns.values():      # warm-up: code objects, allocator, autograd state
        f()
    torch.cuda.synchronize()
    row = dict(batch=B, points=P, iters=iters, distance_evaluations_per_call=2 * B * P * NVERTS * (iters + 1))
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
    print('B=%-3d P=%-6d %s' % (B, P, '   '.join('%s %9.3f ms' % kv for kv in med.items())) + ('' if only else '   x%.2f   |est diff| %.2e   E_n/E_0 ~ %.3f'
                                                                                               % (row['speedup'], row['max_abs_param_diff'], row['mean_final_over_start_energy'])), flush=True)
    with open(out_path, 'w') as f:
        json.dump(row, f)


def kernel_stats(path):
    """rows of a rocprofv3 *kernel_stats.csv, the sixteen largest; the two instances of the search keep their template argument"""
    files = sorted(glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True))
    if not files:
        raise SystemExit('no *kernel_stats.csv under %s' % path)
    rows = []
    for r in csv.DictReader(open(files[-1])):
        name = r.get('Name', '')
        short = name.replace('(anonymous namespace)::', '')
        short = (short[5:] if short.startswith('void ') else short).split('(')[0]
        base = short.split('<')[0].split('::')[-1]
        if base == 'scan_search_kernel' and '<' in short:
            base += '<' + short.split('<', 1)[1].split('>')[0] + '>'
        rows.append(dict(kernel=base, calls=int(r['Calls']), total_us=float(r['TotalDurationNs']) / 1e3, average_us=float(r['AverageNs']) / 1e3,
                         percent=float(r['Percentage'])))
    return sorted(rows, key=lambda r: -r['total_us'])[:16]


def search_summary(row, trace):
    """the search kernels' share of the traced kernel time and their achieved rate, from a trace of `--only fitter` (warm-up + reps calls)"""
    search = [r for r in trace if r['kernel'].startswith('scan_search_kernel')]
    if not search:
        return None
    us, calls = sum(r['total_us'] for r in search), sum(r['calls'] for r in search)
    evals = calls * row['batch'] * row['points'] * NVERTS      # one launch of either instance evaluates the whole B x points x 6890 matrix once
    rate = evals / (us * 1e-6)
    return dict(share_of_traced_kernel_time=sum(r['percent'] for r in search) / 100.0, launches=calls, total_us=us, distance_evaluations_per_second=rate,
                fp32_vector_flops=FP32_VECTOR_FLOPS, flops_per_distance=OPS_PER_DISTANCE,
                share_of_fp32_vector_rate=rate * OPS_PER_DISTANCE / FP32_VECTOR_FLOPS)


def parse_shape(s):
    b, p = s.lower().split('x')
    return int(b), int(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['1x65536', '64x16384'], metavar='BxP')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=400, help='seconds a shape may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_scan_ab.json'))
    ap.add_argument('--only', choices=['fitter', 'torch'], default=None, help='time one side alone (for a kernel trace)')
    ap.add_argument('--kernel-stats', nargs='+', default=None, metavar='BxP=DIR', help='merge rocprofv3 kernel statistics into the existing JSON and exit')
    ap.add_argument('--child', default='', help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out))
        for item in a.kernel_stats:
            shape, d = item.split('=', 1)
            for row in res['rows']:
                if (row['batch'], row['points']) == parse_shape(shape):
                    row['kernel_trace'] = kernel_stats(d)
                    row['search_kernels'] = search_summary(row, row['kernel_trace'])
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print('merged kernel statistics into', a.out)
        return 0
    if a.reps < 5 and not a.only:
        ap.error('--reps must be at least 5')
    if a.child:
        B, P = parse_shape(a.child)
        one_shape(B, P, a.iters, a.reps, a.child_out, a.only)
        return 0
    rows = []
    for shape in a.shapes:      # a fresh process per shape, each under its own limit; nothing more is started after a failure
        tmp = '%s.%s.tmp' % (a.out, shape)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', shape, '--child-out', tmp, '--iters', str(a.iters), '--reps', str(a.reps)]
                                + (['--only', a.only] if a.only else []), timeout=a.limit).returncode
        except subprocess.TimeoutExpired:      # (subprocess.run has killed and reaped the child)
            print('%s ran over its limit of %d s: stopping' % (shape, a.limit))
            return 1
        if rc != 0:
            print('%s failed with exit status %d: stopping' % (shape, rc))
            return 1
        rows.append(json.load(open(tmp)))
        os.remove(tmp)
    import torch
    res = dict(tool='tools/fit_scan_ab.py', when=time.strftime('%Y-%m-%d %H:%M:%S'), torch=torch.__version__,
               what='ms per call of %d scan-fitting iterations (synthetic SMPL model, 6890 vertices, weights 100 / 100, sigma 0): fitter = ScanFitter (per '
                    'iteration seven entry points); torch = rot6d_to_rotmat + SMPL.forward autograd + torch.cdist/min in chunks + torch.optim.Adam' % a.iters,
               timing='device events around a whole call, 1 warm-up, median of %d alternating repetitions' % a.reps, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
