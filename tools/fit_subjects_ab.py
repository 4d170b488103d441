"""Per-launch time of fit_adam_subjects_kernel (csrc/fit_subjects.hip) against fit_adam_kernel (csrc/silfit.hip) on the same inputs, from a kernel
trace: the new kernel replaces the old one for one in a fit loop, so what matters is whether a launch of it costs more -- above all for a subject of
hundreds of frames, whose frames one workgroup walks in rounds.

Sizes: B = 64 as 16 subjects of 4 frames, B = 1 024 as 4 subjects of 256 frames.  Seeded random inputs (oracle/detgen.py), moments given, update = 1.
Every size runs in a child process of its own under `rocprofv3 --kernel-trace --stats` (the program after `--`) and a time limit: --launches
alternating launches of the two kernels after 20 warm-up launches of each, one synchronisation at the end.  The averages are read from the
*kernel_stats.csv of the run; the device's clock report is read before and after (read only).  The first failure ends the run.

    python tools/fit_subjects_ab.py [--launches 500] [--limit 300] [--out profiles/fit_subjects_ab.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((16, 4), (4, 256))      # (subjects, frames per subject)
KERNELS = ('fit_adam_kernel', 'fit_adam_subjects_kernel')


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks', '-d', '0'], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in r.stdout.splitlines() if 'clk' in ln.lower()][:8]
    except Exception as e:      # noqa: BLE001 (the report is a note, not a result)
        return ['unavailable: %s' % e]


def child(G, F, launches, out_path):
    import numpy as np
    import torch
    from detgen import det_uniform
    from straps_amd import hipabi
    from straps_amd.fit import fit_adam_raw, fit_adam_subjects_raw
    dev = torch.device('cuda:0')
    B = G * F
    u = lambda shape, k, lo, hi: torch.from_numpy(det_uniform(shape, 9700 + k, lo, hi)).to(dev)
    est, g_kp, dcam, dx6, dbetas = u((B, 157), 0, -1.0, 1.0), u((B, 157), 1, -1.0, 1.0), u((B, 3), 2, -1.0, 1.0), u((B, 144), 3, -1.0, 1.0), u((B, 10), 4, -1.0, 1.0)
    e_kp, e2 = u((B, 1), 5, 0.1, 1.0), u((B, 2), 6, 0.0, 0.01)
    off = torch.from_numpy((np.arange(G + 1) * F).astype(np.int32)).to(dev)
    opts = hipabi.FitOptsStruct(0, 0, 0.01, 0.01, 0.01, 0.9, 0.999, 1e-8, 0.0, 1e-3, 1e-3, 256.0)
    z = lambda *s: torch.zeros(*s, device=dev)
    a = dict(est=est.clone(), m=z(B, 157), v=z(B, 157), energy=z(B, 1), best=z(B, 157), best_e=z(B))
    b = dict(est=est.clone(), m=z(B, 157), v=z(B, 157), sm=z(G, 10), sv=z(G, 10), energy=z(B, 1), sub=z(G, 1), best=z(B, 157), best_e=z(G))
    before = clocks()
    for i in range(20 + launches):
        fit_adam_raw(opts, a['est'], g_kp, dcam, dx6, dbetas, e_kp, e2, 100.0, 100.0, a['m'], a['v'], a['energy'], 0, None, a['best'], a['best_e'], i, i == 0, True)
        fit_adam_subjects_raw(opts, b['est'], off, None, g_kp, dcam, dx6, dbetas, e_kp, e2, 100.0, 100.0, b['m'], b['v'], b['sm'], b['sv'], b['energy'], 0, b['sub'], None,
                              b['best'], b['best_e'], i, i == 0, True, G)
    torch.cuda.synchronize()
    # cam and pose went the same way in both (the shape did not: it is tied in one of them)
    same = bool(torch.equal(a['est'][:, :147], b['est'][:, :147]))
    with open(out_path, 'w') as f:
        json.dump(dict(batch=B, subjects=G, frames_per_subject=F, launches_each=20 + launches, cam_pose_bits_equal=same, clocks_before=before, clocks_after=clocks()), f)


def kernel_rows(path):
    files = sorted(glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True))
    if not files:
        raise SystemExit('no *kernel_stats.csv under %s' % path)
    out = {}
    for r in csv.DictReader(open(files[-1])):
        for k in KERNELS:
            if k in r.get('Name', ''):      # (neither name is part of the other)
                out[k] = dict(calls=int(r['Calls']), average_us=float(r['AverageNs']) / 1e3, min_us=float(r.get('MinNs', 'nan')) / 1e3, max_us=float(r.get('MaxNs', 'nan')) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=500)
    ap.add_argument('--limit', type=int, default=300, help='seconds a size may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_subjects_ab.json'))
    ap.add_argument('--child', nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default='', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.launches, a.child_out)
        return 0
    rows = []
    for G, F in SIZES:      # a fresh process per size, each under its own limit; nothing more is started after a failure
        d = tempfile.mkdtemp(prefix='fit_subjects_ab_')
        tmp = os.path.join(d, 'child.json')
        cmd = [shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3', '--kernel-trace', '--stats', '-f', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__), '--child', str(G), str(F),
               '--child-out', tmp, '--launches', str(a.launches)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print('%d x %d ran over its limit of %d s: stopping' % (G, F, a.limit))
            return 1
        if rc != 0:
            print('%d x %d failed with exit status %d: stopping' % (G, F, rc))
            return 1
        row = json.load(open(tmp))
        row['kernels'] = kernel_rows(d)
        k = row['kernels']
        if all(n in k for n in KERNELS):
            row['ratio'] = k[KERNELS[1]]['average_us'] / k[KERNELS[0]]['average_us']
        rows.append(row)
        print(json.dumps(row))
    res = dict(tool='tools/fit_subjects_ab.py', when=time.strftime('%Y-%m-%d %H:%M:%S'),
               what='per-launch time (rocprofv3 --kernel-trace --stats, microseconds) of fit_adam_subjects_kernel against fit_adam_kernel on the same seeded inputs, '
                    'update = 1; ratio = new / old', rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
