#!/usr/bin/env python
"""tools/measure_bwd_profile.py [--bodies 64] [--calls 50] [--fit-iters 20] [--out FILE] -- the shape behind the figures of DESIGN.md section 7:
straps_measure_mesh and straps_measure_mesh_bwd on T-pose bodies of the synthetic model with the default measurements, `calls` times each after a
warm-up, and one MeasurementFitter call.

Run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure_bwd_profile.py` for the kernel times (measure_partial_kernel,
measure_finish_kernel, measure_bwd_partial_kernel, measure_bwd_gather_kernel: averages over the calls), and on its own for the event-timed
figures it prints as one JSON line: microseconds per forward call, per backward call and per fit iteration (a fit of `fit-iters` updates is
fit-iters + 1 evaluations; the time is divided by that).  Synthetic model only: its faces are a triangle soup."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import straps_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bodies', type=int, default=64)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--fit-iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B = a.bodies
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=B).to(dev)
    measurer = straps_amd.BodyMeasurer.from_smpl(smpl).to(dev)
    betas = torch.from_numpy(np.random.RandomState(0).uniform(-2, 2, (B, 10)).astype(np.float32)).to(dev)
    eye = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    verts, joints = smpl.forward_arrays(betas, eye)
    dvalues = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (B, len(measurer.names))).astype(np.float32)).to(dev)

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n
    res = {'device': torch.cuda.get_device_name(0), 'bodies': B, 'vertices': int(verts.shape[1]), 'faces': int(measurer.faces.shape[0]),
           'measurements': len(measurer.names), 'calls': a.calls,
           'measure_mesh_us_per_call': timed(lambda: measurer.measure_arrays(verts, joints), a.calls),
           'measure_mesh_bwd_us_per_call': timed(lambda: measurer.measure_grad(verts, joints, dvalues), a.calls)}
    fitter = straps_amd.MeasurementFitter(smpl, measurer, iters=a.fit_iters)
    targets = measurer.measure_arrays(verts, joints) * 1.05
    start = torch.zeros(B, 10, device=dev)
    res['fit_iters'] = a.fit_iters
    res['fit_us_per_iteration'] = timed(lambda: fitter(start, targets), 3) / (a.fit_iters + 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
