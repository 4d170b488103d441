"""Timing of the gradient of the tape-measure girths on the GPU (profiles/measure_tape_bwd_b64.json was filled from its output).

    python tools/measure_tape_bwd_profile.py [--batch 64] [--iters 1000] [--out profiles/measure_tape_bwd_b64.json]

T-pose bodies of the synthetic SMPL model (template + shape directions at random betas, 6890 vertices, 13 776 faces) and their joints, the
seven planes of measure.tape_measurements(), `iters` calls back to back between two device events after a warm-up, on preallocated outputs
and workspaces, all in one process:
    straps_measure_tape (the forward) and straps_measure_tape_bwd at the worst-case capacity and at a capacity just above the largest count;
    straps_measure_tape_bwd with the same planes as SECTION (no march), and with dout == 0 everywhere (what an all-unknown row costs);
    one fit.MeasurementFitter iteration (its evaluating entry points and straps_fit_adam) with the default set -- the existing fit -- and
    with the seven tape girths plus the height.
Before anything is timed the backward's `values` are compared with the forward's bit for bit.  A rocprofv3 --kernel-trace --stats run of
this tool gives the three kernels separately.  Prints one JSON line and, with --out, writes it there.  There is no parent to compare
against and no speed bar.  The synthetic model's faces are a triangle soup that a plane cuts far more often than it would cut a body
surface (`largest_count`), and the soup's section is loose segments whose hull has more corners than a body's: these times are an upper
bound for a real SMPL mesh, which nobody has measured."""
import argparse
import collections
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import straps_amd                      # noqa: E402
from straps_amd import hipabi, measure      # noqa: E402
from straps_amd.fit import NE, MeasurementFitter, fit_adam_raw      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda:0')
    L = hipabi.load()
    B = args.batch
    model = straps_amd.synthetic_smpl_model(0)
    rng = np.random.RandomState(7)
    betas = rng.uniform(-2, 2, (B, 10))
    v = model['v_template'].astype(np.float64)[None] + np.einsum('vcl,bl->bvc', model['shapedirs'].astype(np.float64), betas)
    joints = np.einsum('jv,bvc->bjc', model['J_regressor'].astype(np.float64), v)
    verts, joints = torch.from_numpy(v.astype(np.float32)).to(dev), torch.from_numpy(joints.astype(np.float32)).to(dev)
    specs = measure.tape_measurements()
    m = straps_amd.BodyMeasurer(model['faces'], model['face_parts'], specs, num_vertices=6890, tape_gradients=True).to(dev)
    N, F, M = verts.shape[1], m.faces.shape[0], len(m.specs)
    hull, n_points = measure.tape_structs(m.specs, N)
    section, _ = measure.tape_structs([s._replace(kind=measure.TAPE_KINDS[1]) for s in m.specs], N)
    points = joints[:, :n_points].contiguous()
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out, values = f32(B, M), f32(B, M)
    counts = torch.empty(B, M, dtype=torch.int32, device=dev)
    dout = torch.from_numpy(rng.uniform(0.5, 2.0, (B, M)).astype(np.float32)).to(dev)
    zero_dout = torch.zeros_like(dout)
    dverts, dpoints = f32(B, N, 3), torch.zeros(B, 90, 3, device=dev)
    ws = torch.empty(L.straps_measure_tape_workspace_bytes(B, F, M, 0) // 8, dtype=torch.float64, device=dev)
    ws_bytes = L.straps_measure_tape_bwd_workspace_bytes(B, N, F, M, 0)
    ws_b = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    head = (hipabi.ptr(verts), hipabi.ptr(points), hipabi.ptr(m.faces), hipabi.ptr(m.face_parts))
    fwd = lambda cap: L.straps_measure_tape(*head, hull, hipabi.ptr(out), None, hipabi.ptr(ws), B, N, n_points, F, M, cap, hipabi.stream_ptr())
    bwd = lambda arr, d, val, cnt, cap: L.straps_measure_tape_bwd(*head, hipabi.ptr(m.vf_offsets), hipabi.ptr(m.vf_faces), arr, hipabi.ptr(d), hipabi.ptr(dverts),
                                                                  hipabi.ptr(dpoints), hipabi.ptr(val), hipabi.ptr(cnt), hipabi.ptr(ws_b), B, N, n_points, 90, F, M, cap, 0,
                                                                  hipabi.stream_ptr())

    def timed(fn, iters):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    hipabi.check(fwd(0), 'straps_measure_tape')
    hipabi.check(bwd(hull, dout, values, counts, 0), 'straps_measure_tape_bwd')
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), values.view(torch.int32)) and bool(torch.isfinite(dverts).all()) and bool(dverts.any())
    largest = int(counts.max())
    tight = min(2 * F, (largest + 63) // 64 * 64)
    touched = float((dverts != 0).any(2).sum(1).float().mean())
    us_fwd = timed(lambda: fwd(0), args.iters)
    us_bwd = timed(lambda: bwd(hull, dout, None, None, 0), args.iters)
    us_bwd_values = timed(lambda: bwd(hull, dout, values, counts, 0), args.iters)
    us_fwd_tight = timed(lambda: fwd(tight), args.iters)
    us_bwd_tight = timed(lambda: bwd(hull, dout, None, None, tight), args.iters)
    us_bwd_section = timed(lambda: bwd(section, dout, None, None, 0), args.iters)
    us_bwd_zero = timed(lambda: bwd(hull, zero_dout, None, None, 0), args.iters)

    # one MeasurementFitter iteration: the evaluating entry points and the Adam update, on the fitter's own buffers
    smpl = straps_amd.SMPL(model, batch_size=1).to(dev)

    def fit_iteration_us(measurer):
        fitter = MeasurementFitter(smpl, measurer)
        shape = torch.from_numpy(betas.astype(np.float32)).to(dev)
        with torch.no_grad():
            targets = measurer(verts, joints)['values'] * 1.05
        est, est0, targets, weights = fitter._inputs(shape, targets, None, None)
        buf = fitter._buffers(B, dev)
        mom, var = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev)
        energy, best, best_e = f32(B, 2), f32(B, NE), f32(B)
        opts = fitter.opts()

        def step():
            fitter._terms(est, est0, targets, weights, buf)
            fit_adam_raw(opts, est, buf['g'], None, None, buf['dbetas'], buf['e'], None, 0.0, 0.0, mom, var, energy, 0, None, best, best_e, 0, True, True)
        return timed(step, max(1, args.iters // 4))
    us_fit_default = fit_iteration_us(straps_amd.BodyMeasurer.from_smpl(smpl).to(dev))
    tape_set = collections.OrderedDict(list(specs.items()) + [('height', measure.extent((0.0, 1.0, 0.0)))])
    us_fit_tape = fit_iteration_us(straps_amd.BodyMeasurer.from_smpl(smpl, tape_set, tape_gradients=True).to(dev))
    res = {'what': 'straps_measure_tape_bwd on T-pose bodies of the synthetic SMPL model with measure.tape_measurements() (seven planes); device events '
                   'over back-to-back calls; beside it the forward straps_measure_tape and one fit.MeasurementFitter iteration, same process, same '
                   "inputs.  The synthetic model's triangle soup cuts far more faces per plane than a body surface would: an upper bound for a real SMPL mesh",
           'device': torch.cuda.get_device_name(0), 'batch': B, 'nverts': N, 'nfaces': F, 'n_meas': M, 'n_points': n_points, 'iters': args.iters,
           'us_per_call_forward_worst_case_capacity': round(us_fwd, 2), 'us_per_call_backward_worst_case_capacity': round(us_bwd, 2),
           'ratio_backward_to_forward': round(us_bwd / us_fwd, 2), 'us_per_call_backward_with_values_and_counts': round(us_bwd_values, 2),
           'us_per_call_forward_tight_capacity': round(us_fwd_tight, 2), 'us_per_call_backward_tight_capacity': round(us_bwd_tight, 2),
           'us_per_call_backward_section_no_march': round(us_bwd_section, 2), 'us_per_call_backward_all_dout_zero': round(us_bwd_zero, 2),
           'us_per_fit_iteration_default_set': round(us_fit_default, 2), 'us_per_fit_iteration_tape_set_plus_height': round(us_fit_tape, 2),
           'workspace_bytes_worst_case': int(ws_bytes), 'workspace_bytes_tight': int(L.straps_measure_tape_bwd_workspace_bytes(B, N, F, M, tight)),
           'tight_capacity': tight, 'largest_count': largest, 'largest_count_per_measurement': [int(x) for x in counts.max(0).values.tolist()],
           'worst_case_count': 2 * F, 'mean_vertices_with_a_gradient_per_body': round(touched, 1), 'names': list(m.names)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
