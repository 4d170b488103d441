"""Timing of the tape-measure girths on the GPU (profiles/measure_tape_b64.json was filled from its output).

    python tools/measure_tape_profile.py [--batch 64] [--iters 1000] [--out profiles/measure_tape_b64.json]

T-pose bodies of the synthetic SMPL model (template + shape directions at random betas, 6890 vertices, 13 776 faces) and their joints are
measured with measure.tape_measurements() -- the seven girth planes of the default set as tape girths -- `iters` times back to back
between two device events after a warm-up, on a preallocated output and workspace:
    straps_measure_tape, all HULL, at the worst-case capacity and at a capacity just above the largest count seen;
    straps_measure_tape with the same planes as SECTION (the collect kernel alone, and without its point stores);
    straps_measure_mesh with the same planes as GIRTH, in the same process (the call DESIGN.md times at 37.9 us with the fifteen defaults);
    BodyMeasurer.forward, which allocates output and workspace, at both capacities.
The hull kernel's time is reported as HULL call minus SECTION call: an estimate (the SECTION call skips the stores); a rocprofv3
--kernel-trace --stats run of this tool gives the two kernels separately.  The results are compared with each other before anything is
timed: SECTION against GIRTH, BodyMeasurer against the raw call.  Prints one JSON line and, with --out, writes it there.  There is no parent to compare
against and no speed bar.  The synthetic model's faces are a triangle soup that a plane cuts far more often than it would cut a body
surface (see `largest_count`): these times are an upper bound for a real SMPL mesh, which nobody has measured."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import straps_amd                      # noqa: E402
from straps_amd import hipabi, measure      # noqa: E402


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
    m = straps_amd.BodyMeasurer(model['faces'], model['face_parts'], specs).to(dev)
    N, F, M = verts.shape[1], m.faces.shape[0], len(m.specs)
    hull, n_points = measure.tape_structs(m.specs, N)
    section, _ = measure.tape_structs([s._replace(kind=measure.TAPE_KINDS[1]) for s in m.specs], N)
    girth, _ = measure.measure_structs([measure.girth(s.anchors[0], s.direction, s.parts) for s in m.specs], N)
    points = joints[:, :n_points].contiguous()
    out, out_s, out_g = (torch.empty(B, M, dtype=torch.float32, device=dev) for _ in range(3))
    counts = torch.empty(B, M, dtype=torch.int32, device=dev)
    ws_bytes = L.straps_measure_tape_workspace_bytes(B, F, M, 0)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    ws_g = torch.empty(L.straps_measure_workspace_bytes(B, N, F, M) // 8, dtype=torch.float64, device=dev)
    head = (hipabi.ptr(verts), hipabi.ptr(points), hipabi.ptr(m.faces), hipabi.ptr(m.face_parts))
    tape_call = lambda arr, o, c, cap: L.straps_measure_tape(*head, arr, hipabi.ptr(o), hipabi.ptr(c), hipabi.ptr(ws), B, N, n_points, F, M, cap, hipabi.stream_ptr())
    girth_call = lambda: L.straps_measure_mesh(*head, girth, hipabi.ptr(out_g), hipabi.ptr(ws_g), B, N, n_points, F, M, hipabi.stream_ptr())

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

    hipabi.check(tape_call(hull, out, counts, 0), 'straps_measure_tape')
    hipabi.check(tape_call(section, out_s, None, 0), 'straps_measure_tape')
    hipabi.check(girth_call(), 'straps_measure_mesh')
    torch.cuda.synchronize()
    largest = int(counts.max())
    tight = min(2 * F, (largest + 63) // 64 * 64)
    rel = float(((out_s - out_g).abs() / out_g.abs().clamp_min(1e-6)).max())
    assert rel < 1e-6 and bool(torch.isfinite(out).all()) and bool((out > 0).all()), rel
    m_tight = straps_amd.BodyMeasurer(model['faces'], model['face_parts'], specs, tape_capacity=tight).to(dev)
    assert torch.equal(m(verts, joints)['values'], out) and torch.equal(m_tight(verts, joints)['values'], out)
    us_hull = timed(lambda: tape_call(hull, out, None, 0), args.iters)
    us_hull_tight = timed(lambda: tape_call(hull, out, None, tight), args.iters)
    us_section = timed(lambda: tape_call(section, out_s, None, 0), args.iters)
    us_girth = timed(girth_call, args.iters)
    us_module = timed(lambda: m(verts, joints), max(1, args.iters // 4))
    us_module_tight = timed(lambda: m_tight(verts, joints), max(1, args.iters // 4))
    res = {'what': 'straps_measure_tape on T-pose bodies of the synthetic SMPL model with measure.tape_measurements() (seven planes); device events over '
                   'back-to-back calls; beside it the same planes as SECTION and as GIRTH of straps_measure_mesh, same process, same inputs.  The '
                   "synthetic model's triangle soup cuts far more faces per plane than a body surface would: an upper bound for a real SMPL mesh",
           'device': torch.cuda.get_device_name(0), 'batch': B, 'nverts': N, 'nfaces': F, 'n_meas': M, 'n_points': n_points, 'iters': args.iters,
           'us_per_call_hull_worst_case_capacity': round(us_hull, 2), 'us_per_call_hull_tight_capacity': round(us_hull_tight, 2),
           'us_per_call_section_collect_kernel_alone': round(us_section, 2), 'us_hull_kernel_estimated_as_difference': round(us_hull - us_section, 2),
           'us_per_call_measure_mesh_girth_same_planes': round(us_girth, 2), 'ratio_hull_to_measure_mesh_girth': round(us_hull / us_girth, 2),
           'us_per_call_module_worst_case_capacity': round(us_module, 2), 'us_per_call_module_tight_capacity': round(us_module_tight, 2),
           'bodies_per_s_hull': round(B / us_hull * 1e6, 1), 'workspace_bytes_worst_case': int(ws_bytes),
           'workspace_bytes_tight': int(L.straps_measure_tape_workspace_bytes(B, F, M, tight)), 'tight_capacity': tight, 'largest_count': largest,
           'largest_count_per_measurement': [int(x) for x in counts.max(0).values.tolist()], 'worst_case_count': 2 * F,
           'max_rel_difference_section_vs_girth': rel, 'names': list(m.names), 'hull_body0': [round(float(x), 6) for x in out[0].tolist()],
           'section_body0': [round(float(x), 6) for x in out_s[0].tolist()]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
