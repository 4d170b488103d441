"""Timing of the body measurements on the GPU (profiles/measure_b64.json was filled from its output).

    python tools/measure_profile.py [--batch 64] [--iters 2000] [--out profiles/measure_b64.json]

T-pose bodies of the synthetic SMPL model (template + shape directions at random betas, 6890 vertices, 13 776 faces) and their 24 joints are
measured with measure.default_measurements() `iters` times back to back between two device events after a warm-up: straps_measure_mesh
alone on a preallocated output and workspace (two launches), and the module call BodyMeasurer.forward, which allocates them.  Beside it, on
the same GPU and the same inputs, a float64 torch restatement of the same definitions (gathers of [B,F,3,3] corners per call, one masked
reduction per measurement): what a user would write without the kernel.  The two are compared before anything is timed.  Prints one JSON
line and, with --out, writes it there.  There is no parent to compare against."""
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

HBM_BYTES_PER_S = 6.29e12              # measured float4 copy rate of the MI355X (8.0e12 is the specification)


def torch_restatement(verts, joints, faces, face_parts, specs):
    """float64 torch on the device: the definitions of include/straps_hip.h, measurement by measurement -> [B,M] float32"""
    V, J = verts.double(), joints.double()
    P = V[:, faces.long()]                                      # [B,F,3,3]
    point = lambda a: J[:, a[1]] if isinstance(a, tuple) else V[:, a]
    cols = []
    for s in specs:
        sel = None
        if s.parts:
            sel = torch.zeros_like(face_parts, dtype=torch.bool)
            for p in s.parts:
                sel |= face_parts == p
        pick = lambda t: t if sel is None else t * sel
        if s.kind == hipabi.MEASURE_VOLUME:
            r = P - (point(s.anchors[0])[:, None, None] if s.anchors else 0.0)
            cols.append(pick((r[:, :, 0] * torch.cross(r[:, :, 1], r[:, :, 2], dim=-1)).sum(-1)).sum(1) / 6.0)
        elif s.kind == hipabi.MEASURE_AREA:
            cols.append(0.5 * pick(torch.cross(P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0], dim=-1).norm(dim=-1)).sum(1))
        elif s.kind == hipabi.MEASURE_EXTENT:
            h = V @ torch.tensor(s.direction, dtype=torch.float32, device=V.device).double()            # (the library takes the direction as fp32)
            cols.append(h.max(1).values - h.min(1).values)
        elif s.kind == hipabi.MEASURE_GIRTH:
            n = torch.tensor(s.direction, dtype=torch.float32, device=V.device).double()
            d = (P - point(s.anchors[0])[:, None, None]) @ n               # [B,F,3]
            pos = d >= 0
            cut = ~((pos[..., 0] == pos[..., 1]) & (pos[..., 1] == pos[..., 2]))
            lone = torch.where(pos[..., 1] == pos[..., 2], 0, torch.where(pos[..., 0] == pos[..., 2], 1, 2))
            idx = torch.stack([lone, (lone + 1) % 3, (lone + 2) % 3], -1)      # [B,F,3]: the lone vertex, then the other two
            Q = torch.gather(P, 2, idx[..., None].expand(-1, -1, -1, 3))
            dd = torch.gather(d, 2, idx)
            safe = lambda x: torch.where(cut, x, torch.ones_like(x))
            tb, tc = dd[..., 0] / safe(dd[..., 0] - dd[..., 1]), dd[..., 0] / safe(dd[..., 0] - dd[..., 2])
            xb = Q[:, :, 0] + tb[..., None] * (Q[:, :, 1] - Q[:, :, 0])
            xc = Q[:, :, 0] + tc[..., None] * (Q[:, :, 2] - Q[:, :, 0])
            cols.append(pick((xb - xc).norm(dim=-1) * cut).sum(1))
        else:
            pts = [point(a) for a in s.anchors]
            cols.append(sum((pts[i + 1] - pts[i]).norm(dim=-1) for i in range(len(pts) - 1)))
    return torch.stack(cols, 1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=50)
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
    m = straps_amd.BodyMeasurer(model['faces'], model['face_parts']).to(dev)
    N, F, M = verts.shape[1], m.faces.shape[0], len(m.specs)
    arr, n_points = measure.measure_structs(m.specs, N)
    points = joints[:, :n_points].contiguous()
    out = torch.empty(B, M, dtype=torch.float32, device=dev)
    ws_bytes = L.straps_measure_workspace_bytes(B, N, F, M)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    a = (hipabi.ptr(verts), hipabi.ptr(points), hipabi.ptr(m.faces), hipabi.ptr(m.face_parts), arr, hipabi.ptr(out), hipabi.ptr(ws), B, N, n_points, F, M,
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

    hipabi.check(L.straps_measure_mesh(*a), 'straps_measure_mesh')
    ref = torch_restatement(verts, joints, m.faces, m.face_parts, m.specs)
    torch.cuda.synchronize()
    rel = float(((out - ref).abs() / ref.abs().clamp_min(1e-6)).max())
    assert torch.equal(out, m(verts, joints)['values']) and rel < 1e-5, rel
    us_raw = timed(lambda: L.straps_measure_mesh(*a), args.iters)
    us_module = timed(lambda: m(verts, joints), max(1, args.iters // 4))
    us_torch = timed(lambda: torch_restatement(verts, joints, m.faces, m.face_parts, m.specs), max(1, args.iters // 40))
    vert_bytes = B * N * 12
    res = {'what': 'straps_measure_mesh on T-pose bodies of the synthetic SMPL model with measure.default_measurements(); device events over back-to-back '
                   'calls; beside it a float64 torch restatement of the same definitions on the same GPU and inputs',
           'device': torch.cuda.get_device_name(0), 'batch': B, 'nverts': N, 'nfaces': F, 'n_meas': M, 'n_points': n_points, 'iters': args.iters,
           'us_per_call_library': round(us_raw, 2), 'us_per_call_module': round(us_module, 2), 'us_per_call_torch_float64': round(us_torch, 2),
           'bodies_per_s_library': round(B / us_raw * 1e6, 1), 'workspace_bytes': int(ws_bytes), 'vertex_bytes': vert_bytes,
           'us_to_read_the_vertices_at_hbm_rate': round(vert_bytes / HBM_BYTES_PER_S * 1e6, 3), 'hbm_bytes_per_s_assumed': HBM_BYTES_PER_S,
           'fraction_of_the_call_that_reading_the_vertices_at_hbm_rate_would_take': round(vert_bytes / HBM_BYTES_PER_S * 1e6 / us_raw, 4),
           'max_rel_difference_library_vs_torch': rel, 'names': list(m.names), 'values_body0': [round(float(x), 6) for x in out[0].tolist()]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
