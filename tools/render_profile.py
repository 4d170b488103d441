"""Timing of the shaded mesh renderer on the GPU (profiles/render_mesh_b64.json was filled from its output).

    python tools/render_profile.py [--batch 64] [--wh 256] [--iters 2000]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/render_profile.py --iters 200      # per-kernel times

A Predictor (resnet18 regressor, synthetic SMPL model) runs once on stand-in detections; its vertices and cameras are then drawn `iters`
times back to back between two device events after a warm-up: straps_render_mesh alone on preallocated outputs (five launches: fill,
vertices, normals, faces, resolve) over a background picture, and the module call WeakPerspectiveMeshRenderer.forward, which allocates its
outputs and workspace.  Predictor.render is two such calls.  The shader clock is the one the regressor's convolution kernels ran at in the
same process (straps_set_clock_accumulator covers those kernels only).  Prints one JSON line.  There is no parent to compare against."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import straps_amd                      # noqa: E402
from straps_amd import hipabi          # noqa: E402
from predict_proxy_profile import detections      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--wh', type=int, default=256)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda:0')
    L = hipabi.load()
    B, wh = args.batch, args.wh
    s, j = detections(B, 512, 17)
    torch.manual_seed(1234)
    model = straps_amd.synthetic_smpl_model(0)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=straps_amd.synthetic_mean_params(0)).to(dev).eval()
    smpl = straps_amd.SMPL(model, batch_size=B).to(dev)
    pred = straps_amd.Predictor(reg, smpl)
    clk = torch.zeros(2, dtype=torch.int64, device=dev)
    hipabi.check(L.straps_set_clock_accumulator(hipabi.ptr(clk)), 'straps_set_clock_accumulator')
    for _ in range(3):
        out = pred(torch.from_numpy(s).to(dev), torch.from_numpy(j).to(dev))
    torch.cuda.synchronize()
    hipabi.check(L.straps_set_clock_accumulator(None), 'straps_set_clock_accumulator')
    c, w = (int(v) for v in clk.tolist())
    mhz = round(c / w * L.straps_wall_clock_khz() / 1e3, 1) if w > 0 else None
    rend = straps_amd.WeakPerspectiveMeshRenderer(model['faces'], img_wh=wh).to(dev)
    verts, cam = out['vertices'].contiguous(), out['cam_wp'].contiguous()
    N, F = verts.shape[1], rend.faces.shape[0]
    images = torch.randint(0, 256, (B, wh, wh, 3), dtype=torch.uint8, device=dev)
    rgb = torch.empty(B, wh, wh, 3, dtype=torch.uint8, device=dev)
    mask = torch.empty(B, wh, wh, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.straps_render_mesh_workspace_bytes(B, N, wh) // 8, dtype=torch.float64, device=dev)
    opts = rend.render_opts()
    a = (hipabi.ptr(verts), hipabi.ptr(rend.faces), hipabi.ptr(rend.vf_offsets), hipabi.ptr(rend.vf_faces), hipabi.ptr(cam), 3, None, 0, ctypes.byref(opts),
         hipabi.ptr(images), hipabi.ptr(rgb), hipabi.ptr(mask), None, None, hipabi.ptr(ws), B, N, F, wh, hipabi.stream_ptr())

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

    hipabi.check(L.straps_render_mesh(*a), 'straps_render_mesh')
    us_raw = timed(lambda: L.straps_render_mesh(*a), args.iters)
    us_module = timed(lambda: rend(verts, cam, background=images), max(1, args.iters // 4))
    covered = float(mask.float().mean())
    assert 0.0 < covered < 1.0 and torch.equal(rgb, rend(verts, cam, background=images))
    print(json.dumps({'what': 'straps_render_mesh on Predictor output (resnet18 regressor, synthetic SMPL model), device events over back-to-back calls',
                      'batch': B, 'wh': wh, 'nverts': N, 'nfaces': F, 'iters': args.iters, 'us_per_call_library': round(us_raw, 2),
                      'us_per_call_module': round(us_module, 2), 'bodies_per_s_library': round(B / us_raw * 1e6, 1), 'covered_fraction': round(covered, 4),
                      'workspace_bytes': int(ws.numel() * 8), 'sclk_mhz_of_the_regressor_convolutions': mhz}))


if __name__ == '__main__':
    main()
