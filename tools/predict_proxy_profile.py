"""Timing of the predict front end on the GPU (profiles/predict_proxy_b64.json was filled from its output).

    python tools/predict_proxy_profile.py kernel [--iters N]     # straps_predict_proxy_input alone: B = 64, 512 x 512 -> 256, 17 joints
    python tools/predict_proxy_profile.py e2e [--steps N]        # Predictor end to end (graph replay), resnet18, B = 64
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/predict_proxy_profile.py kernel --iters 200      # per-kernel times

`kernel` times N back-to-back calls between two device events after a warm-up (the call is two launches: the bounding-box kernel and
the writer) and prints the microseconds per call and the write bandwidth B x 18 x 256^2 x 4 bytes / time.  `e2e` replays a captured
Predictor call and prints bodies/s; bench.py --config 1 is the forward-only figure to hold it against (same regressor and SMPL, its
proxy already on the device).  Each prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import straps_amd                      # noqa: E402
from straps_amd import hipabi          # noqa: E402


def detections(B, hw, nj, seed=0):
    """stand-ins for detector output: a filled ellipse per frame (a 0/1 mask) and joints inside and around it, with a confidence column"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:hw, 0:hw]
    sil = np.zeros((B, hw, hw), np.uint8)
    joints = np.zeros((B, nj, 3), np.float32)
    for b in range(B):
        cy, cx = rng.uniform(0.35, 0.65, 2) * hw
        ry, rx = rng.uniform(0.25, 0.42) * hw, rng.uniform(0.08, 0.2) * hw
        sil[b] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0
        joints[b, :, 0] = cx + rng.uniform(-1.1, 1.1, nj) * rx
        joints[b, :, 1] = cy + rng.uniform(-1.1, 1.1, nj) * ry
        joints[b, :, 2] = rng.uniform(0.5, 1.0, nj)
    return sil, joints


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kernel', 'e2e'])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda:0')
    hipabi.load()
    B, hw, out_wh, nj = args.batch, 512, 256, 17
    s, j = detections(B, hw, nj)
    sil, joints = torch.from_numpy(s).to(dev), torch.from_numpy(j).to(dev)
    if args.what == 'kernel':
        patch = torch.from_numpy(straps_amd.heatmap_patch(4)).to(dev)
        out = torch.empty(B, 1 + nj, out_wh, out_wh, device=dev)
        jout = torch.empty(B, nj, 2, device=dev)
        boxes = torch.empty(B, 6, device=dev, dtype=torch.int32)
        L, st = hipabi.lib(), hipabi.stream_ptr()
        a = (hipabi.ptr(sil), hipabi.ptr(joints), 3, hipabi.ptr(patch), 4, 1.2, hipabi.ptr(out), hipabi.ptr(jout), hipabi.ptr(boxes), B, hw, hw, nj, out_wh, st)
        for _ in range(args.warmup):
            hipabi.check(L.straps_predict_proxy_input(*a), 'straps_predict_proxy_input')
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            L.straps_predict_proxy_input(*a)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.iters
        wbytes = B * (1 + nj) * out_wh * out_wh * 4
        assert int(boxes[:, 4].sum()) == B and bool(torch.isfinite(out).all())
        print(json.dumps({'what': 'straps_predict_proxy_input, both launches, device events over back-to-back calls', 'batch': B, 'in': [hw, hw],
                          'out_wh': out_wh, 'nj': nj, 'iters': args.iters, 'us_per_call': round(us, 2), 'write_bytes_per_call': wbytes,
                          'read_bytes_per_call': B * hw * hw, 'write_GBps_over_call_time': round(wbytes / us / 1e3, 1)}))
        return
    torch.manual_seed(1234)
    mp = straps_amd.synthetic_mean_params(0)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=mp).to(dev).eval()
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=B).to(dev)
    p = straps_amd.Predictor(reg, smpl)
    for _ in range(3):
        p(sil, joints)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = p(sil, joints)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        graph.replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool(res['valid'].all()) and bool(torch.isfinite(res['vertices']).all())
    print(json.dumps({'what': 'Predictor end to end (proxy input + resnet18 regressor + SMPL + projection + reposed SMPL), graph replay, host clock over '
                              'synchronised replays', 'batch': B, 'steps': args.steps, 'ms_per_step': round(dt / args.steps * 1e3, 4),
                      'bodies_per_s': round(B * args.steps / dt, 1), 'proxy_nonzero_fraction': round(float((res['proxy_rep'] != 0).float().mean()), 5)}))


if __name__ == '__main__':
    main()
