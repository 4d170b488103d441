"""A/B of the eval-mode regressor forward, single-product bf16 convolutions ('bf16') against the default bf16x3 route: the module captured in
torch.cuda.graph and the one-call composite (InferenceRegressor, eager), for resnet18 / resnet50 at B = 1, 64, 256 -- the two precisions
interleaved on the same box in alternating order over --rounds windows of at least --window seconds, timed with device events, with the
shader clock of the convolution launches (straps_set_clock_accumulator) reported next to the times.  Module and composite must be bit-equal
per precision (asserted before any timing).  Also the accuracy cost: the bf16 estimates against the fp32 route's (conv_precision 'fp32') and
the bf16x3 route's, on the 157 estimates and on the SMPL vertices (mm), for random-init r18 / r50 on the sparse proxy and for the
reference-generated deterministic weights on the golden input.  Writes profiles/regressor_bf16_ab.json.

    python tools/regressor_bf16_ab.py [--layers 18 50] [--batches 1 64 256] [--rounds 3] [--window 1.0]

Kernel-trace mode (one variant, a fixed number of calls, no graphs -- for rocprofv3 --kernel-trace --stats):
    python tools/regressor_bf16_ab.py --trace bf16|bf16x3 --layers 18 --batches 64 --calls 50
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import torch  # noqa: E402

import straps_amd  # noqa: E402
from straps_amd import hipabi  # noqa: E402
from regressor_infer_ab import make_regressor, sparse_proxy, time_window  # noqa: E402

PRECS = ('bf16', 'bf16x3')


def accuracy(dev):
    """max / mean |difference| of the bf16 estimates and their SMPL vertices (mm) from the fp32 route's and the bf16x3 route's"""
    from detgen import det_state_dict, det_uniform
    mp = straps_amd.synthetic_mean_params(0)
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=2).to(dev)
    rows = []
    for layers in (18, 50):
        for weights in ('random', 'golden'):
            if weights == 'golden':
                man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_dict_keys_r%d.json' % layers)))['keys']
                reg = straps_amd.SingleInputRegressor(18, layers, 3, mean_params=mp)
                reg.load_state_dict({k: torch.from_numpy(v) for k, v in det_state_dict(man).items()}, strict=True)
                reg = reg.to(dev).eval()
                x = torch.from_numpy(det_uniform((2, 18, 256, 256), 4242, 0.0, 1.0)).to(dev)
            else:
                reg = make_regressor(layers, dev)
                x = sparse_proxy(2, 18, 256, 256, 5, dev)
            out = {}
            for prec in ('fp32', 'bf16x3', 'bf16'):
                reg.image_encoder.conv_precision = prec
                with torch.no_grad():
                    cam, pose, shape = reg(x)
                    R = straps_amd.rot6d_to_rotmat(pose).view(-1, 24, 3, 3)
                    v = smpl(body_pose=R[:, 1:], global_orient=R[:, 0:1], betas=shape.contiguous(), pose2rot=False).vertices
                out[prec] = (torch.cat([cam, pose, shape], 1).double().cpu(), v.double().cpu() * 1000.0)
            row = dict(layers=layers, weights=weights, batch=2)
            for ref in ('fp32', 'bf16x3'):
                de = (out['bf16'][0] - out[ref][0]).abs()
                dv = (out['bf16'][1] - out[ref][1]).abs()
                row['vs_' + ref] = dict(est_max=float(de.max()), est_mean=float(de.mean()), verts_mm_max=float(dv.max()), verts_mm_mean=float(dv.mean()))
            row['bf16x3_vs_fp32_est_max'] = float((out['bf16x3'][0] - out['fp32'][0]).abs().max())
            rows.append(row)
            print('accuracy r%d %-6s bf16 vs fp32: est max %.3e mean %.3e, verts max %.3f mean %.4f mm  (bf16x3 vs fp32 est max %.1e)' % (
                layers, weights, row['vs_fp32']['est_max'], row['vs_fp32']['est_mean'], row['vs_fp32']['verts_mm_max'], row['vs_fp32']['verts_mm_mean'],
                row['bf16x3_vs_fp32_est_max']), flush=True)
            del reg
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers', type=int, nargs='+', default=[18, 50])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0, help='seconds per timed window (at least)')
    ap.add_argument('--trace', choices=PRECS, default=None)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'regressor_bf16_ab.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    L = hipabi.lib()
    if a.trace:
        reg = make_regressor(a.layers[0], dev)
        reg.image_encoder.conv_precision = a.trace
        x = sparse_proxy(a.batches[0], 18, 256, 256, 11, dev)
        with torch.no_grad():
            for _ in range(a.calls):
                reg(x)
        torch.cuda.synchronize()
        print('trace: %s r%d B=%d, %d calls' % (a.trace, a.layers[0], a.batches[0], a.calls))
        return
    clk = torch.zeros(2, dtype=torch.int64, device=dev)
    rows = []
    with torch.no_grad():
        for layers in a.layers:
            reg = make_regressor(layers, dev)
            for B in a.batches:
                x = sparse_proxy(B, 18, 256, 256, 100 + B, dev)
                static_x = x.clone()
                fns, outs = {}, {}
                for prec in PRECS:
                    reg.image_encoder.conv_precision = prec
                    ir = straps_amd.InferenceRegressor(reg)
                    ref = torch.cat(reg(static_x), 1)
                    got = torch.cat(ir(static_x), 1)
                    assert torch.equal(ref, got), 'r%d B=%d %s: composite != module' % (layers, B, prec)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        outs[prec] = reg(static_x)
                    g.replay()
                    torch.cuda.synchronize()
                    assert torch.equal(torch.cat(outs[prec], 1), ref), 'r%d B=%d %s: graph replay != eager' % (layers, B, prec)
                    fns['module_graph_' + prec] = g.replay
                    fns['composite_' + prec] = (lambda ir_=ir: ir_(static_x))
                n = {}
                for k, f in fns.items():
                    ms = time_window(f, 3)
                    n[k] = max(3, int(a.window * 1e3 / max(ms, 1e-3)) + 1)
                times = {k: [] for k in fns}
                mhz = {k: [] for k in fns}
                for r in range(a.rounds):
                    order = list(fns) if r % 2 == 0 else list(fns)[::-1]
                    for k in order:
                        clk.zero_()
                        L.straps_set_clock_accumulator(hipabi.ptr(clk))
                        try:
                            times[k].append(time_window(fns[k], n[k]))
                        finally:
                            torch.cuda.synchronize()
                            L.straps_set_clock_accumulator(None)
                        c = clk.cpu().tolist()
                        mhz[k].append(round(c[0] / c[1] * L.straps_wall_clock_khz() / 1000.0, 1) if c[1] else None)
                med = {k: statistics.median(v) for k, v in times.items()}
                row = dict(layers=layers, batch=B, ms=med, ms_all=times, sclk_mhz=mhz, calls_per_window=n,
                           speedup_module_graph=med['module_graph_bf16x3'] / med['module_graph_bf16'],
                           speedup_composite=med['composite_bf16x3'] / med['composite_bf16'])
                rows.append(row)
                print('r%d B=%-3d  module graph bf16x3 %8.3f  bf16 %8.3f ms (x%.2f)   composite bf16x3 %8.3f  bf16 %8.3f ms (x%.2f)   clock %s' % (
                    layers, B, med['module_graph_bf16x3'], med['module_graph_bf16'], row['speedup_module_graph'], med['composite_bf16x3'],
                    med['composite_bf16'], row['speedup_composite'], {k: v[-1] for k, v in mhz.items()}), flush=True)
                del fns, outs, g
                torch.cuda.synchronize()
    acc = accuracy(dev)
    res = dict(tool='tools/regressor_bf16_ab.py', device=torch.cuda.get_device_name(0), when=time.strftime('%Y-%m-%d %H:%M:%S'),
               input='seeded sparse proxy, 18 x 256 x 256, ~98 % zeros', rounds=a.rounds, window_s=a.window,
               note='clock: shader clock of the convolution / SMPL launches over each timed window (straps_set_clock_accumulator)', rows=rows, accuracy=acc)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
