"""A/B of the eval-mode regressor forward: SingleInputRegressor.eval() (Python scheduling, ~35 / ~70 library calls per forward) vs
InferenceRegressor (one straps_regressor_fwd_infer call), each eager and captured in torch.cuda.graph -- four variants in one process,
on the same seeded sparse proxy inputs, alternating, after a warm-up, timed with device events over windows of at least --window
seconds.  All four must give bit-equal outputs (asserted before any timing).  Writes profiles/regressor_infer_ab.json.

    python tools/regressor_infer_ab.py [--layers 18 50] [--batches 1 16 64] [--rounds 3] [--window 1.0]

Kernel-trace mode (one variant, a fixed number of calls, no graphs -- for rocprofv3 --kernel-trace --stats):
    python tools/regressor_infer_ab.py --trace module|composite --layers 18 --batches 1 --calls 200
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import straps_amd  # noqa: E402


def sparse_proxy(B, cin, h, w, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, cin, h, w, generator=g)
    return torch.where(torch.rand(B, cin, h, w, generator=g) < 0.02, x, torch.zeros(())).to(dev)


def make_regressor(layers, dev):
    torch.manual_seed(layers)
    reg = straps_amd.SingleInputRegressor(18, layers, 3, mean_params=straps_amd.synthetic_mean_params(0))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for m in reg.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.weight.shape[0]
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return reg.to(dev).eval()


def variants(reg, ir, static_x):
    """name -> callable running one forward on static_x; `out` holds each variant's output tensors (cam, pose, shape)"""
    out = {}

    def module_eager():
        out['module_eager'] = reg(static_x)

    def composite_eager():
        out['composite_eager'] = ir(static_x)
    fns = {'module_eager': module_eager, 'composite_eager': composite_eager}
    for name, fn in (('module_graph', lambda: reg(static_x)), ('composite_graph', lambda: ir(static_x))):
        fn()                                   # warm-up outside the capture (packed weights, workspace)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out[name] = fn()
        fns[name] = g.replay
    return fns, out


def time_window(fn, n):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    st.record()
    for _ in range(n):
        fn()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers', type=int, nargs='+', default=[18, 50])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16, 64])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0, help='seconds per timed window (at least)')
    ap.add_argument('--trace', choices=['module', 'composite'], default=None)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'regressor_infer_ab.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    if a.trace:
        reg = make_regressor(a.layers[0], dev)
        x = sparse_proxy(a.batches[0], 18, 256, 256, 11, dev)
        if a.trace == 'module':
            fn = lambda: reg(x)      # noqa: E731
        else:
            ir = straps_amd.InferenceRegressor(reg)
            fn = lambda: ir(x)       # noqa: E731
        with torch.no_grad():
            for _ in range(a.calls):
                fn()
        torch.cuda.synchronize()
        print('trace: %s r%d B=%d, %d calls' % (a.trace, a.layers[0], a.batches[0], a.calls))
        return
    rows = []
    with torch.no_grad():
        for layers in a.layers:
            reg = make_regressor(layers, dev)
            ir = straps_amd.InferenceRegressor(reg)
            for B in a.batches:
                x = sparse_proxy(B, 18, 256, 256, 100 + B, dev)
                static_x = x.clone()
                fns, out = variants(reg, ir, static_x)
                for f in fns.values():
                    f()
                torch.cuda.synchronize()
                cat = {k: torch.cat(v, 1) for k, v in out.items()}
                ref = cat['module_eager']
                for k, v in cat.items():
                    assert torch.equal(v, ref), 'r%d B=%d: %s differs from module_eager' % (layers, B, k)
                # calls per window from a short calibration of each variant
                n = {}
                for k, f in fns.items():
                    ms = time_window(f, 5)
                    n[k] = max(5, int(a.window * 1e3 / max(ms, 1e-3)) + 1)
                times = {k: [] for k in fns}
                for r in range(a.rounds):
                    order = list(fns) if r % 2 == 0 else list(fns)[::-1]
                    for k in order:
                        times[k].append(time_window(fns[k], n[k]))
                med = {k: statistics.median(v) for k, v in times.items()}
                row = dict(layers=layers, batch=B, ms=med, ms_all=times, calls_per_window=n,
                           composite_vs_module_eager=med['module_eager'] / med['composite_eager'],
                           composite_graph_vs_module_graph=med['module_graph'] / med['composite_graph'],
                           workspace_mb=ir.workspace_bytes(B, 256, 256) / 2 ** 20, prepared_mb=ir.prepared.numel() / 2 ** 20, bit_equal=True)
                rows.append(row)
                print('r%d B=%-3d  module eager %8.3f ms  module graph %8.3f ms  composite eager %8.3f ms  composite graph %8.3f ms'
                      '  (eager x%.2f, graph x%.2f)' % (layers, B, med['module_eager'], med['module_graph'], med['composite_eager'],
                                                        med['composite_graph'], row['composite_vs_module_eager'], row['composite_graph_vs_module_graph']),
                      flush=True)
                del fns, out
                torch.cuda.synchronize()
    res = dict(tool='tools/regressor_infer_ab.py', device=torch.cuda.get_device_name(0), when=time.strftime('%Y-%m-%d %H:%M:%S'),
               input='seeded sparse proxy, 18 x 256 x 256, ~98 % zeros', precision='bf16x3', rounds=a.rounds, window_s=a.window, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
