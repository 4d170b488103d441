"""A/B of the train-mode regressor forward + backward: SingleInputRegressor's autograd path (Python scheduling, ~3x the library calls of
the eval forward) vs CompositeTrainer (one straps_regressor_fwd_train + one straps_regressor_bwd call), each eager and captured in
torch.cuda.graph -- four variants in one process, on the same seeded sparse proxy inputs and upstream gradient, alternating, after a
warm-up, timed with device events over windows of at least --window seconds.  The estimate and every parameter gradient of all four
must be bit-equal (asserted before any timing; the running statistics move with every call but do not enter the train-mode outputs).
Writes profiles/regressor_train_ab.json.

    python tools/regressor_train_ab.py [--configs 18:1 18:16 18:64 50:1 50:32] [--rounds 3] [--window 1.0]
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
    return reg.to(dev).train()


def variants(reg, tr, x, dest):
    """name -> callable running one forward + backward; `out` holds each variant's (estimate, flat gradients)"""
    params = list(reg.parameters())
    out = {}

    def module():
        cam, pose, shape = reg(x)
        gs = torch.autograd.grad([cam, pose, shape], params, [dest[:, :3], dest[:, 3:147], dest[:, 147:157]])
        return torch.cat([cam, pose, shape], 1), gs

    def composite():
        cam, pose, shape = tr.forward(x)
        g, _ = tr.backward(dest)
        return torch.cat([cam, pose, shape], 1), (g,)

    def eager(name, fn):
        def run():
            out[name] = fn()
        return run
    fns = {'module_eager': eager('module_eager', module), 'composite_eager': eager('composite_eager', composite)}
    for name, fn in (('module_graph', module), ('composite_graph', composite)):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):             # warm-up outside the capture (packed weights, workspace, autograd state)
            fn()
        torch.cuda.current_stream().wait_stream(s)
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
    ap.add_argument('--configs', nargs='+', default=['18:1', '18:16', '18:64', '50:1', '50:32'], help='layers:batch')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=1.0, help='seconds per timed window (at least)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'regressor_train_ab.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rows = []
    for cfg in a.configs:
        layers, B = (int(v) for v in cfg.split(':'))
        reg = make_regressor(layers, dev)
        tr = straps_amd.CompositeTrainer(reg)
        x = sparse_proxy(B, 18, 256, 256, 100 + B, dev)
        g = torch.Generator().manual_seed(200 + B)
        dest = torch.zeros(B, 160)
        dest[:, :157] = torch.randn(B, 157, generator=g) * 0.1
        dest = dest.to(dev)
        fns, out = variants(reg, tr, x, dest)
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        flat = {k: (v[0], torch.cat([t.reshape(-1) for t in v[1]])) for k, v in out.items()}
        ref = flat['module_eager']
        for k, (est, grads) in flat.items():
            assert torch.equal(est, ref[0]) and torch.equal(grads, ref[1]), 'r%d B=%d: %s differs from module_eager' % (layers, B, k)
        n = {}
        for k, f in fns.items():
            ms = time_window(f, 3)
            n[k] = max(3, int(a.window * 1e3 / max(ms, 1e-3)) + 1)
        times = {k: [] for k in fns}
        for r in range(a.rounds):
            order = list(fns) if r % 2 == 0 else list(fns)[::-1]
            for k in order:
                times[k].append(time_window(fns[k], n[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        row = dict(layers=layers, batch=B, ms=med, ms_all=times, calls_per_window=n,
                   composite_vs_module_eager=med['module_eager'] / med['composite_eager'],
                   composite_graph_vs_module_graph=med['module_graph'] / med['composite_graph'],
                   workspace_mb=tr.workspace_bytes(B, 256, 256) / 2 ** 20, bit_equal=True)
        rows.append(row)
        print('r%d B=%-3d  module eager %8.3f ms  module graph %8.3f ms  composite eager %8.3f ms  composite graph %8.3f ms'
              '  (eager x%.2f, graph x%.2f)' % (layers, B, med['module_eager'], med['module_graph'], med['composite_eager'],
                                                med['composite_graph'], row['composite_vs_module_eager'], row['composite_graph_vs_module_graph']),
              flush=True)
        del fns, out, tr, reg
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    res = dict(tool='tools/regressor_train_ab.py', device=torch.cuda.get_device_name(0), when=time.strftime('%Y-%m-%d %H:%M:%S'),
               input='seeded sparse proxy, 18 x 256 x 256, ~98 % zeros; ms per forward + backward (all parameter gradients)',
               precision='bf16x3', rounds=a.rounds, window_s=a.window, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
