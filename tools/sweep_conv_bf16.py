"""Tile sweep of the single-product bf16 convolution (straps_conv_fwd_bf16, csrc/conv_bf16.hip) over every resnet18 / resnet50 eval
convolution shape (256 x 256 input) at B = 1, 64, 256: each admissible tile configuration (tile_cfg 1..10) timed on the launch the eval
forward makes (folded BatchNorm, ReLU, fp32 output + one bf16 output plane; projections: fp32 output only), next to the bf16x3 launch of
the same shape (straps_conv_fwd_x3p / straps_conv_fwd_x3) and the automatic rule's pick.  Device events, median of --reps launches after
a warm-up, the shader clock read through straps_set_clock_accumulator.  Writes profiles/sweep_conv_bf16.json (or --out).

    python tools/sweep_conv_bf16.py [--batches 1 64 256] [--reps 20] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import straps_amd  # noqa: E402
from straps_amd import hipabi  # noqa: E402

NCFG = 10


def eval_conv_shapes(layers, h=256, w=256):
    """unique (H, W, cin, cout, k, stride, pad, relu) of the eval forward's 3x3 / 1x1 convolutions (relu = 0: a projection)"""
    net = straps_amd.resnet18(18) if layers == 18 else straps_amd.resnet50(18)
    out = []

    def o(x, k, s, p):
        return (x + 2 * p - k) // s + 1
    H, W = o(o(h, 7, 2, 3), 3, 2, 1), o(o(w, 7, 2, 3), 3, 2, 1)
    for li in range(1, 5):
        for u in getattr(net, 'layer%d' % li):
            if u.downsample is not None:
                c = u.downsample[0]
                out.append((H, W, c.in_channels, c.out_channels, 1, c.stride[0], 0, 0))
            th, tw = H, W
            for conv, _ in u.conv_bn_pairs():
                k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
                out.append((th, tw, conv.in_channels, conv.out_channels, k, s, p, 1))
                th, tw = o(th, k, s, p), o(tw, k, s, p)
            H, W = th, tw
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def median_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sweep_conv_bf16.json'))
    a = ap.parse_args()
    L = hipabi.lib()
    dev = torch.device('cuda:0')
    clk = torch.zeros(2, dtype=torch.int64, device=dev)
    shapes = {}
    for layers in (18, 50):
        for s in eval_conv_shapes(layers):
            shapes.setdefault(s, []).append('r%d' % layers)
    rows = []
    S = hipabi.stream_ptr
    P = hipabi.ptr
    for B in a.batches:
        for (H, W, cin, cout, k, s, p, relu), nets in shapes.items():
            Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
            n_in, n_out = B * H * W * cin, B * Ho * Wo * cout
            x = torch.rand(n_in, device=dev) - 0.5
            wt = torch.randn(cout, cin, k, k, device=dev) * (2.0 / (cin * k * k)) ** 0.5
            ss = torch.stack([torch.rand(cout, device=dev) + 0.5, torch.rand(cout, device=dev) - 0.5])
            x1 = torch.empty((n_in + 7) // 8 * 8, dtype=torch.int16, device=dev)
            w1 = torch.empty(wt.numel(), dtype=torch.int16, device=dev)
            hipabi.check(L.straps_split_bf16_cm(P(x), P(x1), B * H * W, cin, S()), 'split')
            hipabi.check(L.straps_pack_conv_weight_bf16(P(wt), P(w1), cout, cin, k, k, S()), 'pack')
            from straps_amd.encoder_exec import split3, weight_planes
            x3, xps = split3(L, x.view(-1, cin))
            w3, wps = weight_planes(L, wt)
            y = torch.empty(n_out, device=dev)
            y1 = torch.empty((n_out + 7) // 8 * 8, dtype=torch.int16, device=dev)
            y3 = torch.empty(3, (n_out + 7) // 8 * 8, dtype=torch.int16, device=dev)
            yps = y3.shape[1]

            def bf16(cfg):
                return lambda: hipabi.check(L.straps_conv_fwd_bf16(P(x1), P(w1), P(ss[0]), P(ss[1]), None, relu, P(y), P(y1) if relu else None,
                                                                   B, H, W, cin, cout, k, k, s, p, cfg, S()), 'bf16 cfg %d' % cfg)

            def x3p():
                if relu:
                    hipabi.check(L.straps_conv_fwd_x3p(P(x3), xps, P(w3), wps, P(ss[0]), P(ss[1]), None, 1, P(y), P(y3), yps, B, H, W, cin, cout,
                                                       k, k, s, p, 0, S()), 'x3p')
                else:
                    hipabi.check(L.straps_conv_fwd_x3(P(x3), xps, P(w3), wps, P(ss[0]), P(ss[1]), None, 0, P(y), None, B, H, W, cin, cout,
                                                      k, k, s, p, 0, S()), 'x3')
            rule = L.straps_conv_bf16_tile_choice(B, H, W, cin, cout, k, k, s, p)
            row = dict(nets=nets, B=B, H=H, W=W, cin=cin, cout=cout, k=k, stride=s, relu=relu, M=B * Ho * Wo, rule=rule, cfg_us={})
            clk.zero_()
            L.straps_set_clock_accumulator(P(clk))
            try:
                row['x3_us'] = median_us(x3p, a.reps)
                for cfg in range(1, NCFG + 1):
                    if L.straps_conv_fwd_bf16(P(x1), P(w1), P(ss[0]), P(ss[1]), None, relu, P(y), P(y1) if relu else None,
                                              B, H, W, cin, cout, k, k, s, p, cfg, S()) != 0:
                        continue          # (not admitted for this geometry: refused before any launch)
                    row['cfg_us'][cfg] = median_us(bf16(cfg), a.reps)
            finally:
                torch.cuda.synchronize()
                L.straps_set_clock_accumulator(None)
            c = clk.cpu().tolist()
            row['sclk_mhz'] = round(c[0] / c[1] * L.straps_wall_clock_khz() / 1000.0, 1) if c[1] else None
            best = min(row['cfg_us'], key=row['cfg_us'].get)
            row['best'] = best
            row['rule_us'] = row['cfg_us'].get(rule)
            row['speedup_rule_vs_x3'] = round(row['x3_us'] / row['rule_us'], 3) if row['rule_us'] else None
            rows.append(row)
            print('B=%3d %-7s %3dx%-3d %4d->%-4d k%d s%d  x3 %8.1f us  rule %2d %8.1f us  best %2d %8.1f us  (%.0f MHz)' % (
                B, '/'.join(nets), H, W, cin, cout, k, s, row['x3_us'], rule, row['rule_us'] or -1, best, row['cfg_us'][best],
                row['sclk_mhz'] or 0), flush=True)
            del x, x1, x3, w3, y, y1, y3
    tot = {}
    for r in rows:
        t = tot.setdefault(r['B'], dict(x3=0.0, rule=0.0, best=0.0))
        t['x3'] += r['x3_us']
        t['rule'] += r['rule_us']
        t['best'] += r['cfg_us'][r['best']]
    res = dict(tool='tools/sweep_conv_bf16.py', device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows,
               totals_us_per_batch={str(k): v for k, v in tot.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res['totals_us_per_batch']))


if __name__ == '__main__':
    main()
