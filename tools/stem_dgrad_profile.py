"""Workloads for timing the stem data gradient (straps_stem_dgrad) and for tracing a frozen-regressor input-gradient backward.

    python tools/stem_dgrad_profile.py kernels [--batch 64] [--calls 20]
        the dense stem forward (training-mode launch, every input cell marked non-zero: bench.py --dense-stem's kernel) and the stem data
        gradient on the same shapes (cin = 18, 256 x 256), alternating, after a warm-up; prints device-event times per call and the share
        of the fp32 matrix peak.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel times.
    python tools/stem_dgrad_profile.py frozen [--batch 8] [--layers 18]
        one backward of loss(reg(x)) with every parameter frozen and x.requires_grad: the trace lists the data-gradient and BatchNorm
        kernels, and no weight-gradient kernel.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import straps_amd  # noqa: E402
from straps_amd import hipabi  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12       # MI355X, v_mfma_f32_32x32x2_f32 / 16x16x4_f32


def kernels(args):
    dev = torch.device('cuda:0')
    L = hipabi.lib()
    B, C, H, W = args.batch, 18, 256, 256
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, C, H, W, generator=g).to(dev)
    w = (torch.rand(64, C, 7, 7, generator=g) - 0.5).to(dev)
    dy = (torch.rand(B, Ho, Wo, 64, generator=g) - 0.5).to(dev)
    wf = torch.empty(L.straps_stem_weight_floats(C), device=dev)
    hipabi.check(L.straps_pack_stem_weight(hipabi.ptr(w), hipabi.ptr(wf), C, hipabi.stream_ptr()), 'pack')
    wd = torch.empty(L.straps_stem_dgrad_weight_floats(C), device=dev)
    hipabi.check(L.straps_pack_stem_dgrad_weight(hipabi.ptr(w), hipabi.ptr(wd), C, hipabi.stream_ptr()), 'pack dgrad')
    nz = torch.full((L.straps_stem_nzmask_words(B, C, H, W),), -1, device=dev, dtype=torch.int32)
    y = torch.empty(B, Ho, Wo, 64, device=dev)
    part = torch.empty(L.straps_stem_stat_blocks(B, H, W), 64, 2, device=dev)
    dx = torch.empty(B, C, H, W, device=dev)

    def fwd():
        hipabi.check(L.straps_stem_fwd(hipabi.ptr(x), hipabi.ptr(wf), None, None, 0, hipabi.ptr(y), hipabi.ptr(part), hipabi.ptr(nz), B, C, H, W,
                                       hipabi.stream_ptr()), 'straps_stem_fwd')

    def dgrad():
        hipabi.check(L.straps_stem_dgrad(hipabi.ptr(dy), hipabi.ptr(wd), hipabi.ptr(dx), B, C, H, W, 0, hipabi.stream_ptr()), 'straps_stem_dgrad')

    for _ in range(3):
        fwd()
        dgrad()
    torch.cuda.synchronize()
    t = {'stem_fwd_dense': [], 'stem_dgrad': []}
    for _ in range(args.calls):
        for name, fn in (('stem_fwd_dense', fwd), ('stem_dgrad', dgrad)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    flop = 2.0 * B * Ho * Wo * 64 * C * 49
    for name, v in t.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print('%-15s B=%d cin=%d %dx%d: median %.3f ms (min %.3f, max %.3f) over %d calls; %.1f TFLOP/s = %.2f of the fp32 matrix peak'
              % (name, B, C, H, W, med, v[0], v[-1], len(v), flop / med * 1e-9, flop / med * 1e-9 / (FP32_MATRIX_PEAK * 1e-12)))


def frozen(args):
    dev = torch.device('cuda:0')
    reg = straps_amd.SingleInputRegressor(18, args.layers, 3, mean_params=straps_amd.synthetic_mean_params(0)).to(dev).eval()
    for p in reg.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(args.batch, 18, 256, 256, generator=g)
    x = torch.where(torch.rand(x.shape, generator=g) < 0.05, x, torch.zeros(())).to(dev).requires_grad_(True)
    out = torch.cat(reg(x), 1)
    torch.cuda.synchronize()
    out.sum().backward()
    torch.cuda.synchronize()
    print('frozen r%d B=%d: |x.grad| max %.3e, parameter grads all None: %s'
          % (args.layers, args.batch, float(x.grad.abs().max()), all(p.grad is None for p in reg.parameters())))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernels', 'frozen'])
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--layers', type=int, default=18)
    a = ap.parse_args()
    if a.batch is None:
        a.batch = 64 if a.mode == 'kernels' else 8
    hipabi.load()
    kernels(a) if a.mode == 'kernels' else frozen(a)
