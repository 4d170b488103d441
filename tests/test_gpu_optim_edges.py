"""GPU: the kernels that close a training step at their edges, behind redzones (tests/redzone.py) -- straps_adam_step, straps_mse_fwd,
straps_mse_bwd (csrc/train.hip); cases, launch rules and float64 references are tests/head_cases.py, held together by
tests/test_head_cases_cpu.py (the Adam reference against torch.optim.Adam, the MSE reference against F.mse_loss with an index-selected mask).

Common form: outputs and the 512-float workspace from Zone.guarded (exactly the advertised size, sentinel margins; NaN-filled where the kernel
only writes), operands from Zone.at_end (the row mask, one byte per row, ends before a margin of non-zero bytes: a row read past its end counts as
kept), Zone.check() after every call, float64 references on the CPU from the same fp32 data and from the fp32 values of the scalar arguments,
comparisons per element.

Bounds, derived by counting roundings (head_cases.adam_reference, head_cases.mse_reference), never tuned:
  * Adam: m within 4 u (|b1 m| + |(1 - b1) g|), v within 5 u (b2 v + (1 - b2) g^2) (below 2^-126 only v >= 0), p within u |p_new| + 12 u |update|,
    u = 2^-24; an element with g = m = v = 0 leaves p bit-identical.  Worst error / bound seen on an MI355X: m 0.516, v 0.712, p 0.999 (the final
    subtraction's half ulp where p_new lies just above a power of two: half an ulp is u |p_new| there, the whole first term);
  * MSE forward: the count exact, the sum within (ceil(n / 65536) + 20) u sum d^2, the mean within that / count + 2 u |mean|; all rows masked: sum
    and count +0.0, mean NaN (a mean over nothing, as F.mse_loss gives; pinned so that a change is deliberate).  Worst seen: sum 0.034, mean 0.033;
  * MSE backward: masked rows exactly +0.0 over a NaN-filled grad, kept elements within 4 u |c| (|p| + |t ts| + |tb|).  Worst seen: 0.246.
"""
import pytest
import torch

import head_cases as H
import straps_amd  # noqa: F401
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
P = hipabi.ptr
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    lib = hipabi.load()
    import os
    assert os.path.abspath(lib._name) == os.path.abspath(hipabi.LIB_PATH), 'these tests run on the product library, not %s' % lib._name
    return torch.device('cuda:0')


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_adam_step

def _adam_run(dev, p, g, m, v, step, gs, on_device):
    L = hipabi.lib()
    z = Zone(dev)
    n = p.numel()
    pd, md, vd = z.guarded((n,), name='params'), z.guarded((n,), name='exp_avg'), z.guarded((n,), name='exp_avg_sq')
    pd.copy_(p)
    md.copy_(m)
    vd.copy_(v)
    sd = z.at_end(torch.tensor([step], dtype=torch.int64)) if on_device else None
    hipabi.check(L.straps_adam_step(P(pd), P(z.at_end(g)), P(md), P(vd), n, 0 if on_device else step, H.ADAM_LR, H.ADAM_B1, H.ADAM_B2, H.ADAM_EPS, gs,
                                    P(sd), None), 'straps_adam_step')
    z.check()
    return pd.detach().cpu(), md.detach().cpu(), vd.detach().cpu()


@pytest.mark.parametrize('step', H.ADAM_STEPS)
@pytest.mark.parametrize('n', H.ADAM_N)
def test_adam_step(dev, n, step):
    """host `step` and the same step through `step_dev` (a device int64, step = 0 on the host side), grad_scale 1, 1/2 and 1/3; n = 1048576 is
    4096 workgroups exactly, 1048577 one element into the grid-stride loop's second trip.  The device form must meet the same bounds; whether it is
    bit-identical to the host form (pow() of the device against the host's) is printed, not asserted (on an MI355X: identical in all 54 launches)."""
    p, g, m, v = H.adam_data(n, step)
    for gs in H.ADAM_GRAD_SCALES:
        r = H.adam_reference(p, g, m, v, step, gs)
        normal = r['v'] >= 2.0 ** -126
        res = {}
        for form in ('host', 'device'):
            pn, mn, vn = res[form] = _adam_run(dev, p, g, m, v, step, gs, form == 'device')
            H.check_ratio('adam m [%s]' % form, mn, r['m'], r['m_bound'])
            assert bool((vn >= 0).all()), 'exp_avg_sq is negative or NaN somewhere'
            H.check_ratio('adam v [%s]' % form, vn[normal], r['v'][normal], r['v_bound'][normal])
            H.check_ratio('adam p [%s]' % form, pn, r['p'], r['p_bound'])
            assert torch.equal(H.bits(pn[r['untouched']]), H.bits(p[r['untouched']])), 'an element with g = m = v = 0 changed'
        same = all(torch.equal(H.bits(a), H.bits(b)) for a, b in zip(res['host'], res['device']))
        print('INFO adam n=%d step=%d grad_scale=%.4f: the device-step form is %sbit-identical to the host form' % (n, step, gs, '' if same else 'NOT '))


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_mse_fwd / straps_mse_bwd

def _mse_fwd(dev, pred, tgt, mask, scale):
    L = hipabi.lib()
    z = Zone(dev)
    rows, cols = pred.shape
    out3, ws = z.guarded((3,), name='out3'), z.guarded((512,), name='workspace')
    hipabi.check(L.straps_mse_fwd(P(z.at_end(pred)), P(z.at_end(tgt)), P(z.at_end(mask)), rows, cols, scale[0], scale[1], P(out3), P(ws), None), 'straps_mse_fwd')
    z.check()
    return out3.detach().cpu()


@pytest.mark.parametrize('rows,cols', H.MSE)
def test_mse_fwd(dev, rows, cols):
    for mk in H.MSE_MASKS:
        for sc in H.MSE_SCALES:
            pred, tgt, mask = H.mse_data(rows, cols, mk, sc)
            r = H.mse_reference(pred, tgt, mask, sc)
            out3 = _mse_fwd(dev, pred, tgt, mask, sc)
            assert float(out3[1]) == float(r['count']), 'count %r, want %d (%s mask)' % (float(out3[1]), r['count'], mk)
            H.check_ratio('mse_fwd sum', out3[0:1], torch.tensor([r['sum']], dtype=torch.float64), r['sum_bound'])
            H.check_ratio('mse_fwd mean', out3[2:3], torch.tensor([r['mean']], dtype=torch.float64), r['mean_bound'])


@pytest.mark.parametrize('rows,cols', [(7, 10), (65537, 1)])
def test_mse_fwd_all_rows_masked(dev, rows, cols):
    """sum and count +0.0, mean NaN: what a mean over nothing gives in the reference"""
    pred, tgt, mask = H.mse_data(rows, cols, 'none', H.MSE_SCALES[1])
    out3 = _mse_fwd(dev, pred, tgt, mask, H.MSE_SCALES[1])
    assert int(H.bits(out3)[0]) == 0 and int(H.bits(out3)[1]) == 0 and bool(torch.isnan(out3[2]))


@pytest.mark.parametrize('rows,cols', H.MSE + H.MSE_BWD_EXTRA)
def test_mse_bwd(dev, rows, cols):
    L = hipabi.lib()
    coef = torch.tensor([-0.37])
    for mk in H.MSE_MASKS + ('none',):
        for sc in H.MSE_SCALES:
            pred, tgt, mask = H.mse_data(rows, cols, mk, sc)
            r = H.mse_reference(pred, tgt, mask, sc)
            z = Zone(dev)
            grad = z.guarded((rows, cols), name='grad')
            hipabi.check(L.straps_mse_bwd(P(z.at_end(pred)), P(z.at_end(tgt)), P(z.at_end(mask)), rows, cols, sc[0], sc[1], P(z.at_end(coef)), P(grad), None),
                         'straps_mse_bwd')
            z.check()
            g = grad.detach().cpu()
            assert bool((H.bits(g[~r['keep']]) == 0).all()), 'a masked row is not exactly +0.0'
            c = float(coef[0])
            H.check_ratio('mse_bwd', g[r['keep']], c * r['d'][r['keep']], 4 * H.U * abs(c) * r['mag'][r['keep']])
