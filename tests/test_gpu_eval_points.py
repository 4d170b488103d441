"""GPU: straps_point_align (csrc/metrics.hip) on the point cases of tests/eval_cases.py: its error sums equal straps_point_metrics bit for bit
and the float64 restatement to the project's bar for this kernel; every coordinate of the corrected / aligned points is within 1 fp32 ulp
of the frame's largest coordinate of the float64 result; null outputs leave the others unchanged.  Every output sits between redzone
margins, NaN-filled: an element the kernel does not write shows as NaN, a write outside as a damaged margin."""
import numpy as np
import pytest
import torch

import eval_cases as EC
import straps_amd
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


_REF = {}


def _reference(name):
    """float64 restatement, computed once per case and shared"""
    if name not in _REF:
        pred, target = EC.point_case(name)
        _REF[name] = (pred, target) + EC.aligned_points64(pred, target)
    return _REF[name]


def _align(dev, pred, target, want=(True, True, True)):
    """the raw library call on guarded buffers -> (out3, pred_sc, pred_pa) numpy, None where not requested"""
    B, N = pred.shape[0], pred.shape[1]
    z = Zone(dev)
    p, t = z.at_end(torch.from_numpy(pred)), z.at_end(torch.from_numpy(target))
    bufs = [z.guarded(s, name=n) if w else None for w, s, n in zip(want, ((B, 3), (B, N, 3), (B, N, 3)), ('out3', 'pred_sc', 'pred_pa'))]
    hipabi.check(hipabi.lib().straps_point_align(hipabi.ptr(p), hipabi.ptr(t), hipabi.ptr(bufs[0]), hipabi.ptr(bufs[1]), hipabi.ptr(bufs[2]), B, N,
                                                 hipabi.stream_ptr()), 'straps_point_align')
    torch.cuda.synchronize()
    z.check()
    return tuple(None if b is None else b.cpu().numpy() for b in bufs)


def _metrics(dev, pred, target):
    z = Zone(dev)
    out = z.guarded((pred.shape[0], 3), name='out3')
    p, t = z.at_end(torch.from_numpy(pred)), z.at_end(torch.from_numpy(target))
    hipabi.check(hipabi.lib().straps_point_metrics(hipabi.ptr(p), hipabi.ptr(t), hipabi.ptr(out), pred.shape[0], pred.shape[1], hipabi.stream_ptr()),
                 'straps_point_metrics')
    torch.cuda.synchronize()
    z.check()
    return out.cpu().numpy()


def _bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize('name', EC.POINT_CASES)
def test_point_align_against_point_metrics_and_the_float64_restatement(dev, name):
    pred, target, sums64, sc64, pa64 = _reference(name)
    out3, sc, pa = _align(dev, pred, target)
    assert not np.isnan(out3).any() and not np.isnan(sc).any() and not np.isnan(pa).any(), 'an output element was not written'
    assert np.array_equal(_bits(out3), _bits(_metrics(dev, pred, target))), 'out3 differs from straps_point_metrics'
    EC.assert_sums_close(out3, sums64, name, pred, target)
    worst = 0.0
    for what, got, want in (('pred_sc', sc, sc64), ('pred_pa', pa, pa64)):
        ulps = np.abs(got.astype(np.float64) - want).reshape(len(want), -1).max(1) / EC.ulp32_of_largest(want)
        print('%s %s: largest error %.3f fp32 ulp of the frame\'s largest coordinate' % (name, what, ulps.max()))
        worst = max(worst, float(ulps.max()))
        assert (ulps <= 1.0).all(), (name, what, ulps)
    print('%s: worst %.3f ulp' % (name, worst))


@pytest.mark.parametrize('name', EC.POINT_CASES)
def test_null_outputs_leave_the_others_unchanged(dev, name):
    pred, target = _reference(name)[:2]
    full = _align(dev, pred, target)
    for want in ((True, True, False), (True, False, True), (False, True, True), (True, False, False), (False, True, False), (False, False, True)):
        part = _align(dev, pred, target, want)
        for w, a, b in zip(want, part, full):
            assert (a is None) == (not w)
            if w:
                assert np.array_equal(_bits(a), _bits(b)), (name, want)


def test_three_points(dev):
    """N = 3 (rank-2 cross-covariance in both sets): the construction needs no third singular value (tests/test_eval_cases_cpu.py), and the
    kernel agrees with the float64 restatement like on any other case"""
    from detgen import det_metrics_case
    pred, target = det_metrics_case(3, 306, batch=3)
    s = EC.cross_covariance_singular_values(pred, target)
    assert (s[:, 1] / s[:, 0]).min() >= 0.05
    sums64, sc64, pa64 = EC.aligned_points64(pred, target)
    out3, sc, pa = _align(dev, pred, target)
    np.testing.assert_allclose(out3, sums64, rtol=5e-5)
    for got, want in ((sc, sc64), (pa, pa64)):
        assert (np.abs(got.astype(np.float64) - want).reshape(3, -1).max(1) <= EC.ulp32_of_largest(want)).all()


def test_module_function(dev):
    """metrics.aligned_points: the same three arrays as device tensors; point_error_sums unchanged beside it"""
    pred, target, sums64, sc64, pa64 = _reference('det_b3_n14')
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)
    sums, sc, pa = straps_amd.metrics.aligned_points(p, t)
    assert sums.shape == (3, 3) and sc.shape == pa.shape == p.shape and sums.is_cuda and sc.dtype == pa.dtype == torch.float32
    assert torch.equal(sums, straps_amd.metrics.point_error_sums(p, t))
    raw = _align(dev, pred, target)
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(raw[1])) and np.array_equal(_bits(pa.cpu().numpy()), _bits(raw[2]))
    with pytest.raises(RuntimeError):
        straps_amd.metrics.aligned_points(p[:, :2], t[:, :2])
