"""GPU: straps_val_head (csrc/val.hip) -- the forward-only head of a validation step: five task losses, eleven per-sample metric sums and
the device-resident accumulator -- against float64 restatements, behind redzones, on the poisoned allocator.

Bounds (derived, not measured):
  * batch_out: every sum is taken in fp64 from the fp32 inputs and every stored value is rounded to fp32 once.  One fp32 rounding is
    2^-24 relative; fp64 accumulation of at most 1e5 terms adds about 1e5 * 2^-53 = 2^-36.  Both sit inside 2^-22 times the magnitude of
    the terms that make up the value: |mse * exp(-lv)| + |lv| for a task, the sum of the five for the total.
  * per_sample columns 0-7: the project's bar for the aligned-point mathematics, eval_cases.assert_sums_close against
    eval_cases.kernel_emulation64.
  * per_sample columns 8-10: numpy float64, rtol 2^-22; the pixel distances carry a floor of 17 * 2^-40 * max|coordinate| (17 square roots of
    fp64 differences of values of that size).
"""
import functools

import numpy as np
import pytest
import torch

import eval_cases as EC
import loss_cases as LC
import redzone
from detgen import det_metrics_case
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
H36M14 = [73 + k for k in (6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10)]
COCO = [24, 26, 25, 28, 27, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8]
REL = 2.0 ** -22
WH = LC.IMG_WH


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, launcher, restatements
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(B, nverts, ld_est=160, seed=60, j2d_range=(-40.0, 300.0)):
    """loss_cases.make_inputs cut to `nverts` vertices, plus reposed vertices (prep, trep) from detgen.  Shared between tests: never modified
    in place (`_copy` first)."""
    x = LC.make_inputs(B, ld_est=ld_est, seed=seed, j2d_range=j2d_range)
    x['pverts'] = x['pverts'][:, :nverts].contiguous()
    x['tverts'] = x['tverts'][:, :nverts].contiguous()
    pr, tr = det_metrics_case(nverts, seed + 20, batch=B)
    x['prep'], x['trep'] = torch.from_numpy(pr), torch.from_numpy(tr)
    return x


def _copy(x):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else dict(v) if isinstance(v, dict) else v) for k, v in x.items()}


def run_head(x, outputs=('batch', 'rows', 'acc'), reposed=True, acc_init=None, expect_rc=0, overrides=None, zone=None, acc=None):
    """one straps_val_head call through the C ABI: operands at the end of poison, every output and the workspace (exactly the advertised
    size) guarded.  -> dict of CPU tensors (absent outputs None).  overrides: {'batch' | 'nverts' | 'ld_est': value, 'prep' / 'trep': None}."""
    L = hipabi.lib()
    z = redzone.Zone(DEV) if zone is None else zone
    B, ld = x['est'].shape
    nverts = x['pverts'].shape[1]
    o = dict(batch=B, nverts=nverts, ld_est=ld)
    o.update(overrides or {})
    t = {k: z.at_end(x[k]) for k in ('pverts', 'joints', 'est', 'prot', 'tverts', 'tj2d', 'tj3d', 'tshape', 'trot')}
    t['prep'] = z.at_end(x['prep']) if reposed and o.get('prep', 1) is not None else None
    t['trep'] = z.at_end(x['trep']) if reposed and o.get('trep', 1) is not None else None
    lvd = z.at_end(torch.tensor([x['lv0'][k] for k in LC.ORDER], dtype=torch.float32))
    out = z.guarded((12,), name='batch_out') if 'batch' in outputs else None
    rows = z.guarded((B, 11), name='per_sample') if 'rows' in outputs else None
    if acc is None and 'acc' in outputs:
        acc = z.guarded((24,), dtype=torch.float64, name='acc')
        acc.copy_(torch.zeros(24, dtype=torch.float64) if acc_init is None else torch.as_tensor(acc_init, dtype=torch.float64))
    nbytes = L.straps_val_head_workspace_bytes(B)
    assert nbytes == B * (16 * 8 + 11 * 4) and nbytes % 4 == 0
    ws = z.guarded((nbytes // 4,), name='workspace')
    p = hipabi.ptr
    rc = L.straps_val_head(p(t['pverts']), p(t['prep']), p(t['joints']), p(t['est']), o['ld_est'], p(t['prot']), p(t['tverts']), p(t['trep']), p(t['tj2d']),
                           p(t['tj3d']), p(t['tshape']), p(t['trot']), p(lvd), p(out), p(rows), p(acc), p(ws), o['batch'], o['nverts'], WH, None)
    assert rc == expect_rc, 'return code %d, expected %d: %s' % (rc, expect_rc, L.straps_last_error().decode())
    z.check()
    res = dict(batch=None if out is None else out.cpu(), rows=None if rows is None else rows.cpu(), acc=None if acc is None else acc.cpu(),
               error=L.straps_last_error().decode() if rc else '')
    return res


@functools.lru_cache(maxsize=None)
def _loss_reference(B, nverts, seed=60, j2d_range=(-40.0, 300.0)):
    return LC.reference(_inputs(B, nverts, 160, seed, j2d_range))['loss'].numpy()


def assert_batch_out(got, ref, lv0):
    """got [12] fp32 against the oracle's [12] fp64 under the module docstring's bound"""
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    lv = np.array([lv0[k] for k in LC.ORDER], np.float64)
    mag = np.abs(ref[6:11] * np.exp(-lv)) + np.abs(lv)
    for k in range(5):
        if np.isnan(ref[1 + k]):
            continue
        assert abs(got[1 + k] - ref[1 + k]) <= REL * mag[k], ('weighted', k, got[1 + k], ref[1 + k])
        assert abs(got[6 + k] - ref[6 + k]) <= REL * mag[k], ('mse', k, got[6 + k], ref[6 + k])
    if not np.isnan(ref[0]):
        assert abs(got[0] - ref[0]) <= REL * mag.sum(), ('total', got[0], ref[0])
    assert got[11] == ref[11]


def rows_reference(x, reposed=True):
    """-> ([B,8] float64 columns 0-7 by eval_cases.kernel_emulation64, [B,3] float64 columns 8-10)"""
    f64 = lambda k: x[k].numpy().astype(np.float64)
    B = x['est'].shape[0]
    pts = np.zeros((B, 8))
    pts[:, 0:3] = EC.kernel_emulation64(x['pverts'].numpy(), x['tverts'].numpy())[0]
    if reposed:
        pts[:, 3:5] = EC.kernel_emulation64(x['prep'].numpy(), x['trep'].numpy())[0][:, :2]
    pts[:, 5:8] = EC.kernel_emulation64(x['joints'].numpy()[:, H36M14], x['tj3d'].numpy())[0]
    est, J = f64('est'), f64('joints')
    tail = np.zeros((B, 3))
    tail[:, 0] = ((est[:, 147:157] - f64('tshape')) ** 2).sum(1)
    tail[:, 1] = ((f64('prot') - f64('trot')) ** 2).reshape(B, -1).sum(1)
    uv = est[:, None, 0:1] * (J[:, COCO, :2] + est[:, None, 1:3])          # orthographic projection (utils/cam_utils.py:21-22)
    tail[:, 2] = np.linalg.norm((uv + 1.0) * (WH / 2.0) - f64('tj2d'), axis=-1).sum(1)      # undo_keypoint_normalisation, then pixel distances
    return pts, tail


def assert_rows(got, x, reposed=True, name='val_head', zero=False):
    got = np.asarray(got, np.float64)
    pts, tail = rows_reference(x, reposed)
    nm = 'hand_identical' if zero else name                    # (zero: every point sum is rounding noise -- eval_cases.sums_atol's floor)
    EC.assert_sums_close(got[:, 0:3], pts[:, 0:3], nm, x['pverts'].numpy(), x['tverts'].numpy())
    if reposed:
        rep = np.concatenate([got[:, 3:5], got[:, 2:3]], 1), np.concatenate([pts[:, 3:5], got[:, 2:3]], 1)      # (third column: a filler equal to itself)
        EC.assert_sums_close(rep[0], rep[1], nm, x['prep'].numpy(), x['trep'].numpy())
    else:
        assert (got[:, 3:5] == 0).all()
    EC.assert_sums_close(got[:, 5:8], pts[:, 5:8], nm, x['joints'].numpy()[:, H36M14], x['tj3d'].numpy())
    floor = np.array([0.0, 0.0, 17 * 2.0 ** -40 * float(max(np.abs(x['tj2d'].numpy()).max(), WH))])
    assert (np.abs(got[:, 8:11] - tail) <= REL * np.abs(tail) + floor[None]).all(), (got[:, 8:11], tail)


def acc_expected(batch_out, rows, B):
    """what one call adds to a zero accumulator, with the kernel's own operations: B * float64(fp32 loss), a sequential float64 loop over rows"""
    a = np.zeros(24)
    a[0:11] = float(B) * batch_out.numpy().astype(np.float64)[0:11]
    a[11] = float(batch_out[11])
    r = rows.numpy().astype(np.float64)
    for k in range(11):
        s = 0.0
        for b in range(B):
            s += r[b, k]
        a[12 + k] = s
    a[23] = float(B)
    return a


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------------------
# against float64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld_est', [157, 160])
@pytest.mark.parametrize('nverts', [3, 255, 256, 257, 6890])
@pytest.mark.parametrize('batch', [1, 2, 5])
def test_head_against_float64(batch, nverts, ld_est):
    x = _inputs(batch, nverts, ld_est)
    res = run_head(x)
    print('batch_out', res['batch'].numpy(), 'oracle', _loss_reference(batch, nverts))
    assert_batch_out(res['batch'].numpy(), _loss_reference(batch, nverts), x['lv0'])
    assert_rows(res['rows'].numpy(), x)
    assert same_bits(res['acc'].numpy(), acc_expected(res['batch'], res['rows'], batch))


@pytest.mark.parametrize('case', EC.POINT_CASES)
def test_point_cases_as_vertices(case):
    """eval_cases' point cases (sizes around the 256-thread stride, identical / similar / flat / mirrored hand cases) as the vertex sets"""
    pred, target = EC.point_case(case)
    B = pred.shape[0]
    x = _copy(_inputs(B, 3))
    x['pverts'], x['tverts'] = torch.from_numpy(pred), torch.from_numpy(target)
    x['prep'], x['trep'] = torch.from_numpy(pred).flip(0).contiguous(), torch.from_numpy(target).flip(0).contiguous()
    res = run_head(x, outputs=('rows',))
    got = res['rows'].numpy().astype(np.float64)
    want = EC.kernel_emulation64(pred, target)[0]
    EC.assert_sums_close(got[:, 0:3], want, case, pred, target)
    atol = EC.sums_atol(case, pred, target)
    assert (np.abs(got[:, 3:5] - want[::-1, :2]) <= 5e-5 * np.abs(want[::-1, :2]) + atol[None, :2]).all(), (case, got[:, 3:5], want[::-1, :2])


# ------------------------------------------------------------------------------------------------------------------------------
# accumulator
# ------------------------------------------------------------------------------------------------------------------------------
def test_accumulator_adds_two_batches_bit_for_bit():
    xa, xb = _inputs(2, 257, 160, 60), _inputs(5, 257, 160, 90)
    a, b = run_head(xa)['acc'].numpy(), run_head(xb)['acc'].numpy()
    z = redzone.Zone(DEV)
    acc = z.guarded((24,), dtype=torch.float64, name='acc')
    acc.zero_()
    run_head(xa, zone=z, acc=acc)
    both = run_head(xb, zone=z, acc=acc)['acc'].numpy()
    assert same_bits(both, a + b), (both, a + b)
    assert both[23] == 7.0 and np.isfinite(both).all()


def test_accumulator_under_graph_replay():
    """the same two calls captured once on one stream and replayed"""
    L, p = hipabi.lib(), hipabi.ptr
    xa, xb = _inputs(2, 257, 160, 60), _inputs(5, 257, 160, 90)
    a, b = run_head(xa)['acc'].numpy(), run_head(xb)['acc'].numpy()
    z = redzone.Zone(DEV)
    acc = z.guarded((24,), dtype=torch.float64, name='acc')
    calls = []
    for x in (xa, xb):
        B = x['est'].shape[0]
        t = {k: z.at_end(x[k]) for k in ('pverts', 'prep', 'joints', 'est', 'prot', 'tverts', 'trep', 'tj2d', 'tj3d', 'tshape', 'trot')}
        t['lv'] = z.at_end(torch.tensor([x['lv0'][k] for k in LC.ORDER], dtype=torch.float32))
        t['ws'] = z.guarded((L.straps_val_head_workspace_bytes(B) // 4,), name='workspace')
        calls.append((t, B))

    def launch():
        for t, B in calls:
            hipabi.check(L.straps_val_head(p(t['pverts']), p(t['prep']), p(t['joints']), p(t['est']), 160, p(t['prot']), p(t['tverts']), p(t['trep']),
                                           p(t['tj2d']), p(t['tj3d']), p(t['tshape']), p(t['trot']), p(t['lv']), None, None, p(acc), p(t['ws']), B, 257, WH,
                                           hipabi.stream_ptr()), 'straps_val_head')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    acc.zero_()
    g.replay()
    torch.cuda.synchronize()
    z.check()
    assert same_bits(acc.cpu().numpy(), a + b)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(acc.cpu().numpy(), (a + b) + a + b)


# ------------------------------------------------------------------------------------------------------------------------------
# independence
# ------------------------------------------------------------------------------------------------------------------------------
PER_SAMPLE_KEYS = ('pverts', 'tverts', 'prep', 'trep', 'joints', 'est', 'prot', 'tj2d', 'tj3d', 'tshape', 'trot')


def _pick(x, idx):
    y = _copy(x)
    for k in PER_SAMPLE_KEYS:
        y[k] = x[k][idx].contiguous()
    return y


def test_rows_do_not_depend_on_position_run_or_neighbours():
    x = _inputs(5, 257)
    alone = [run_head(_pick(x, [i]), outputs=('rows',))['rows'].numpy()[0] for i in range(5)]
    for r in range(5):                                   # sample i sits at position (i + r) % 5: every sample at every position
        order = [(q - r) % 5 for q in range(5)]
        rows = run_head(_pick(x, order), outputs=('rows',))['rows'].numpy()
        for q, i in enumerate(order):
            assert same_bits(rows[q], alone[i]), (r, q, i)
    first, again = run_head(x)['rows'].numpy(), run_head(x)['rows'].numpy()
    assert same_bits(first, again)
    y = _copy(x)
    for k in PER_SAMPLE_KEYS:
        y[k][2] = float('nan')                           # one body that is all NaN
    rows = run_head(y, outputs=('rows',))['rows'].numpy()
    assert np.isnan(rows[2][[0, 1, 2, 5, 6, 7, 8, 9, 10]]).all()
    for q in (0, 1, 3, 4):
        assert same_bits(rows[q], first[q]), q


def test_null_outputs_and_null_reposed():
    x = _inputs(2, 255)
    full = run_head(x)
    for only in ('batch', 'rows', 'acc'):
        one = run_head(x, outputs=(only,))
        assert same_bits(one[only].numpy(), full[only].numpy()), only
        assert all(one[k] is None for k in ('batch', 'rows', 'acc') if k != only)
    bare = run_head(x, reposed=False)
    assert same_bits(bare['batch'].numpy(), full['batch'].numpy())
    assert (bare['rows'].numpy()[:, 3:5] == 0).all() and (full['rows'].numpy()[:, 3:5] > 0).all()
    keep = [0, 1, 2, 5, 6, 7, 8, 9, 10]
    assert same_bits(bare['rows'].numpy()[:, keep], full['rows'].numpy()[:, keep])
    assert (bare['acc'].numpy()[15:17] == 0).all()
    akeep = [k for k in range(24) if k not in (15, 16)]
    assert same_bits(bare['acc'].numpy()[akeep], full['acc'].numpy()[akeep])
    assert_rows(bare['rows'].numpy(), x, reposed=False)


# ------------------------------------------------------------------------------------------------------------------------------
# edges
# ------------------------------------------------------------------------------------------------------------------------------
def test_no_visible_joint():
    x = _inputs(2, 256, 160, 60, (300.0, 400.0))
    ref = _loss_reference(2, 256, 60, (300.0, 400.0))
    assert np.isnan(ref[[0, 2, 7]]).all() and ref[11] == 0
    res = run_head(x)
    assert_batch_out(res['batch'].numpy(), ref, x['lv0'])
    assert_rows(res['rows'].numpy(), x)                  # the pixel distances count every joint, visible or not
    acc = res['acc'].numpy()
    assert np.isnan(acc[[0, 2, 7]]).all() and acc[11] == 0 and np.isfinite(acc[12:]).all()


def test_one_visible_joint_and_targets_on_the_border():
    x = _copy(_inputs(2, 256, 160, 60, (300.0, 400.0)))
    x['tj2d'][1, 5] = torch.tensor([17.25, 200.5])
    ref = LC.reference(x)['loss'].numpy()
    assert ref[11] == 1
    res = run_head(x)
    assert_batch_out(res['batch'].numpy(), ref, x['lv0'])
    assert_rows(res['rows'].numpy(), x)
    # 0 and img_wh themselves are visible (strict comparisons, utils/joints2d_utils.py:23-32); one ulp outside is not
    y = _copy(_inputs(2, 256))
    y['tj2d'][0, :4] = torch.tensor([[0.0, 0.0], [256.0, 256.0], [0.0, 256.0], [256.0, 0.0]])
    y['tj2d'][1, :3] = torch.tensor([[float(np.nextafter(np.float32(256), np.float32(300))), 10.0], [10.0, -1e-30], [-0.0, 256.0]])
    ref = LC.reference(y)['loss'].numpy()
    res = run_head(y)
    assert_batch_out(res['batch'].numpy(), ref, y['lv0'])
    assert_rows(res['rows'].numpy(), y)


def test_zero_error():
    """prediction == target wherever the head compares arrays directly: the losses are exactly zero, the point sums rounding noise"""
    x = _copy(_inputs(3, 257))
    x['tverts'], x['trep'] = x['pverts'].clone(), x['prep'].clone()
    x['tj3d'] = x['joints'][:, H36M14].contiguous()
    x['tshape'] = x['est'][:, 147:157].contiguous()
    x['trot'] = x['prot'].clone()
    res = run_head(x)
    out = res['batch'].numpy()
    assert (out[[6, 8, 9, 10]] == 0).all() and (out[[1, 3, 4, 5]] == 0).all()
    assert_batch_out(out, LC.reference(x)['loss'].numpy(), x['lv0'])
    assert_rows(res['rows'].numpy(), x, zero=True)
    assert (res['rows'].numpy()[:, [0, 3, 5, 8, 9]] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what, overrides, outputs', [
    ('batch', {'batch': 0}, ('batch', 'rows', 'acc')),
    ('nverts', {'nverts': 2}, ('batch', 'rows', 'acc')),
    ('ld_est', {'ld_est': 156}, ('batch', 'rows', 'acc')),
    ('batch_out', {}, ()),
    ('tgt_reposed', {'trep': None}, ('batch', 'rows', 'acc')),
    ('pred_reposed', {'prep': None}, ('batch', 'rows', 'acc')),
])
def test_bad_arguments_are_refused_before_anything_is_written(what, overrides, outputs):
    x = _inputs(2, 255)
    res = run_head(x, outputs=outputs, overrides=overrides, expect_rc=1, acc_init=[float('nan')] * 24)
    assert 'straps_val_head' in res['error'] and ('`%s`' % what) in res['error'], res['error']
    for k in ('batch', 'rows', 'acc'):
        assert res[k] is None or bool(torch.isnan(res[k]).all()), 'a refused call wrote to %s' % k
