"""GPU: the SMPL gradient (csrc/smpl_bwd.hip: straps_smpl_bwd, straps_smpl_bwd_aa) per joint, at its edges, behind redzones.

Reference: float64 autograd of oracle/straps_oracle.py (smpl_forward, batch_rodrigues).  The entry points are called through the C ABI,
so that `chunks` and the workspace are the test's: every output and the workspace (exactly straps_smpl_bwd_workspace_bytes) is a
guarded buffer pre-filled with NaN (tests/redzone.py), every input sits at the end of a NaN-poisoned allocation.

Metric (tests/grad_metrics.py): besides the tensor-max error of the older tests, a per-joint (per shape component) and a per-body
error, each against the slice's own maximum in the oracle; no element left out.  Dense upstream gradients: no floor (the CPU test
tests/test_smpl_bwd_cases_cpu.py asserts that no scale of the matrix is below 1e-3 of its tensor's maximum).  Sparse ones (one-hot
joints, single tiles, a single body): exact zeros where the oracle's slice is zero, scales clamped at 1e-3 of the tensor maximum.

Bars: the project's 1e-4 (CEILING) on every slice, and the measured bar
    error of a slice <= MULTIPLE x (error of the float32 oracle on that slice) + floor,
floor = the float32 oracle's worst slice error over the whole case matrix (smpl_cases.float32_floor(), evaluated at run time from the
reference arithmetic alone).  The kernel sums the same fp32 products in another order (32-vertex tiles, chunk partials, then the chain);
more than 32 x the float32 oracle's distance from float64 would not be a reordering of the same sums.

Measured on an MI355X (every case, kind and `chunks` of this file: 191 tensors; ratio = (kernel error - floor) / float32-oracle error of
the same slice, 0 where the kernel error is below the floor).  The float32 oracle is CPU arithmetic and depends on the host's BLAS:
  - host A: floor 2.1e-6 (dense_regressors_onehot, drot).  Worst ratios 5.9 (verts_last_tile daa, joint 8: kernel 4.2e-6, float32 oracle
    3.6e-7), 5.0 (the same case, drot), 3.6 (batch33 chunks=1 drot, joint 11: kernel 6.0e-6, float32 oracle 1.1e-6), 2.7 (shallow tree,
    drot joint 16).
  - host B (the GPU box's): floor 1.07e-5 (batch1024 dbetas, one body); no kernel error reaches it: worst ratio 0.
  - the kernel's worst slice errors: 6.0e-6 per joint (batch33, chunks=1: all 54 rounds summed in one workgroup), 2.5e-6 per body, 1.3e-6 by
    tensor maximum.
MULTIPLE = 16: the smallest power of two that is at least twice the worst ratio seen (2 x 5.9 = 11.8).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import straps_amd
import straps_oracle as O
import grad_metrics as G
import smpl_cases as S
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
CEILING = 1e-4
MULTIPLE = 16
RATIOS = []


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    hipabi.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _oracle_threads_and_report():
    before = torch.get_num_threads()
    torch.set_num_threads(S.cpu_threads())
    yield
    torch.set_num_threads(before)
    RATIOS.sort(reverse=True)
    print('\nfloat32 floor %.3e (%s); largest (kernel error - floor) / float32-oracle error:' % (S.float32_floor(), S.float32_floor_case()))
    for r in RATIOS[:12]:
        print('  ratio %7.3f  %s %s %d: kernel %.3e float32 oracle %.3e' % r)


_SMPL = {}


def _smpl(dev, name):
    if name not in _SMPL:
        _SMPL[name] = straps_amd.SMPL(S.model(name), batch_size=1).to(dev)
    return _SMPL[name]


def _on_device(z, x, kind):
    d = {k: z.at_end(x[k]) for k in ('betas', 'R', 'aa')}
    d['gv'] = z.at_end(x['gv']) if kind in ('both', 'verts') else None
    d['gj'] = z.at_end(x['gj']) if kind in ('both', 'joints') else None
    return d


def _launch(smpl, d, chunks, entry):
    """entry: 'rot' (straps_smpl_bwd) | 'aa' (straps_smpl_bwd_aa with drotmats) | 'aa_only' (drotmats = NULL).  A fresh set of guarded outputs and
    a guarded workspace of exactly the advertised size per launch -> dict of CPU tensors"""
    L = hipabi.lib()
    dev = d['betas'].device
    B = d['betas'].shape[0]
    z = Zone(dev)
    nbytes = L.straps_smpl_bwd_workspace_bytes(B, chunks)
    assert nbytes == S.workspace_bytes_formula(B, chunks)
    ws = z.guarded((nbytes // 4,), name='workspace')
    dbetas = z.guarded((B, 10), name='dbetas')
    drot = z.guarded((B, 24, 3, 3), name='drotmats') if entry != 'aa_only' else None
    p, ms = hipabi.ptr, C.byref(smpl._model_struct())
    if entry == 'rot':
        daa = None
        rc = L.straps_smpl_bwd(ms, p(d['betas']), p(d['R']), p(d['gv']), p(d['gj']), p(dbetas), p(drot), p(ws), B, chunks, hipabi.stream_ptr())
    else:
        daa = z.guarded((B, 24, 3), name='dfull_pose_aa')
        rc = L.straps_smpl_bwd_aa(ms, p(d['betas']), p(d['R']), p(d['aa']), p(d['gv']), p(d['gj']), p(dbetas), p(daa), p(drot), p(ws), B, chunks,
                                  hipabi.stream_ptr())
    hipabi.check(rc, 'straps_smpl_bwd' + ('' if entry == 'rot' else '_aa'))
    z.check()
    return {'dbetas': dbetas.cpu(), 'drot': None if drot is None else drot.cpu(), 'daa': None if daa is None else daa.cpu()}


def _rodrigues_bwd(dev, aa, drot):
    z = Zone(dev)
    n = aa.numel() // 3
    out = z.guarded((n, 3), name='daa')
    a, g = z.at_end(aa.reshape(n, 3)), z.at_end(drot.reshape(n, 9))
    hipabi.check(hipabi.lib().straps_rodrigues_bwd(hipabi.ptr(a), hipabi.ptr(g), hipabi.ptr(out), n, hipabi.stream_ptr()), 'straps_rodrigues_bwd')
    z.check()
    return out.cpu().view(-1, 24, 3)


def _same(a, b):
    return all((a[k] is None or b[k] is None) or torch.equal(a[k], b[k]) for k in a)


def _against_oracle(tag, got, name, kind, sparse, floor):
    r64, r32 = S.oracle(name, kind, torch.float64), S.oracle(name, kind, torch.float32)
    for k in ('dbetas', 'drot', 'daa'):
        if got[k] is not None:
            G.assert_slices('%s %s' % (tag, k), got[k], r64[k], CEILING, sparse, ref32=r32[k], multiple=MULTIPLE, floor=floor, ratios=RATIOS)


@pytest.mark.parametrize('name', list(S.CASES))
def test_smpl_backward_case_vs_float64_oracle(dev, name):
    """every case of smpl_cases.CASES: both entry points against the oracle under the per-joint / per-body metric; straps_smpl_bwd_aa ==
    straps_smpl_bwd + straps_rodrigues_bwd bit for bit; with explicit `chunks`: three launches bit-identical, and the results for
    different `chunks` within the measured bar of each other."""
    c = S.CASES[name]
    x = S.inputs(name)
    floor = S.float32_floor()
    smpl = _smpl(dev, c['model'])
    sparse = c['up'] != 'dense'
    explicit = any(ch != 0 for ch in c['chunks'])
    for kind in c['kinds']:
        d = _on_device(Zone(dev), x, kind)
        first = None
        for chunks in c['chunks']:
            tag = '%s/%s/chunks=%d' % (name, kind, chunks)
            rot = _launch(smpl, d, chunks, 'rot')
            got = dict(rot)
            if x['aa'] is not None:
                aa = _launch(smpl, d, chunks, 'aa')
                assert torch.equal(aa['dbetas'], rot['dbetas']) and torch.equal(aa['drot'], rot['drot']), tag
                assert torch.equal(aa['daa'], _rodrigues_bwd(dev, x['aa'], rot['drot'])), tag + ': fused != composed'
                assert _same(_launch(smpl, d, chunks, 'aa_only'), aa), tag + ': drotmats = NULL changes a result'
                got['daa'] = aa['daa']
            if explicit:
                for _ in range(2):
                    assert _same(_launch(smpl, d, chunks, 'rot' if x['aa'] is None else 'aa'), got), tag + ': not reproducible'
            _against_oracle(tag, got, name, kind, sparse, floor)
            if first is None:
                first = got
                continue
            # another summation order of the same products: not bit for bit, but within the measured bar of the first `chunks`
            r64, r32 = S.oracle(name, kind, torch.float64), S.oracle(name, kind, torch.float32)
            for k, v in got.items():
                if v is None:
                    continue
                e, e32 = G.slice_errors(v, first[k], sparse), G.slice_errors(r32[k], r64[k], sparse)
                for part in ('tensor', 'group', 'body'):
                    assert np.all(np.asarray(e[part]) <= MULTIPLE * np.asarray(e32[part]) + floor), '%s %s: differs from chunks=%d' % (tag, k, c['chunks'][0])
    if c['up'] != 'dense' and c['up'][0] == 'body':
        others = [b for b in range(c['B']) if b != c['up'][1]]
        for k, v in got.items():
            assert not v[others].any(), '%s: a body without upstream gradient has a non-zero %s' % (name, k)


@pytest.mark.parametrize('name', list(S.MODEL_VARIANTS))
def test_forward_of_every_model_variant_vs_float64_oracle(dev, name):
    """the backward recomputes v_posed: every model variant also goes through the forward (fp32 mode; 2e-5 m as every SMPL test of
    tests/test_gpu_forward.py)"""
    case = 'batch31' if name == 'seed0' else 'model_' + name
    x = S.inputs(case)
    smpl = _smpl(dev, name)
    v, j = smpl.forward_arrays(x['betas'].to(dev), x['R'].to(dev), precision='fp32')
    v64, j64 = O.smpl_forward(S.model(name), x['betas'].double(), rotmats=x['R'].double(), dtype=torch.float64)
    ev, ej = float((v.cpu().double() - v64).abs().max()), float((j.cpu().double() - j64).abs().max())
    print('%s: vertices %.2e m, joints %.2e m from float64' % (name, ev, ej))
    assert ev < 2e-5 and ej < 2e-5


def test_body_independence_at_equal_chunks(dev):
    """body b of a batch of 65 has the same bits alone and inside a batch of 7, at equal explicit `chunks` (no atomics, a fixed order)"""
    x = S.inputs('batch65')
    smpl = _smpl(dev, 'seed0')
    chunks = 5
    full = _launch(smpl, _on_device(Zone(dev), x, 'both'), chunks, 'aa')
    for sl in (slice(0, 1), slice(31, 32), slice(64, 65), slice(30, 37), slice(58, 65)):
        part = _launch(smpl, _on_device(Zone(dev), {k: v[sl] for k, v in x.items()}, 'both'), chunks, 'aa')
        for k in full:
            assert torch.equal(part[k], full[k][sl]), 'bodies %s: %s depends on the rest of the batch' % (sl, k)
