"""Test helper: the model variants, inputs and float64 / float32 oracle gradients of tests/test_gpu_smpl_bwd_edges.py, and the CPU checks
of their conditioning in tests/test_smpl_bwd_cases_cpu.py.  Everything is made with numpy from `synthetic_smpl_model` and `det_uniform`;
the reference is autograd of oracle/straps_oracle.py (`smpl_forward`, `batch_rodrigues`) alone.
"""
import os

import numpy as np
import torch

import straps_oracle as O
from detgen import det_uniform
from straps_amd.synthetic_smpl import synthetic_smpl_model

NV, NJ_OUT = 6890, 90
# the first and the last output joint of every class: regressed SMPL joints 0..23, picked vertices 24..44, J_regressor_extra 45..53,
# cocoplus 54..72, h36m 73..89
ONE_HOT_JOINTS = (0, 23, 24, 44, 45, 53, 54, 72, 73, 89)
DENSE_ROW_H36M = 5                      # 'dense_regressors': J_regressor_h36m row with ~400 non-zeros = output joint 73 + 5
WIDE_FIXED = (0, 1, 2, 3, 6886, 6887, 6888, 6889)


def cpu_threads():
    """threads the oracle may use: what the environment grants (OMP_NUM_THREADS), at most 16 -- never the machine's CPU count."""
    try:
        n = int(os.environ.get('OMP_NUM_THREADS', '16'))
    except ValueError:
        n = 16
    return max(1, min(16, n))


def real_magnitude_model(model):
    """the synthetic SMPL model with its blend directions scaled to the real model's magnitudes (missing #3): the synthetic
    posedirs are uniform +-1e-3 where SMPL_NEUTRAL's largest entries are one to two orders larger, and the shape directions about three times
    smaller than the real ones -- every 'm from float64' figure of the split-precision modes is a statement about the SMALL directions."""
    big = dict(model)
    big['posedirs'] = (np.asarray(model['posedirs'], dtype=np.float64) * 50.0).astype(np.float32)
    big['shapedirs'] = (np.asarray(model['shapedirs'], dtype=np.float64) * 3.0).astype(np.float32)
    return big


def _rigid(m):
    w = np.zeros_like(m['weights'])
    w[np.arange(NV), np.argmax(m['weights'], axis=1)] = 1.0
    m['weights'] = w
    return m


def _wide(m):
    """about 5 % of the vertices -- among them 0..3 and 6886..6889, the last real rows of the last 32-vertex tile -- weighted to 7 joints"""
    w = m['weights'].astype(np.float64)
    vs = np.unique(np.concatenate([np.arange(7, NV, 20), np.asarray(WIDE_FIXED)]))
    order = np.argsort(det_uniform((len(vs), 24), 9001, 0.0, 1.0), axis=1, kind='stable')[:, :7]
    vals = det_uniform((len(vs), 7), 9002, 0.2, 1.0).astype(np.float64)
    rows = np.zeros((len(vs), 24))
    np.put_along_axis(rows, order, vals, axis=1)
    w[vs] = rows / rows.sum(axis=1, keepdims=True)
    m['weights'] = w.astype(np.float32)
    return m


def _unskinned(m, joint=15):
    """no vertex is skinned to `joint`: its weight goes to the joint's parent"""
    w = m['weights'].astype(np.float64)
    w[:, int(m['parents'][joint])] += w[:, joint]
    w[:, joint] = 0.0
    m['weights'] = w.astype(np.float32)
    return m


def _chain(m):
    m['parents'] = np.arange(-1, 23, dtype=np.int32)                 # one chain of 24 joints, depth 23
    return m


def _shallow(m):
    m['parents'] = np.asarray([-1] + [(j - 1) // 3 for j in range(1, 24)], dtype=np.int32)   # every joint with up to 3 children, depth 3
    return m


def _dense_regressors(m):
    """a J_regressor row and a J_regressor_h36m row with 400 non-zeros on vertices 3200..3599: long joint-gradient lists in 13 tiles"""
    for key, row, seed in (('J_regressor', 7, 9011), ('J_regressor_h36m', DENSE_ROW_H36M, 9012)):
        r = np.zeros(NV)
        r[3200:3600] = det_uniform((400,), seed, 0.2, 1.0)
        a = m[key].astype(np.float64)
        a[row] = r / r.sum()
        m[key] = a.astype(np.float32)
    return m


MODEL_VARIANTS = {
    'seed0': lambda: synthetic_smpl_model(0),
    'seed1': lambda: synthetic_smpl_model(1),
    'real_magnitude': lambda: real_magnitude_model(synthetic_smpl_model(0)),
    'rigid': lambda: _rigid(synthetic_smpl_model(0)),
    'wide': lambda: _wide(synthetic_smpl_model(0)),
    'unskinned_joint': lambda: _unskinned(synthetic_smpl_model(0)),
    'chain_tree': lambda: _chain(synthetic_smpl_model(0)),
    'shallow_tree': lambda: _shallow(synthetic_smpl_model(0)),
    'dense_regressors': lambda: _dense_regressors(synthetic_smpl_model(0)),
}
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = MODEL_VARIANTS[name]()
    return _MODELS[name]


# ---- the case matrix -------------------------------------------------------------------------------------------------------------------
# name -> dict(model, B, pose (axis-angle range), beta (range), up (upstream gradient), kinds, chunks, special)
#   up: 'dense' | ('verts', lo, hi) | ('body', b) | ('joint', j)
#   special: 'identity_body' (body 1 at the all-zero axis-angle), 'big_beta' (body 0 with |beta| up to 10), 'off_manifold' (rotation
#   matrices R + 0.05 uniform: straps_smpl_bwd only)
def _case(model='seed0', B=3, pose=0.8, beta=2.5, up='dense', kinds=('both',), chunks=(0,), special=(), seed=None):
    return dict(model=model, B=B, pose=pose, beta=beta, up=up, kinds=kinds, chunks=chunks, special=special, seed=seed)


CASES = {}
# one body: every per-component "maximum over bodies" of dbetas is a single value, and a component that happens to be a near-cancellation
# of its terms is ill-conditioned in any fp32 evaluation (seed 3000: the FLOAT32 ORACLE is 1.2e-4 from float64 on one component).  The
# seed below was picked among ten by the oracle alone: float32 autograd within 2e-6 of float64 on every slice, like the larger batches.
CASES['batch1'] = _case(B=1, seed=4003)
for _B in (31, 32, 65):
    CASES['batch%d' % _B] = _case(B=_B)
CASES['batch33'] = _case(B=33, kinds=('both', 'verts', 'joints'), chunks=(0, 1, 3, 5, 8, 54, 100))
CASES['batch64'] = _case(B=64, chunks=(0, 1, 3, 5, 8, 54, 100))
CASES['batch1024'] = _case(B=1024, chunks=(5, 54))
CASES['pose3'] = _case(B=6, pose=3.0, kinds=('both', 'verts', 'joints'), special=('identity_body',))
CASES['big_beta'] = _case(B=6, special=('big_beta', 'identity_body'))
CASES['off_manifold'] = _case(B=6, special=('off_manifold',))
for _m in MODEL_VARIANTS:
    if _m != 'seed0':
        CASES['model_' + _m] = _case(model=_m, B=5, special=('big_beta',) if _m == 'real_magnitude' else ())
CASES['verts_last_tile'] = _case(up=('verts', 6880, 6890), kinds=('verts',))
CASES['verts_first_tile'] = _case(up=('verts', 0, 32), kinds=('verts',))
CASES['one_body'] = _case(B=5, up=('body', 3))
for _j in ONE_HOT_JOINTS:
    CASES['onehot%d' % _j] = _case(up=('joint', _j), kinds=('joints',))
CASES['wide_last_tile'] = _case(model='wide', up=('verts', 6880, 6890), kinds=('verts',))
CASES['wide_first_tile'] = _case(model='wide', up=('verts', 0, 32), kinds=('verts',))
CASES['dense_regressors_onehot'] = _case(model='dense_regressors', up=('joint', 73 + DENSE_ROW_H36M), kinds=('joints',))
CASES['chain_tree_onehot23'] = _case(model='chain_tree', up=('joint', 23), kinds=('joints',))
DENSE = [n for n, c in CASES.items() if c['up'] == 'dense']
SPARSE = [n for n, c in CASES.items() if c['up'] != 'dense']


def _seed(name):
    return CASES[name]['seed'] or 3000 + 16 * list(CASES).index(name)


_FLOOR = []


def float32_floor():
    """the float32 oracle's worst slice error against the float64 oracle over the WHOLE case matrix (every case, kind and output tensor):
    the floor of the measured bar.  From the reference arithmetic alone; computed once per process (the oracles are cached for the tests)."""
    import grad_metrics as G
    if not _FLOOR:
        w, where = 0.0, None
        for name, c in CASES.items():
            for kind in c['kinds']:
                r64, r32 = oracle(name, kind, torch.float64), oracle(name, kind, torch.float32)
                for k, ref in r64.items():
                    if ref is not None:
                        e = G.worst(G.slice_errors(r32[k], ref, c['up'] != 'dense'))
                        if e > w:
                            w, where = e, '%s/%s %s' % (name, kind, k)
        _FLOOR.extend([w, where])
    return _FLOOR[0]


def float32_floor_case():
    """the case / tensor on which float32_floor() was met"""
    float32_floor()
    return _FLOOR[1]


_INPUTS = {}


def inputs(name):
    """-> dict(betas [B,10], aa [B,72] | None, R [B,24,3,3] fp32, gv [B,6890,3], gj [B,90,3]) CPU fp32 tensors; the last call is cached"""
    if name in _INPUTS:
        return _INPUTS[name]
    c, s = CASES[name], _seed(name)
    B = c['B']
    betas = det_uniform((B, 10), s, -c['beta'], c['beta'])
    aa = det_uniform((B, 72), s + 1, -c['pose'], c['pose'])
    if 'big_beta' in c['special']:
        betas[0] = np.asarray([10.0, -8.0, 6.0, 4.0, -4.0, 3.0, 3.0, -3.0, 2.0, 2.0], np.float32)
    if 'identity_body' in c['special']:
        aa[1] = 0.0
    aa = torch.from_numpy(aa)
    R = O.batch_rodrigues(aa.reshape(-1, 3)).view(B, 24, 3, 3)
    if 'off_manifold' in c['special']:
        R = R + 0.05 * torch.from_numpy(det_uniform((B, 24, 3, 3), s + 2))
        aa = None
    gv = det_uniform((B, NV, 3), s + 3)
    gj = det_uniform((B, NJ_OUT, 3), s + 4)
    up = c['up']
    if up != 'dense':
        if up[0] == 'verts':
            keep = np.zeros((1, NV, 1), np.float32)
            keep[:, up[1]:up[2]] = 1.0
            gv = gv * keep
        elif up[0] == 'body':
            keep = np.zeros((B, 1, 1), np.float32)
            keep[up[1]] = 1.0
            gv, gj = gv * keep, gj * keep
        elif up[0] == 'joint':
            keep = np.zeros((1, NJ_OUT, 1), np.float32)
            keep[:, up[1]] = 1.0
            gj = gj * keep
    _INPUTS.clear()
    _INPUTS[name] = dict(betas=torch.from_numpy(betas), aa=aa, R=R.contiguous(), gv=torch.from_numpy(gv), gj=torch.from_numpy(gj))
    return _INPUTS[name]


def oracle_grads(mdl, x, kind, dtype, block=64):
    """autograd of the oracle in `dtype`, `block` bodies at a time (bodies are independent) -> dict(dbetas [B,10], drot [B,24,3,3],
    daa [B,24,3] | None) float64 CPU tensors.  kind: 'both' | 'verts' (djoints absent) | 'joints' (dverts absent)."""
    B = x['betas'].shape[0]
    outs = {'dbetas': [], 'drot': [], 'daa': []}
    for lo in range(0, B, block):
        sl = slice(lo, min(lo + block, B))
        n = sl.stop - sl.start
        b = x['betas'][sl].to(dtype).requires_grad_()
        if x['aa'] is not None:
            a = x['aa'][sl].to(dtype).requires_grad_()
            R = O.batch_rodrigues(a.reshape(-1, 3)).view(n, 24, 3, 3)
            R.retain_grad()
        else:
            a, R = None, x['R'][sl].to(dtype).requires_grad_()
        v, j = O.smpl_forward(mdl, b, rotmats=R, dtype=dtype)
        loss = 0.0
        if kind in ('both', 'verts'):
            loss = loss + (v * x['gv'][sl].to(dtype)).sum()
        if kind in ('both', 'joints'):
            loss = loss + (j * x['gj'][sl].to(dtype)).sum()
        loss.backward()
        outs['dbetas'].append(b.grad.double())
        outs['drot'].append(R.grad.double())
        if a is not None:
            outs['daa'].append(a.grad.double().view(n, 24, 3))
    return {k: (torch.cat(v) if v else None) for k, v in outs.items()}


_ORACLE = {}


def oracle(name, kind, dtype):
    key = (name, kind, dtype)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_grads(model(CASES[name]['model']), inputs(name), kind, dtype)
    return _ORACLE[key]


def workspace_bytes_formula(batch, chunks):
    """the formula of include/straps_hip.h (straps_smpl_bwd_workspace_bytes): host arithmetic only"""
    if chunks <= 0:
        chunks = 8 if batch >= 1024 else 54
    chunks = min(chunks, 54)
    rounds_per_chunk = (54 + chunks - 1) // chunks
    used = (54 + rounds_per_chunk - 1) // rounds_per_chunk
    return batch * (1 + used) * (224 + 288) * 4
