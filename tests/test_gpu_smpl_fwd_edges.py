"""GPU: the SMPL forward (csrc/smpl.hip: straps_smpl_fwd -- smpl_pose_kernel, the four vertex kernels, smpl_joints_kernel) on every
model variant, at its body-count and chunk edges, behind redzones.

Reference: the float64 oracle (oracle/straps_oracle.py: smpl_forward, batch_rodrigues), cached per case in tests/smpl_fwd_cases.py, whose
CPU companion tests/test_smpl_fwd_cases_cpu.py asserts that the float32 oracle is within 5e-6 m of it on every case used here.  The entry
point is called through the C ABI, so that `chunks`, the kernel choice and the workspace are the test's:
  * verts, joints and a workspace of exactly straps_smpl_workspace_bytes are guarded buffers pre-filled with NaN (tests/redzone.py): a
    store outside them damages a margin, an element nobody wrote stays NaN (a tile that a chunk boundary drops, a body past a group);
  * betas, rotmats and EVERY packed model table sit at the end of NaN-poisoned allocations: a read past a table whose value is used is a
    NaN in the result.  (Read from csrc/smpl.hip before this was first run: every table index is bounded by tile < n_tiles, j < 24,
    r < 63 or j < 45 -- the integer tables are never read past their end, so the poison behind them is never used as an index.)
Bar: 2e-5 m from float64 on vertices and joints, the bar of every SMPL test here (north_star: 1e-4).  A failure names the 32-vertex tile
and the output-joint class (chain 0..23, picked 24..44, regressed 45..53 / 54..72 / 73..89).

The relation "within 3 x the exact-fp32 kernel's error + 1e-6" is asserted for the parity-grade split modes fp16x3 and fp16x3_lbs, as in
tests/test_gpu_forward.py::test_smpl_split_precision_vs_oracle; the opt-in modes fp16x3_lbs_pd16 / _p16 round the pose-corrective
directions to plain fp16 and are held to the 2e-5 bar alone (test_smpl_pd16_mode_vs_oracle), and not run on 'real_magnitude', where
their 1e-3 / > 1e-4 pin lives in tests/test_gpu_forward.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import straps_amd
import smpl_fwd_cases as FC
from redzone import Zone
from straps_amd import hipabi
from straps_amd.smpl import KERNELS, PRECISIONS

pytestmark = pytest.mark.gpu
BAR = 2e-5
EINVAL = 1
MODES = {                                   # tag -> (precision, kernel)
    'fp32': ('fp32', 'auto'), 'fp16x3': ('fp16x3', 'auto'),
    'fp16x3_lbs/narrow': ('fp16x3_lbs', 'narrow'), 'fp16x3_lbs/wide': ('fp16x3_lbs', 'wide'), 'fp16x3_lbs/wide_builtin': ('fp16x3_lbs', 'wide_builtin'),
    'fp16x3_lbs_pd16/narrow': ('fp16x3_lbs_pd16', 'narrow'), 'fp16x3_lbs_pd16/wide': ('fp16x3_lbs_pd16', 'wide'),
    'fp16x3_lbs_p16/narrow': ('fp16x3_lbs_p16', 'narrow'), 'fp16x3_lbs_p16/wide': ('fp16x3_lbs_p16', 'wide'),
}
OPT_IN = tuple(t for t in MODES if '_pd16' in t or '_p16' in t)
PARITY_SPLIT = ('fp16x3', 'fp16x3_lbs/narrow', 'fp16x3_lbs/wide', 'fp16x3_lbs/wide_builtin')
SAME_BITS = (('fp16x3_lbs/narrow', 'fp16x3_lbs/wide', 'fp16x3_lbs/wide_builtin'), ('fp16x3_lbs_pd16/narrow', 'fp16x3_lbs_pd16/wide'),
             ('fp16x3_lbs_p16/narrow', 'fp16x3_lbs_p16/wide'))
EDGE_MODES = ('fp32', 'fp16x3', 'fp16x3_lbs/narrow', 'fp16x3_lbs/wide')       # the body-count and chunk edges: one tag per kernel
BODY_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128)   # (and 129, the whole case): 8 bodies per pose block, 4 per joints block,
BODY_CHUNKS = 5                                                              # 32 per narrow workgroup, 64 per wide one; `chunks` explicit: 28 rounds as 5 x 6 - 2
CHUNKS = (1, 2, 5, 9, 26, 27, 28, 29, 53, 54, 55, 56, 57, 100, 1000, -3)     # round counts: 28 / 27 (narrow, with / without joints), 56 / 54 (wide)
WORST = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    hipabi.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nworst error against float64 per mode, over every comparison of this file:')
    for tag, (e, where) in WORST.items():
        print('  %-26s %.3e m  (%s)' % (tag, e, where))


_SMPL = {}


def _smpl(dev, name):
    """the module of a variant with every packed table re-homed at the end of a NaN-poisoned allocation"""
    if name not in _SMPL:
        smpl = straps_amd.SMPL(FC.model(name), batch_size=1).to(dev)
        z = Zone(dev)
        for key, buf in list(smpl.named_buffers()):
            if key.startswith('_k_'):
                setattr(smpl, key, z.at_end(buf))
        smpl._struct_key = None
        p = FC.packed(name)
        assert (smpl.n_tiles, smpl.skin_k, smpl.max_depth) == (p['n_tiles'], p['skin_k'], p['max_depth'])
        _SMPL[name] = (smpl, z)
    return _SMPL[name][0]


def _nan_free(tag, v, j):
    for what, t, per in (('vertices', v, 32), ('joints', j, 1)):
        if t is not None and bool(torch.isnan(t).any()):
            cols = torch.isnan(t).any(dim=2)
            ids = sorted(set((cols.any(dim=0).nonzero().flatten() // per).tolist()))
            cls = '' if per == 32 else ' (classes: %s)' % ', '.join(n for n, lo, hi in FC.JOINT_CLASSES if any(lo <= i < hi for i in ids))
            raise AssertionError('%s: NaN left in the %s: %s %s%s of bodies %s' % (tag, what, 'tiles' if per == 32 else 'joints', ids[:16], cls,
                                                                                   cols.any(dim=1).nonzero().flatten()[:16].tolist()))


def _run(smpl, d, tag, chunks, joints=True, keep_ws=False):
    """one straps_smpl_fwd with fresh guarded outputs and a guarded workspace of exactly the advertised size -> (verts, joints | None[, workspace]) on the CPU"""
    L = hipabi.lib()
    B = d['betas'].shape[0]
    z = Zone(d['betas'].device)
    ms = C.byref(smpl._model_struct())
    nbytes = L.straps_smpl_workspace_bytes(ms, B)
    assert nbytes == FC.workspace_bytes_formula(B, smpl.n_tiles)
    ws = z.guarded((nbytes // 4,), name='workspace')
    v = z.guarded((B, FC.NV, 3), name='verts')
    j = z.guarded((B, FC.NJ_OUT, 3), name='joints') if joints else None
    prec, kern = MODES[tag]
    p = hipabi.ptr
    hipabi.check(L.straps_smpl_fwd(ms, p(d['betas']), p(d['R']), p(v), p(j), p(ws), B, chunks, PRECISIONS[prec] | KERNELS[kern], hipabi.stream_ptr()), 'straps_smpl_fwd')
    z.check()
    v, j = v.cpu(), None if j is None else j.cpu()
    _nan_free('%s chunks=%d B=%d' % (tag, chunks, B), v, j)
    return (v, j, ws.cpu()) if keep_ws else (v, j)


def _on_device(dev, x, sl=slice(None)):
    z = Zone(dev)
    return {'betas': z.at_end(x['betas'][sl]), 'R': z.at_end(x['R'][sl]), 'zone': z}


def _against_float64(tag, what, v, j, v64, j64):
    rep = FC.assert_close('%s, %s' % (what, tag), v, j, v64, j64, BAR)
    e = max(rep['verts'], rep['joints'])
    if e > WORST.get(tag, (-1.0, ''))[0]:
        WORST[tag] = (e, '%s: %s' % (what, FC.describe(rep)))
    return rep


@pytest.mark.parametrize('name', list(FC.FWD_VARIANTS))
def test_every_variant_through_every_kernel(dev, name):
    """B = 67: two narrow workgroups + 3 bodies, one wide group + 3, 16 joints blocks + 3, 8 pose blocks + 3."""
    case = 'var_' + name
    smpl = _smpl(dev, name)
    d = _on_device(dev, FC.inputs(case))
    v64, j64 = FC.oracle(case)
    pick = torch.as_tensor(np.asarray(FC.model(name)['extra_vertex_ids']), dtype=torch.long)
    got, rep = {}, {}
    for tag in MODES:
        if name == 'real_magnitude' and tag in OPT_IN:
            continue
        what = '%s B=%d' % (name, FC.VARIANT_B)
        v, j = got[tag] = _run(smpl, d, tag, 0)
        rep[tag] = _against_float64(tag, what, v, j, v64, j64)
        print('%s %-26s %s' % (name, tag, FC.describe(rep[tag])))
        FC.assert_same_bits('%s, %s: joints 24..44 are not copies of the picked vertices' % (what, tag), j[:, 24:45], v[:, pick], joints=True)
        if name == 'empty_regressor_row':
            assert not j[:, FC.EMPTY_JOINT].any(), '%s, %s: joint %d of the empty regressor row is not exactly zero' % (what, tag, FC.EMPTY_JOINT)
        v2, none = _run(smpl, d, tag, 0, joints=False)
        assert none is None
        FC.assert_same_bits('%s, %s: joints = NULL changes the vertices' % (what, tag), v2, v)
    for tag in PARITY_SPLIT:
        for k in ('verts', 'joints'):
            assert rep[tag][k] <= 3 * rep['fp32'][k] + 1e-6, \
                '%s, %s: %s, the exact-fp32 kernel %s' % (name, tag, FC.describe(rep[tag]), FC.describe(rep['fp32']))
    for group in SAME_BITS:
        for tag in group[1:]:
            if tag in got:
                FC.assert_same_bits('%s: %s against %s, vertices' % (name, tag, group[0]), got[tag][0], got[group[0]][0])
                FC.assert_same_bits('%s: %s against %s, joints' % (name, tag, group[0]), got[tag][1], got[group[0]][1], joints=True)


@pytest.mark.parametrize('tag', EDGE_MODES)
@pytest.mark.parametrize('name', ['seed0', 'wide'])
def test_body_count_edges(dev, name, tag):
    """129 bodies once, against float64; then the first B and the last B bodies of the same inputs for every B around the block sizes: each
    bit-identical to its rows of the 129-body result (bodies are independent; `chunks` explicit)."""
    case = 'bodies_' + name
    smpl = _smpl(dev, name)
    x = FC.inputs(case)
    v64, j64 = FC.oracle(case)
    v, j = _run(smpl, _on_device(dev, x), tag, BODY_CHUNKS)
    _against_float64(tag, '%s B=%d' % (name, FC.BODIES_B), v, j, v64, j64)
    for B in BODY_COUNTS:
        for sl, which in ((slice(0, B), 'first'), (slice(FC.BODIES_B - B, FC.BODIES_B), 'last')):
            vs, js = _run(smpl, _on_device(dev, x, sl), tag, BODY_CHUNKS)
            what = '%s, %s: the %s %d bodies alone against the same bodies in the batch of %d' % (name, tag, which, B, FC.BODIES_B)
            FC.assert_same_bits(what + ', vertices', vs, v[sl])
            FC.assert_same_bits(what + ', joints', js, j[sl], joints=True)


@pytest.mark.parametrize('tag', EDGE_MODES)
@pytest.mark.parametrize('B', [33, 65])
def test_chunk_edges(dev, B, tag):
    """chunks of one round, uneven last chunks, `chunks` above the round count, the automatic rule (-3): every vertex is produced by one
    wave whatever the split, so each result is bit-identical to chunks = 1; a tile that a chunk boundary drops is a NaN; twice each."""
    smpl = _smpl(dev, 'seed0')
    x = FC.inputs('chunks')
    d = _on_device(dev, x, slice(0, B))
    v64, j64 = FC.oracle('chunks')
    for joints in (True, False):
        v1, j1 = _run(smpl, d, tag, 1, joints=joints)
        _against_float64(tag, 'seed0 B=%d chunks=1' % B, v1, j1, v64[:B], j64[:B])
        for chunks in CHUNKS:
            for rep in range(2):
                v, j = _run(smpl, d, tag, chunks, joints=joints)
                what = 'seed0 B=%d, %s, joints %s: chunks=%d (run %d) against chunks=1' % (B, tag, joints, chunks, rep)
                FC.assert_same_bits(what + ', vertices', v, v1)
                FC.assert_same_bits(what + ', joints', j, j1, joints=True)


def test_input_edges(dev):
    """the extreme body, the identity pose with zero betas, axis-angle components up to 3.0 and an off-manifold body in one batch of 6"""
    smpl = _smpl(dev, 'seed0')
    d = _on_device(dev, FC.inputs('input_edges'))
    v64, j64 = FC.oracle('input_edges')
    m = FC.model('seed0')
    vt = torch.from_numpy(np.asarray(m['v_template'], np.float64))
    jt = torch.from_numpy(np.asarray(m['J_regressor'], np.float64)) @ vt
    for tag in MODES:
        v, j = _run(smpl, d, tag, 0)
        rep = _against_float64(tag, 'input edges B=6', v, j, v64, j64)
        print('input edges %-26s %s' % (tag, FC.describe(rep)))
        ident = FC.error_report(v[1:2], None, vt[None], None)
        assert ident['verts'] <= 1e-6, '%s: the identity body is not v_template: tile %d, %.3e m' % (tag, ident['tile'], ident['verts'])
        assert float((j[1, :24].double() - jt).abs().max()) <= 1e-6, '%s: joints 0..23 of the identity body are not J_regressor @ v_template' % tag


@pytest.mark.parametrize('case,name', [('var_chain_tree', 'chain_tree'), ('var_shallow_tree', 'shallow_tree'), ('chunks', 'seed0')])
def test_pose_kernel_alone(dev, case, name):
    """F and A read back from the guarded workspace in the layout smpl_pose_kernel writes -- F row = [1 | betas | (R_j - I), j = 1..23 | 0 x 6],
    A = [G_R | G_t - G_R J] per joint -- against the float64 restatement at 2e-6; the F entries that are copies bit for bit.  Depth 23, 3 and 8;
    B = 1 (a quarter wave), 9 (one pose block + 1 body) and 65."""
    smpl = _smpl(dev, name)
    x = FC.inputs(case)
    p = FC.packed(name)
    for B in (1, 9, 65):
        d = _on_device(dev, x, slice(0, B))
        v, j, ws = _run(smpl, d, 'fp32', 0, keep_ws=True)
        F, A = ws[:B * 224].view(B, 224), ws[B * 224:B * 512].view(B, 24, 3, 4)
        F64, A64, Gt = FC.numpy_pose_from_packed(p, x['betas'][:B].numpy(), x['R'][:B].numpy())
        what = '%s B=%d' % (name, B)
        assert torch.equal(F[:, 0], torch.ones(B)) and torch.equal(F[:, 1:11], x['betas'][:B]) and not F[:, 218:].any(), what + ': F columns 0..10 / 218..223'
        eF = np.abs(F[:, 11:218].double().numpy() - F64[:, 11:218])
        eA = np.abs(A.double().numpy() - A64)
        eJ = np.abs(j[:, :24].double().numpy() - Gt)
        assert not np.isnan(eF).any() and not np.isnan(eA).any()
        print('%s: F %.3e, A %.3e (joint %d), chain joints %.3e from float64' % (what, eF.max(), eA.max(), int(np.argmax(eA.max(axis=(0, 2, 3)))), eJ.max()))
        assert eF.max() <= 2e-6, '%s: pose feature of joint %d off by %.3e' % (what, 1 + int(np.argmax(eF.max(axis=0))) // 9, eF.max())
        assert eA.max() <= 2e-6, '%s: transform of joint %d (depth %d) off by %.3e' % (what, int(np.argmax(eA.max(axis=(0, 2, 3)))),
                                                                                   int(p['depth'][int(np.argmax(eA.max(axis=(0, 2, 3))))]), eA.max())
        assert eJ.max() <= 2e-6, '%s: chain joint %d off by %.3e' % (what, int(np.argmax(eJ.max(axis=(0, 2)))), eJ.max())


def test_a_virtual_vertex_row_beyond_the_joint_kernels_lds_is_refused(dev):
    """n_tiles = 264: smpl_joints_kernel would be launched with 4 x 48 x 96 x 4 = 73 728 bytes of dynamic LDS, above the 64 KB a kernel may
    ask for without raising its limit (which straps_smpl_fwd does not do for it).  Refused before the first launch: with real buffers, the
    outputs and the workspace keep their NaN pre-fill."""
    smpl = _smpl(dev, 'seed0')
    L = hipabi.lib()
    big = hipabi.SmplModelStruct()
    C.memmove(C.byref(big), C.byref(smpl._model_struct()), C.sizeof(big))
    big.n_tiles = 264
    B = 5
    d = _on_device(dev, FC.inputs('input_edges'), slice(0, B))
    z = Zone(dev)
    nbytes = L.straps_smpl_workspace_bytes(C.byref(big), B)
    assert nbytes == FC.workspace_bytes_formula(B, 264)
    ws, v, j = z.guarded((nbytes // 4,), name='workspace'), z.guarded((B, FC.NV, 3), name='verts'), z.guarded((B, FC.NJ_OUT, 3), name='joints')
    p = hipabi.ptr
    for tag in ('fp32', 'fp16x3_lbs/wide'):
        prec, kern = MODES[tag]
        rc = L.straps_smpl_fwd(C.byref(big), p(d['betas']), p(d['R']), p(v), p(j), p(ws), B, 0, PRECISIONS[prec] | KERNELS[kern], hipabi.stream_ptr())
        assert rc == EINVAL and b'n_tiles 264 exceeds 256' in L.straps_last_error(), (rc, L.straps_last_error())
    z.check()
    assert bool(torch.isnan(v).all()) and bool(torch.isnan(j).all()) and bool(torch.isnan(ws).all())
    v, j = _run(smpl, d, 'fp32', 0)                       # (the model itself, 224 tiles, is served)
    assert bool(torch.isfinite(v).all())
