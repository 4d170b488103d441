"""Test helper: the model variants, inputs, float64 / float32 oracles, the "where" error report and the packed-table restatement of
tests/test_gpu_smpl_fwd_edges.py (straps_smpl_fwd at its edges, behind redzones) and of the CPU checks of their conditioning in
tests/test_smpl_fwd_cases_cpu.py.  Everything is numpy / torch on the CPU, made from `synthetic_smpl_model(0)` and `det_uniform`; the
reference is oracle/straps_oracle.py (`smpl_forward`, `batch_rodrigues`) alone.

FWD_VARIANTS is the forward's own table: smpl_cases.MODEL_VARIANTS (which the backward suite iterates over, and whose measured floor
depends on it) stays as it is.
"""
import numpy as np
import torch

import straps_oracle as O
import smpl_cases as S
from detgen import det_uniform
from smpl_cases import NV, NJ_OUT, cpu_threads, real_magnitude_model          # (re-exported for the two test files)
from straps_amd.smpl import pack_smpl_model
from straps_amd.synthetic_smpl import synthetic_smpl_model

VPAD, TILES, KP = 6912, 216, 224
DENSE_NNZ = 600                  # 'all_dense_regressors': non-zeros of every one of the 45 regressor rows
SIGNED_ROW = 3                   # 'signed_regressor': the J_regressor_h36m row with alternating signs = output joint 73 + 3
EMPTY_ROW = 2                    # 'empty_regressor_row': the all-zero J_regressor_extra row = output joint 45 + 2
EMPTY_JOINT = 45 + EMPTY_ROW
SIGNED_JOINT = 73 + SIGNED_ROW
EXTREME_BETAS = (10.0, -8.0, 6.0, 4.0, -4.0, 3.0, 3.0, -3.0, 2.0, 2.0)      # the extreme body of test_smpl_split_precision_vs_oracle


def _all_dense(m):
    """every one of the 45 rows: DENSE_NNZ non-negative entries on a det_uniform-chosen vertex set, normalised to sum 1.  600 vertices
    touch all 24 bones, so every (joint, bone) pair exists: 45 x 24 = 1080 virtual vertices, the most non-negative rows can give."""
    for key, n, seed in (('J_regressor_extra', 9, 9101), ('J_regressor_cocoplus', 19, 9102), ('J_regressor_h36m', 17, 9103)):
        idx = np.argsort(det_uniform((n, NV), seed, 0.0, 1.0), axis=1, kind='stable')[:, :DENSE_NNZ]
        w = det_uniform((n, DENSE_NNZ), seed + 10, 0.2, 1.0).astype(np.float64)
        rows = np.zeros((n, NV))
        np.put_along_axis(rows, idx, w / w.sum(axis=1, keepdims=True), axis=1)
        m[key] = rows.astype(np.float32)
    return m


def _signed(m):
    """every second non-zero of one J_regressor_h36m row times -0.8: per bone the coefficients nearly cancel (|sum| < sum|.| / 4), the
    case pack_smpl_model splits by sign"""
    a = m['J_regressor_h36m'].astype(np.float64)
    nz = np.nonzero(a[SIGNED_ROW])[0]
    a[SIGNED_ROW, nz[1::2]] *= -0.8
    m['J_regressor_h36m'] = a.astype(np.float32)
    return m


def _empty_row(m):
    m['J_regressor_extra'][EMPTY_ROW] = 0.0
    return m


FWD_VARIANTS = dict(S.MODEL_VARIANTS)
FWD_VARIANTS['all_dense_regressors'] = lambda: _all_dense(synthetic_smpl_model(0))
FWD_VARIANTS['signed_regressor'] = lambda: _signed(synthetic_smpl_model(0))
FWD_VARIANTS['empty_regressor_row'] = lambda: _empty_row(synthetic_smpl_model(0))

# what pack_smpl_model gives for each variant (tests/test_smpl_fwd_cases_cpu.py asserts it): n_tiles, nvirt = vj_ptr[45], skin_k, max_depth
PACKED_FIGURES = {
    'seed0': (224, 254, 4, 8),
    'seed1': (232, 260, 4, 8),
    'real_magnitude': (224, 254, 4, 8),
    'rigid': (224, 111, 1, 8),
    'wide': (240, 668, 7, 8),
    'unskinned_joint': (224, 251, 4, 8),
    'chain_tree': (224, 254, 4, 23),
    'shallow_tree': (224, 254, 4, 3),
    'dense_regressors': (232, 273, 4, 8),
    'all_dense_regressors': (256, 1080, 4, 8),
    'signed_regressor': (232, 258, 4, 8),
    'empty_regressor_row': (224, 250, 4, 8),
}

_MODELS, _PACKED = {}, {}


def model(name):
    if name in S.MODEL_VARIANTS:
        return S.model(name)                       # (one copy per process, shared with the backward suite)
    if name not in _MODELS:
        _MODELS[name] = FWD_VARIANTS[name]()
    return _MODELS[name]


def packed(name):
    if name not in _PACKED:
        _PACKED[name] = pack_smpl_model(model(name))
    return _PACKED[name]


def sign_split_pairs(mdl):
    """number of (joint, bone) pairs of the 45 regressor rows whose coefficients cancel: the condition of pack_smpl_model's sign split,
    restated from the model alone"""
    R45 = np.concatenate([np.asarray(mdl[n], np.float64) for n in ('J_regressor_extra', 'J_regressor_cocoplus', 'J_regressor_h36m')], axis=0)
    W = np.asarray(mdl['weights'], np.float32).astype(np.float64)
    n = 0
    for j in range(45):
        cols = np.nonzero(R45[j])[0]
        if cols.size:
            Cj = R45[j, cols, None] * W[cols]
            live = np.any(Cj != 0, axis=0)
            n += int((np.abs(Cj.sum(0))[live] < 0.25 * np.abs(Cj).sum(0)[live]).sum())
    return n


# ---- the case matrix of the GPU file ----------------------------------------------------------------------------------------------------
# name -> dict(model, B, special).  special: 'big_beta' (body 0 = EXTREME_BETAS), 'identity' (body 1 at the identity pose with zero
# betas), 'pose3' (body 2 with axis-angle components up to 3.0), 'off_manifold' (body 3: R + 0.05 uniform; the forward is multilinear in R).
# Smaller batches of a test are the first / last bodies of its case.
VARIANT_B, BODIES_B, CHUNKS_B = 67, 129, 65
CASES = {}
for _v in FWD_VARIANTS:
    CASES['var_' + _v] = dict(model=_v, B=VARIANT_B, special=('big_beta', 'identity'))
CASES['bodies_seed0'] = dict(model='seed0', B=BODIES_B, special=('big_beta', 'identity'))
CASES['bodies_wide'] = dict(model='wide', B=BODIES_B, special=('big_beta', 'identity'))
CASES['chunks'] = dict(model='seed0', B=CHUNKS_B, special=('big_beta',))
CASES['input_edges'] = dict(model='seed0', B=6, special=('big_beta', 'identity', 'pose3', 'off_manifold'))
SEEDS = {}                                       # name -> seed, where the default missed the conditioning bar (chosen by the oracle alone)


def _seed(name):
    return SEEDS.get(name, 5000 + 16 * list(CASES).index(name))


_INPUTS = {}


def inputs(name):
    """-> dict(betas [B,10], R [B,24,3,3]) CPU fp32 tensors"""
    if name not in _INPUTS:
        c, s = CASES[name], _seed(name)
        B = c['B']
        betas = det_uniform((B, 10), s, -2.5, 2.5)
        aa = det_uniform((B, 72), s + 1, -0.8, 0.8)
        if 'big_beta' in c['special']:
            betas[0] = np.asarray(EXTREME_BETAS, np.float32)
        if 'identity' in c['special']:
            betas[1] = 0.0
            aa[1] = 0.0
        if 'pose3' in c['special']:
            aa[2] = det_uniform((72,), s + 2, -3.0, 3.0)
        R = O.batch_rodrigues(torch.from_numpy(aa).reshape(-1, 3)).view(B, 24, 3, 3)
        if 'identity' in c['special']:
            R[1] = torch.eye(3)                  # (batch_rodrigues of a zero vector is I + 1e-8 terms)
        if 'off_manifold' in c['special']:
            R[3] = R[3] + 0.05 * torch.from_numpy(det_uniform((24, 3, 3), s + 3))
        _INPUTS[name] = dict(betas=torch.from_numpy(betas), R=R.contiguous())
    return _INPUTS[name]


def oracle_forward(mdl, betas, R, dtype, block=32):
    """O.smpl_forward in `dtype`, `block` bodies at a time (bodies are independent) -> (verts [B,6890,3], joints [B,90,3]) float64"""
    vs, js = [], []
    for lo in range(0, betas.shape[0], block):
        v, j = O.smpl_forward(mdl, betas[lo:lo + block].to(dtype), rotmats=R[lo:lo + block].to(dtype), dtype=dtype)
        vs.append(v.double())
        js.append(j.double())
    return torch.cat(vs), torch.cat(js)


_ORACLE = {}


def oracle(name, dtype=torch.float64):
    """the oracle of a case in `dtype`, as float64 tensors; computed once per process and left unchanged"""
    key = (name, dtype)
    if key not in _ORACLE:
        x = inputs(name)
        before = torch.get_num_threads()
        torch.set_num_threads(cpu_threads())
        try:
            _ORACLE[key] = oracle_forward(model(CASES[name]['model']), x['betas'], x['R'], dtype)
        finally:
            torch.set_num_threads(before)
    return _ORACLE[key]


# ---- an error report that says where -----------------------------------------------------------------------------------------------------
JOINT_CLASSES = (('chain 0..23', 0, 24), ('picked 24..44', 24, 45), ('regressed extra 45..53', 45, 54),
                 ('regressed cocoplus 54..72', 54, 73), ('regressed h36m 73..89', 73, 90))


def _abs_err(got, ref):
    e = (torch.as_tensor(got).detach().cpu().double() - torch.as_tensor(ref).double()).abs()
    return torch.nan_to_num(e, nan=float('inf'), posinf=float('inf')).numpy()          # an element never written (NaN pre-fill) is the worst


def error_report(v, j, v64, j64):
    """-> dict(verts: worst |error| of the vertices, tiles [216]: per 32-vertex tile, tile: the worst tile, vertex / body of the worst
    element; joints: worst |error| of the joints, per_joint [90], classes {class name: (worst, joint)}, joint_class: the worst class).
    `j` may be None (a vertices-only call)."""
    ev = _abs_err(v, v64)
    pv = np.zeros(VPAD)
    pv[:NV] = ev.max(axis=(0, 2))
    tiles = pv.reshape(TILES, 32).max(axis=1)
    b, vid, _ = np.unravel_index(int(np.argmax(ev)), ev.shape)
    rep = dict(verts=float(ev.max()), tiles=tiles, tile=int(np.argmax(tiles)), vertex=int(vid), body=int(b), joints=0.0, per_joint=None, classes={},
               joint_class=None)
    if j is not None:
        ej = _abs_err(j, j64)
        pj = ej.max(axis=(0, 2))
        rep['joints'], rep['per_joint'] = float(pj.max()), pj
        for name, lo, hi in JOINT_CLASSES:
            rep['classes'][name] = (float(pj[lo:hi].max()), lo + int(np.argmax(pj[lo:hi])))
        rep['joint_class'] = max(rep['classes'], key=lambda k: rep['classes'][k][0])
        rep['joint_body'] = int(np.argmax(ej.max(axis=(1, 2))))
    return rep


def describe(rep):
    s = 'vertices %.3e m (tile %d, vertex %d, body %d)' % (rep['verts'], rep['tile'], rep['vertex'], rep['body'])
    if rep['per_joint'] is not None:
        w, jt = rep['classes'][rep['joint_class']]
        s += '; joints %.3e m (class %s, joint %d, body %d)' % (w, rep['joint_class'], jt, rep['joint_body'])
    return s


def assert_close(tag, v, j, v64, j64, bar):
    """both outputs within `bar` of the reference; the message names every tile and every joint class above the bar"""
    rep = error_report(v, j, v64, j64)
    if rep['verts'] <= bar and rep['joints'] <= bar:
        return rep
    bad_t = np.nonzero(~(rep['tiles'] <= bar))[0]
    msg = '%s: above %.1e m: %s' % (tag, bar, describe(rep))
    if bad_t.size:
        msg += '; tiles above the bar: %s%s' % (', '.join('%d (%.2e)' % (t, rep['tiles'][t]) for t in bad_t[:12]), ' ...' if bad_t.size > 12 else '')
    bad_c = [(n, jt, w) for n, (w, jt) in rep['classes'].items() if not w <= bar]
    if bad_c:
        msg += '; joint classes above the bar: ' + ', '.join('%s (joint %d: %.2e)' % c for c in bad_c)
    raise AssertionError(msg)


def assert_same_bits(tag, a, b, joints=False):
    """torch.equal, with a message that names the first tile (or joint) that differs"""
    if a is None and b is None:
        return
    a, b = a.detach().cpu(), b.detach().cpu()
    if torch.equal(a, b):
        return
    # (NaN != NaN: a NaN on both sides counts as a difference too -- an output of these tests never holds one)
    diff = (a != b).any(dim=2)
    bodies, cols = diff.any(dim=1).nonzero().flatten(), diff.any(dim=0).nonzero().flatten()
    if joints:
        where = 'joints %s' % cols[:12].tolist()
    else:
        where = 'tiles %s' % sorted(set((cols // 32).tolist()))[:12]
    worst = float(torch.nan_to_num((a.double() - b.double()).abs(), nan=float('inf')).max())
    raise AssertionError('%s: not bit-identical in %s of bodies %s (%d elements, largest difference %.3e)'
                         % (tag, where, bodies[:12].tolist(), int((a != b).sum()), worst))


# ---- the forward restated from the PACKED tables alone (float64) -------------------------------------------------------------------------
def unpack_blend_frag(p):
    """blend_frag [tile][coord][g 28][h 2][i 32][e 4] (include/straps_hip.h) -> D [224][32 * n_tiles][3], float64"""
    nt = p['n_tiles']
    f = np.asarray(p['blend_frag'], np.float64).reshape(nt, 3, 28, 2, 32, 4)
    return f.transpose(2, 3, 5, 0, 4, 1).reshape(KP, nt * 32, 3)


def unpack_blend_frag_h(p):
    """blend_frag_h [tile][kstep 14][coord][hi|lo][hh 2][i 32][j 8] -> (hi + lo) / S_D as D [224][32 * n_tiles][3], float64"""
    nt = p['n_tiles']
    f = np.asarray(p['blend_frag_h']).astype(np.float64).reshape(nt, 14, 3, 2, 2, 32, 8)
    s_d = 1.0 / (float(p['blend_h_unscale']) * 64.0)
    return (f[:, :, :, 0] + f[:, :, :, 1]).transpose(1, 3, 5, 0, 4, 2).reshape(KP, nt * 32, 3) / s_d


def unpack_skin_sparse(p):
    """skin_w / skin_j [32 * n_tiles][skin_k] -> dense W [32 * n_tiles][24], float64"""
    n, k = p['skin_w'].shape
    W = np.zeros((n, 24))
    np.add.at(W, (np.repeat(np.arange(n), k), np.asarray(p['skin_j']).reshape(-1)), np.asarray(p['skin_w'], np.float64).reshape(-1))
    return W


def unpack_skin_frag_p(p):
    """skin_frag_p [tile][kstep 5][hh 2][i 32][j 8] -> the 80 packed columns P [32 * n_tiles][80] = [hi 24 | hi 24 | lo 24 | 0 x 8], float64"""
    nt = p['n_tiles']
    f = np.asarray(p['skin_frag_p']).astype(np.float64).reshape(nt, 5, 2, 32, 8)
    return f.transpose(0, 3, 1, 2, 4).reshape(nt * 32, 80)


def unpack_skin_split(p):
    """the dense weights rebuilt from skin_frag_p as (hi + lo) * 2^-14"""
    P = unpack_skin_frag_p(p)
    return (P[:, :24] + P[:, 48:72]) * 2.0 ** -14


def numpy_pose_from_packed(p, betas, R):
    """what smpl_pose_kernel writes, float64: F [B][224] = [1 | betas | (R_j - I), j = 1..23 | 0 x 6], A [B][24][3][4] = [G_R | G_t - G_R J],
    and the chain joints G_t [B][24][3] -- from j_template, j_shapedirs and parents"""
    betas, R = np.asarray(betas, np.float64), np.asarray(R, np.float64)
    B = betas.shape[0]
    F = np.zeros((B, KP))
    F[:, 0] = 1.0
    F[:, 1:11] = betas
    F[:, 11:218] = (R[:, 1:] - np.eye(3)).reshape(B, 207)
    J = np.asarray(p['j_template'], np.float64)[None] + np.einsum('jcl,bl->bjc', np.asarray(p['j_shapedirs'], np.float64), betas)
    parents = [int(x) for x in p['parents']]
    GR, Gt = np.zeros((B, 24, 3, 3)), np.zeros((B, 24, 3))
    GR[:, 0], Gt[:, 0] = R[:, 0], J[:, 0]
    for j in range(1, 24):
        q = parents[j]
        GR[:, j] = GR[:, q] @ R[:, j]
        Gt[:, j] = np.einsum('brc,bc->br', GR[:, q], J[:, j] - J[:, q]) + Gt[:, q]
    A = np.concatenate([GR, (Gt - np.einsum('bjrc,bjc->bjr', GR, J))[..., None]], axis=3)
    return F, A, Gt


def numpy_forward_from_packed(p, betas, R, tables='fp32', with_bound=False):
    """the forward restated in float64 from the packed tables only (not from the model dict) -> (verts [B,6890,3], joints [B,90,3]).
    tables: 'fp32' = blend_frag + skin_w / skin_j; 'split' = blend_frag_h as (hi + lo) / S_D + skin_frag_p as (hi + lo) * 2^-14.
    with_bound: also the bound on what the two-term fp16 splits can cost, derived from the case: every entry x of a split table is
    hi + lo + e with |e| <= 2^-22 |x| (11 bits each) while lo is a normal fp16 number and <= 2^-25 / scale below that, so
        |d v_posed| <= 2^-22 sum_k |F_k| |D_k| + 2^-25 / S_D  ||F||_1,      |d T| <= 2^-22 sum_j W_j |A_j| + 2^-39 sum_{j: W_j != 0} |A_j|
    per element (the product of the two is left out: 1e-13), carried through the skinning and, for the regressed joints, through the sum over their virtual vertices."""
    D = unpack_blend_frag(p) if tables == 'fp32' else unpack_blend_frag_h(p)
    W = unpack_skin_sparse(p) if tables == 'fp32' else unpack_skin_split(p)
    F, A, Gt = numpy_pose_from_packed(p, betas, R)
    B = F.shape[0]
    vposed = np.einsum('bk,kvc->bvc', F, D)
    T = np.einsum('vj,bjrc->bvrc', W, A)
    out = np.einsum('bvrc,bvc->bvr', T[..., :3], vposed) + T[..., 3]
    vj_ptr = np.asarray(p['vj_ptr'])
    pick = np.asarray(p['pick_ids'])

    def gather(o):
        joints = np.zeros((B, NJ_OUT, 3))
        joints[:, 24:45] = o[:, pick]
        for j in range(45):
            joints[:, 45 + j] = o[:, VPAD + vj_ptr[j]:VPAD + vj_ptr[j + 1]].sum(axis=1)
        return joints
    joints = gather(out)
    joints[:, :24] = Gt
    if not with_bound:
        return out[:, :NV], joints
    s_d = 1.0 / (float(p['blend_h_unscale']) * 64.0)
    e_vp = 2.0 ** -22 * np.einsum('bk,kvc->bvc', np.abs(F), np.abs(D)) + (2.0 ** -25 / s_d) * np.abs(F).sum(1)[:, None, None]
    absT = np.einsum('vj,bjrc->bvrc', np.abs(W), np.abs(A))
    absT0 = np.einsum('vj,bjrc->bvrc', (W != 0).astype(np.float64), np.abs(A))          # (the absolute 2^-25 / 2^14 of a weight's low half)
    avp = np.abs(vposed)
    e_out = np.einsum('bvrc,bvc->bvr', absT[..., :3], e_vp) \
        + 2.0 ** -22 * (np.einsum('bvrc,bvc->bvr', absT[..., :3], avp) + absT[..., 3]) \
        + 2.0 ** -39 * (np.einsum('bvrc,bvc->bvr', absT0[..., :3], avp) + absT0[..., 3])
    return out[:, :NV], joints, float(max(e_out[:, :NV].max(), gather(e_out).max()))


def workspace_bytes_formula(batch, n_tiles):
    """include/straps_hip.h, straps_smpl_workspace_bytes: F [B][224], A [B][288], virtual-vertex rows [B][(n_tiles - 216) * 96]"""
    return batch * (224 + 288 + (n_tiles - 216) * 96) * 4
