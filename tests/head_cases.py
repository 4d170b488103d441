"""Test helper: the case tables and float64 references of tests/test_gpu_ief_edges.py, tests/test_gpu_pose_edges.py and tests/test_gpu_optim_edges.py
-- the kernels between the encoder and SMPL (csrc/ief.hip, csrc/pose.hip, rot6d_bwd_kernel of csrc/backward.hip) and the ones that close a training
step (adam_kernel, mse_sum_kernel, mse_grad_kernel, project_targets_kernel of csrc/train.hip).  No GPU and no call of the library here:
tests/test_head_cases_cpu.py holds the tables to the edges they claim and the references to independent evaluations (torch.matmul, autograd of the
oracle, torch.optim.Adam, F.mse_loss).

The launch rules are restated as plain Python next to the tables; all of them are file-local in the library (nothing exported confirms them without
a launch), so a change of one has to be repeated here by hand:

    linear_kernel        G = K >> 3 groups of 8, dealt round-robin to LW = 8 waves (`for g = wave; g < G; g += LW`, unrolled by 4)       csrc/ief.hip
    gemm_multi_kernel    G = (K + 7) >> 3, a wave takes groups g and g + LW per trip of `for g = wave; g < G; g += 2 * LW`, k < K masked  csrc/ief.hip
    ief_pack_kernel      min(ceil(total / 256), 2048) workgroups of 256, grid-stride                                                    csrc/ief.hip
    broadcast_rows, rot6d, rot6d_bwd, rodrigues, ortho_project, persp_project, project_targets: ceil(n / 256) workgroups, one element per thread
    ortho_project_bwd    one workgroup of 256 per body, thread t sums n = t, t + 256, ...; 64-lane shuffle tree; four waves through LDS   csrc/pose.hip
    adam_kernel, mse_grad_kernel   capped_grid: min(ceil(n / 256), 4096) workgroups, grid-stride                                        csrc/train.hip
    mse_sum_kernel       256 workgroups of 256 always: a stride of 65536 elements                                                       csrc/train.hip
"""
from collections import namedtuple

import numpy as np
import torch

import straps_oracle as O
from detgen import det_uniform

U = 2.0 ** -24                     # unit roundoff of fp32
LW = 8


def f32(v):
    """a Python scalar as the fp32 value a `float` argument of the library carries"""
    return float(np.float32(v))


PERIOD = (1 << 19) + 17


def det(shape, seed, lo=-1.0, hi=1.0):
    """det_uniform data as a CPU tensor; beyond 2^19 elements one det_uniform block repeated (as tests/test_gpu_norm_pool_edges.py does)"""
    shape = tuple(int(s) for s in shape)
    n = 1
    for d in shape:
        n *= d
    if n <= PERIOD:
        return torch.from_numpy(det_uniform(shape, seed, lo, hi).copy())
    blk = torch.from_numpy(det_uniform((PERIOD,), seed, lo, hi))
    return blk.repeat(-(-n // PERIOD))[:n].view(shape).contiguous()


def tracer(shape, seed):
    """integers in {-2, ..., 2} as fp32: every product and partial sum of a dot product over K <= 2048 of them is an integer below 2^24, so the
    fp32 result is the integer result whatever the summation order"""
    return det(shape, seed, -2.49, 2.49).round() + 0.0


def ordv(t):
    """fp32 -> integers in the order of the values (both zeros map to 0): the distance of two values in ulps is the difference"""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def check_ratio(family, got, want, bound):
    """per element |got - want| <= bound; prints `RATIO <family> <worst error / bound>`; -> that ratio"""
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), '%s: not finite (an element nobody wrote, or a read past an operand)' % family
    err = (got.double() - want.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('RATIO %s %.4f' % (family, worst))
    k = int(ratio.argmax()) if ratio.numel() else 0
    assert worst <= 1.0, '%s: error %.3e against a bound of %.3e at flat index %d' % (family, float(err.flatten()[k]), float(bound.flatten()[k]), k)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. straps_linear_fwd

# ldw / ldx: kdim + the pad; ldo: the row stride of out and addend; addend: 0 none | 1 a buffer (run twice: separate, and `out` itself)
LinCase = namedtuple('LinCase', 'm n k wpad xpad ldo bias relu addend')
LINEAR = [
    LinCase(1, 1, 8, 0, 0, 1, 1, 0, 0),
    LinCase(1, 157, 8, 4, 4, 160, 1, 1, 1),
    LinCase(31, 32, 56, 0, 4, 32, 0, 0, 1),
    LinCase(32, 33, 64, 4, 0, 33, 1, 1, 0),
    LinCase(33, 33, 72, 4, 4, 33, 1, 0, 1),
    LinCase(70, 96, 160, 0, 0, 96, 1, 1, 0),
    LinCase(33, 157, 160, 0, 0, 160, 1, 0, 1),          # fc3 of the regressor: the in-place estimate update
    LinCase(1, 157, 520, 0, 4, 157, 0, 1, 1),
    LinCase(70, 157, 2048, 0, 0, 160, 1, 0, 0),
    LinCase(31, 1, 2048, 4, 0, 1, 0, 1, 1),
    LinCase(32, 32, 64, 0, 0, 32, 0, 0, 0),
    LinCase(33, 96, 520, 4, 4, 96, 1, 1, 1),
    LinCase(70, 33, 72, 0, 0, 33, 0, 1, 0),
    LinCase(1, 32, 56, 0, 0, 32, 1, 0, 0),
    LinCase(31, 157, 72, 0, 4, 160, 0, 0, 1),
    LinCase(32, 1, 160, 4, 0, 1, 1, 1, 1),
    LinCase(33, 1, 8, 0, 0, 1, 0, 1, 0),
    LinCase(70, 1, 520, 0, 0, 1, 1, 0, 1),
    LinCase(1, 96, 2048, 0, 0, 96, 0, 0, 0),
    LinCase(32, 157, 64, 0, 0, 157, 1, 1, 1),
]
LIN_M, LIN_N, LIN_K = (1, 31, 32, 33, 70), (1, 32, 33, 96, 157), (8, 56, 64, 72, 160, 520, 2048)


def linear_reach(k):
    """-> (idle waves, trips of the busiest wave, the unrolled-by-4 body runs, a remainder trip runs) of linear_kernel's K loop"""
    G = k >> 3
    trips = [len(range(w, G, LW)) for w in range(LW)]
    return (sum(1 for t in trips if t == 0), max(trips), any(t >= 4 for t in trips), any(t % 4 for t in trips))


def linear_data(c, kind, seed=100):
    """-> x [m][ldx], w [n_pad][ldw], bias [n] | None, addend [m][ldo] | None.  The columns k >= kdim of x and w hold NaN: they must never be read.
    w has exactly ceil(n / 32) * 32 rows, rows >= n zero (the header's contract)."""
    gen = tracer if kind == 'tracer' else det
    npad = (c.n + 31) // 32 * 32
    x = torch.full((c.m, c.k + c.xpad), float('nan'))
    x[:, :c.k] = gen((c.m, c.k), seed + 1)
    w = torch.full((npad, c.k + c.wpad), float('nan'))
    w[:, :c.k] = 0.0
    w[:c.n, :c.k] = gen((c.n, c.k), seed + 2)
    bias = gen((c.n,), seed + 3) if c.bias else None
    addend = None
    if c.addend:
        addend = torch.full((c.m, c.ldo), float('nan'))
        addend[:, :c.n] = gen((c.m, c.n), seed + 4)
    if kind == 'tracer' and c.relu:
        # an exact zero in the pre-activation by construction (still integers): element (0, 0) is cancelled by the addend, else by the bias, else
        # row 0 of x is zero; negatives occur by themselves (tests/test_head_cases_cpu.py asserts both)
        pre00 = float((x[0, :c.k].double() * w[0, :c.k].double()).sum()) + (float(bias[0]) if c.bias else 0.0)
        if c.addend:
            addend[0, 0] = -pre00
        elif c.bias:
            bias[0] -= pre00
        else:
            assert c.m > 1
            x[0, :c.k] = 0.0
    return x, w, bias, addend


def linear_reference(c, x, w, bias, addend):
    """float64 -> (want [m][n] after the activation, the pre-activation, the per-element bound of the real-data check:
    (K + 16) 2^-24 sum_k |x w| + 2^-23 (|bias| + |addend| + |want|): the worst-case forward error of an fp32 dot product in any order plus the
    epilogue's additions; ReLU does not enlarge a difference)"""
    X, W = x[:, :c.k].double(), w[:c.n, :c.k].double()
    pre = (X[:, None, :] * W[None, :, :]).sum(-1)
    mag = (X[:, None, :] * W[None, :, :]).abs().sum(-1)
    extra = torch.zeros_like(pre)
    if bias is not None:
        pre = pre + bias.double()[None, :]
        extra = extra + bias.double().abs()[None, :]
    if addend is not None:
        pre = pre + addend[:, :c.n].double()
        extra = extra + addend[:, :c.n].double().abs()
    bound = (c.k + 16) * U * mag + 2 * U * (extra + pre.abs())
    return (pre.clamp_min(0) if c.relu else pre), pre, bound


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. straps_gemm_multi

# a: 'T' (sam = 1, sak = ld: A stored [k][m]) | 'N' (sam = ld, sak = 1: A stored [m][k]) | 'one' (sam = sak = 0, a single 1.0f; m = 1)
# b: 'nk' (sbk = 1, sbn = ld: B stored [n][k]) | 'kn' (sbk = ld, sbn = 1: B stored [k][n]);  cpad: ldc = n + cpad
# acc: accumulate; c2: 0 none | 1 accumulate2 = 0 | 2 accumulate2 = 1; addend (ldadd = n + 3, never ldc); mask
GemmCase = namedtuple('GemmCase', 'm n k a b cpad acc c2 addend mask')
GEMM = [
    GemmCase(1, 1, 1, 'N', 'kn', 0, 0, 0, 0, 0),
    GemmCase(31, 33, 3, 'T', 'nk', 2, 0, 1, 0, 0),
    GemmCase(32, 32, 4, 'N', 'nk', 0, 1, 0, 1, 0),
    GemmCase(33, 31, 5, 'T', 'kn', 0, 0, 2, 0, 1),
    GemmCase(65, 1, 8, 'N', 'kn', 1, 1, 1, 1, 1),
    GemmCase(1, 65, 9, 'one', 'kn', 0, 0, 0, 0, 0),              # a bias gradient: column sums
    GemmCase(33, 33, 64, 'T', 'kn', 0, 0, 0, 0, 0),
    GemmCase(31, 65, 65, 'N', 'nk', 5, 1, 2, 1, 1),
    GemmCase(65, 65, 128, 'T', 'nk', 0, 0, 0, 0, 0),
    GemmCase(32, 33, 129, 'N', 'kn', 0, 0, 1, 0, 1),
    GemmCase(1, 31, 136, 'one', 'nk', 1, 1, 0, 0, 0),
    GemmCase(65, 65, 300, 'T', 'kn', 7, 0, 2, 1, 1),
    GemmCase(33, 1, 300, 'N', 'nk', 0, 0, 0, 1, 0),
    GemmCase(1, 32, 3, 'one', 'kn', 0, 0, 0, 0, 0),
]
GEMM_K, GEMM_MN = (1, 3, 4, 5, 8, 9, 64, 65, 128, 129, 136, 300), (1, 31, 32, 33, 65)
GEMM_MULTI = (0, 1, 3, 5, 7, 9, 10, 11)        # the 8-problem launch: problem 0 is 1x1x1, problem 7 is 65x65x300


def gemm_reach(k):
    """-> (trips of the outer loop for the busiest wave, a wave whose second group g + LW lies beyond G, a group cut inside a half-group
    (K % 4 != 0), a group cut between its half-groups or with an all-masked half (0 < K % 8 <= 4), idle waves)"""
    G = (k + 7) >> 3
    trips = [len(range(w, G, 2 * LW)) for w in range(LW)]
    beyond = any(g + LW >= G for w in range(LW) for g in range(w, G, 2 * LW))
    return (max(trips), beyond, k % 4 != 0, 0 < k % 8 <= 4, sum(1 for t in trips if t == 0))


def gemm_data(c, kind, seed=200):
    """-> dict: A [m][k], B [k][n] (logical, fp32), a / b as stored with their strides, old c / c2 [m][ldc] (NaN where nothing accumulates: it must be
    overwritten, not read), addend [m][n + 3], mask [m][n]"""
    gen = tracer if kind == 'tracer' else det
    d = dict(ldc=c.n + c.cpad, ldadd=c.n + 3)
    B = gen((c.k, c.n), seed + 2)
    if c.a == 'one':
        assert c.m == 1
        A = torch.ones(1, c.k)
        d.update(a=torch.ones(1), sam=0, sak=0)
    else:
        A = gen((c.m, c.k), seed + 1)
        if c.a == 'T':
            d.update(a=A.t().contiguous(), sam=1, sak=c.m)
        else:
            d.update(a=A.contiguous(), sam=c.k, sak=1)
    if c.b == 'nk':
        d.update(b=B.t().contiguous(), sbk=1, sbn=c.k)
    else:
        d.update(b=B.contiguous(), sbk=c.n, sbn=1)
    d.update(A=A, B=B)
    d['c_old'] = gen((c.m, d['ldc']), seed + 3) if c.acc else None
    d['c2_old'] = gen((c.m, d['ldc']), seed + 4) if c.c2 == 2 else None
    d['addend'] = gen((c.m, d['ldadd']), seed + 5) if c.addend else None
    mask = None
    if c.mask:
        mask = det((c.m, c.n), seed + 6).flatten()          # entries > 0 and negative; 0.0, -0.0 and NaN placed
        mask[0::7], mask[1::7], mask[2::7] = 0.0, -0.0, float('nan')
        if mask.numel() > 3:
            mask[3] = 2.0 ** -140                           # the smallest kind of "> 0" (a denormal is not flushed by a compare)
        mask = mask.view(c.m, c.n)
    d['mask'] = mask
    return d


def gemm_reference(c, d):
    """float64 -> (v [m][n] after addend and mask, want of c, want of c2 | None, the bound of c, the bound of c2)
    bound: (K + 24) 2^-24 sum_k |a b| + 2^-23 (|addend| + |old| + |want|)"""
    A, B = d['A'].double(), d['B'].double()
    v = (A[:, :, None] * B[None, :, :]).sum(1)
    mag = (A[:, :, None] * B[None, :, :]).abs().sum(1)
    extra = torch.zeros_like(v)
    if d['addend'] is not None:
        v = v + d['addend'][:, :c.n].double()
        extra = extra + d['addend'][:, :c.n].double().abs()
    if d['mask'] is not None:
        keep = d['mask'] > 0
        v, mag, extra = torch.where(keep, v, torch.zeros_like(v)), torch.where(keep, mag, torch.zeros_like(v)), torch.where(keep, extra, torch.zeros_like(v))
    want = v + d['c_old'][:, :c.n].double() if c.acc else v
    e1 = extra + (d['c_old'][:, :c.n].double().abs() if c.acc else 0)
    want2 = e2 = None
    if c.c2:
        want2 = v + d['c2_old'][:, :c.n].double() if c.c2 == 2 else v
        e2 = extra + (d['c2_old'][:, :c.n].double().abs() if c.c2 == 2 else 0)
    bnd = lambda w_, e_: (c.k + 24) * U * mag + 2 * U * (e_ + w_.abs())
    return v, want, want2, bnd(want, e1), (bnd(want2, e2) if c.c2 else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. straps_ief_pack, straps_broadcast_rows

# (f, p, h1, h2, ld_e).  The fifth case is the fourth with h2 = 64: straps_linear_fwd needs kdim % 8 == 0 and ldw % 4 == 0, which the fourth's
# h2 = 65 cannot give, so the cross-check of the two contracts (the packed w3 as straps_linear_fwd's weight) runs on the second and the fifth.
PACK = [(8, 5, 3, 7, 8), (512, 157, 512, 512, 160), (1024, 157, 512, 512, 160), (40, 157, 33, 65, 157), (40, 157, 33, 64, 157)]
PACK_LINEAR = (1, 4)
BROADCAST = [(157, 160, 1), (157, 160, 4), (157, 157, 5), (1, 3, 85), (1, 3, 86)]          # cols, ld_dst, m


def pack_total(f, p, h1, h2, ld_e):
    return h1 * f + h1 * ld_e + (p + 31) // 32 * 32 * h2


def pack_reach(f, p, h1, h2, ld_e):
    """-> (workgroups, the stride loop takes a second trip, w1e has padding columns)"""
    total = pack_total(f, p, h1, h2, ld_e)
    blocks = min((total + 255) // 256, 2048)
    return blocks, total > blocks * 256, ld_e > p


def pack_reference(fc1, fc3, f, p, h1, h2, ld_e):
    w1f = fc1[:, :f].contiguous()
    w1e = torch.zeros(h1, ld_e)
    w1e[:, :p] = fc1[:, f:]
    w3 = torch.zeros((p + 31) // 32 * 32, h2)
    w3[:p] = fc3
    return w1f, w1e, w3


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. straps_rot6d_fwd / straps_rot6d_bwd

# (rows, per_row, ld, ldd).  A stride of 157 or 160 is that of an estimate buffer [rows][stride]: the pose columns start 3 floats into every
# row (a [rows][157] buffer in fit.py, [rows][160] in train_step.py), for x6 and dx6 alike; every other stride starts at column 0.
ROT6D = [(1, 1, 6, 6), (255, 1, 6, 8), (256, 1, 8, 6), (257, 1, 6, 6), (1, 24, 144, 144), (11, 24, 157, 144), (11, 24, 160, 160), (3, 24, 157, 157)]
ROT6D_SEEDS = (15, 15, 15, 15, 15, 15, 15, 17)          # per case; the filter below replaces at most 5 % of a case's rotations with them


def rot6d_offset(ld):
    return 3 if ld in (157, 160) else 0


def rot6d_well_conditioned(rows, per_row, seed):
    """-> (x [rows * per_row][6] fp32, the fraction of rotations the filter replaced).  det_uniform in [-1.5, 1.5]; a rotation with |a1| < 0.25 or
    |a2 - (b1.a2) b1| < 0.25 is replaced by the rotation before it (the first by the first one kept): the launch shape stays"""
    x = det((rows * per_row, 6), seed, -1.5, 1.5)
    xd = x.double().view(-1, 3, 2)
    a1, a2 = xd[:, :, 0], xd[:, :, 1]
    n1 = a1.norm(dim=1)
    b1 = a1 / n1.clamp_min(1e-300)[:, None]
    u = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    ok = (n1 >= 0.25) & (u.norm(dim=1) >= 0.25)
    assert bool(ok.any())
    first = int(ok.nonzero()[0])
    for i in range(x.shape[0]):
        if not ok[i]:
            x[i] = x[i - 1] if i > 0 else x[first]
    return x, 1.0 - float(ok.double().mean())


def rot6d_formula(x, g=None, dtype=torch.float64):
    """the Gram-Schmidt of utils/rigid_transform_utils.py:27-41 with its clamps, and its derivative by hand, in `dtype`: x [n][6] -> R [n][3][3]
    (columns b1, b2, b3) and, with g = dL/dR, dL/dx [n][6].  In a clamped branch the derivative of the normalisation is g / 1e-12 without the
    projection term, which is what autograd of clamp_min gives.  (An independent restatement: the GPU tests compare with autograd of the oracle;
    tests/test_head_cases_cpu.py holds this to autograd, and evaluates it in fp32 to measure what an honest fp32 evaluation reaches.)"""
    x = x.to(dtype).view(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    eps = torch.tensor(1e-12, dtype=dtype)
    n1r = (a1 * a1).sum(1, keepdim=True).sqrt()
    n1 = torch.maximum(n1r, eps)
    b1 = a1 / n1
    d = (b1 * a2).sum(1, keepdim=True)
    u = a2 - d * b1
    n2r = (u * u).sum(1, keepdim=True).sqrt()
    n2 = torch.maximum(n2r, eps)
    b2 = u / n2
    b3 = torch.linalg.cross(b1, b2, dim=1)
    R = torch.stack((b1, b2, b3), dim=-1)
    if g is None:
        return R
    g = g.to(dtype).view(-1, 3, 3)
    gb1, gb2, gb3 = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    gb1 = gb1 + torch.linalg.cross(b2, gb3, dim=1)
    gb2 = gb2 + torch.linalg.cross(gb3, b1, dim=1)
    gu = torch.where(n2r > eps, (gb2 - b2 * (b2 * gb2).sum(1, keepdim=True)) / n2, gb2 / n2)
    gd = -(gu * b1).sum(1, keepdim=True)
    ga2 = gu + gd * b1
    gb1 = gb1 + (-d * gu + gd * a2)
    ga1 = torch.where(n1r > eps, (gb1 - b1 * (b1 * gb1).sum(1, keepdim=True)) / n1, gb1 / n1)
    return R, torch.stack((ga1, ga2), dim=-1).reshape(-1, 6)


def rot6d_autograd(x, g):
    """float64 autograd of the oracle: x [n][6] fp32, g [n][3][3] fp32 -> (R, dL/dx) in float64"""
    xo = x.double().clone().requires_grad_()
    R = O.rot6d_to_rotmat(xo)
    R.backward(g.double().view(-1, 3, 3))
    return R.detach(), xo.grad.detach()


def _x6(a1, a2):
    return [a1[0], a2[0], a1[1], a2[1], a1[2], a2[2]]


def rot6d_degenerate():
    """-> list of (kind, x6 [6], exact) for the degenerate test.  `exact` rows are built on the coordinate axes with dyadic entries: b1, b2, d and
    u are then exact in fp32 and in float64 alike, every intermediate of the backward with a dyadic dL/dR is exact up to the final division, and
    the clamped branch is reached in both precisions.  The generic rows (`exact` False) are ill-conditioned: u is rounding noise, different noise
    in fp32 and float64; only what the issue asks of them is checked.  `exact` 'bwd': the forward is compared to 2e-6 (the fp32 constant 1e-12f is
    not the double 1e-12), the backward per entry like the exact rows."""
    rows = [
        ('a1=0', _x6((0, 0, 0), (0, 2, 0)), True), ('a1=0', _x6((0, 0, 0), (0, 0, -0.5)), True), ('a1=0', _x6((0, 0, 0), (0.3, -1.1, 0.7)), False),
        ('a2=0', _x6((0.5, 0, 0), (0, 0, 0)), True), ('a2=0', _x6((0, 0, -4), (0, 0, 0)), True), ('a2=0', _x6((0.3, -1.1, 0.7), (0, 0, 0)), False),
        ('collinear', _x6((0.5, 0, 0), (1, 0, 0)), True), ('collinear', _x6((0, -2, 0), (0, -4, 0)), True), ('collinear', _x6((0, 0, 1), (0, 0, 2)), True),
        ('collinear', _x6((0.3, -1.1, 0.7), (0.6, -2.2, 1.4)), False),
        ('near', _x6((0.3, -1.1, 0.7), (0.3 + 1e-7, -1.1, 0.7)), False), ('near', _x6((1.0, 0.5, -0.25), (1.0, 0.5, -0.25 + 1e-7)), False),
        # 0 < |u| <= 1e-12 and 0 < |a1| <= 1e-12: the clamped quotient is NOT zero (b2 = u / 1e-12 = (0, 1/2, 0) or (0, -1/4, 0)), so the projection term that the
        # clamped branch must leave out would change the gradient by a quarter -- with u = 0 exactly it vanishes and either branch gives the same
        ('tiny-u', _x6((1, 0, 0), (1, 5e-13, 0)), 'bwd'), ('tiny-u', _x6((0, 0, -2), (0, -2.5e-13, -4)), 'bwd'),
        ('tiny-a1', _x6((5e-13, 0, 0), (0, 2, 0)), 'bwd'), ('tiny-a1', _x6((0, -2.5e-13, 0), (0, 0, 0.5)), 'bwd'),
    ]
    return [(k, torch.tensor(v, dtype=torch.float32), e) for k, v, e in rows]


def dyadic(shape, seed):
    """multiples of 1/8 in [-1, 1]"""
    return (det(shape, seed, -8.49, 8.49).round() + 0.0) / 8


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. straps_rodrigues_fwd

RODRIGUES_N = (1, 255, 256, 257)
_S3 = 1.0 / 3.0 ** 0.5
_PI = float(np.pi)


def rodrigues_specials():
    """-> list of (family, row).  'zero' is the marked row inside the excluded neighbourhood (see rodrigues_excluded): r = 0 gives d = 0 and the
    identity exactly, in the kernel and in the reference alike."""
    rows = [('zero', (0.0, 0.0, 0.0))]
    for a in (1e-4, 1e-3):
        rows += [('small', (a, 0, 0)), ('small', (0, -a, 0)), ('small', (0, 0, a))]
    for ang in (_PI, 2 * _PI):
        rows += [('pi', (ang, 0, 0)), ('pi', (0, 0, -ang)), ('pi', (ang * _S3, ang * _S3, ang * _S3)), ('pi', (-ang * _S3, -ang * _S3, -ang * _S3))]
    rows += [('r10', (10.0, 0, 0)), ('r10', (0, -10.0, 0)), ('r10', (10 * _S3, 10 * _S3, 10 * _S3)), ('r10', (-10 * _S3, 10 * _S3, -10 * _S3))]
    rows += [('r50', (50.0, 0, 0)), ('r50', (0, 0, -50.0)), ('r50', (50 * _S3, 50 * _S3, 50 * _S3)), ('r50', (-50 * _S3, -50 * _S3, 50 * _S3))]
    return rows


def rodrigues_rows(n):
    """-> (aa [n][3] fp32, families: list of n names).  det_uniform in [-3, 3] ('random'); the special rows overwrite the END of the table (the last
    lanes of the last workgroup), the zero row index 0; n = 1 is one random row"""
    aa = det((n, 3), 9, -3, 3)
    fam = ['random'] * n
    sp = rodrigues_specials()
    if n == 1:
        return aa, fam
    aa[0], fam[0] = torch.tensor(sp[0][1]), 'zero'
    for j, (f, r) in enumerate(sp[1:]):
        i = n - 1 - j
        if i <= 0:
            break
        aa[i], fam[i] = torch.tensor(r, dtype=torch.float64).float(), f
    return aa, fam


def rodrigues_excluded(aa):
    """rows whose three components are all within 1e-7 of -1e-8: angle = ||r + 1e-8|| vanishes there and d = r / angle is singular, in the
    reference too"""
    return ((aa.double() + 1e-8).abs() <= 1e-7).all(dim=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. projections

ORTHO = [(1, 1, 3), (1, 17, 3), (3, 85, 160), (3, 86, 160), (2, 6890, 3)]            # B, N, ld_cam
ORTHO_BWD_N, ORTHO_BWD_B = (1, 17, 63, 64, 65, 255, 256, 257, 513, 6890), (1, 3)
PERSP = [(1, 1), (3, 85), (3, 86), (2, 6890)]
TARGETS_B = (1, 8, 9, 70)
COCO = list(O.ALL_JOINTS_TO_COCO_MAP)
H36M14 = [O.ALL_JOINTS_TO_H36M_MAP[j] for j in O.H36M_TO_J14]


def cam_rows(B, ld_cam, seed):
    """cam [B][ld_cam]: (s, tx, ty) in the first three columns, NaN in the others"""
    cam = torch.full((B, ld_cam), float('nan'))
    cam[:, 0] = det((B,), seed, 0.5, 1.5)
    cam[:, 1:3] = det((B, 2), seed + 1, -0.5, 0.5)
    return cam


def ortho_reference(pts, cam):
    """fl32(s * fl32(x + tx)): two roundings, no contraction possible -> fp32 [B][N][2]"""
    t = (pts[:, :, :2].double() + cam[:, None, 1:3].double()).float()
    return (cam[:, None, 0:1].double() * t.double()).float()


def ortho_bwd_reach(N):
    """-> (trips of thread 0, threads without a point, partial waves: lanes of a wave with unequal trip counts, waves without a point)"""
    trips = [len(range(t, N, 256)) for t in range(256)]
    waves = [trips[64 * w:64 * w + 64] for w in range(4)]
    return trips[0], sum(1 for t in trips if t == 0), any(len(set(w)) > 1 for w in waves), sum(1 for w in waves if max(w) == 0)


def ortho_bwd_reference(pts, cam, dout):
    """-> dpoints fp32 [B][N][3] (exact: fl32(s du), fl32(s dv), +0.0), dcam float64 [B][3], the bound [B][3]:
    (ceil(N / 256) + 12) 2^-24 sum |terms| -- the depth of the kernel's fixed summation tree plus the roundings of one term"""
    B, N = dout.shape[:2]
    s = cam[:, 0].double()
    dp = torch.zeros(B, N, 3)
    dp[:, :, :2] = (s[:, None, None] * dout.double()).float()
    tx = (pts[:, :, :2].double() + cam[:, None, 1:3].double()) * dout.double()
    dcam = torch.stack((tx.sum((1, 2)), s * dout[:, :, 0].double().sum(1), s * dout[:, :, 1].double().sum(1)), 1)
    mag = torch.stack((tx.abs().sum((1, 2)), (s[:, None] * dout[:, :, 0].double()).abs().sum(1), (s[:, None] * dout[:, :, 1].double()).abs().sum(1)), 1)
    return dp, dcam, (-(-N // 256) + 12) * U * mag


def persp_inputs(B, N, per_body, seed=600):
    """points in [-1, 1]^3, rotations = O.batch_rodrigues of rows in [-3, 3] rounded to fp32, translations with z in [2, 20], K = the intrinsics of
    the oracle (one matrix) or one per body with a non-zero skew entry"""
    pts = det((B, N, 3), seed)
    rot = O.batch_rodrigues(det((B, 3), seed + 1, -3, 3).double()).float()
    tr = torch.cat((det((B, 2), seed + 2, -0.5, 0.5), det((B, 1), seed + 3, 2.0, 20.0)), 1)
    K0 = torch.from_numpy(O.intrinsics_matrix()).float()
    if per_body:
        K = K0[None].repeat(B, 1, 1)
        K[:, 0, 1] = det((B,), seed + 4, 1.0, 40.0)            # skew
        K[:, 0, 0] += det((B,), seed + 5, -500, 500)
        K[:, 1, 1] += det((B,), seed + 6, -500, 500)
    else:
        K = K0
    return pts, rot, tr, K.contiguous()


def persp_eval(pts, rot, tr, K, dtype):
    B = pts.shape[0]
    Kb = K if K.dim() == 3 else K[None].expand(B, 3, 3)
    return O.perspective_project(pts.to(dtype), rot.to(dtype), tr.to(dtype), Kb.to(dtype))


_MEASURED = {}


def persp_fp32_cpu_error():
    """the worst per-element error of O.perspective_project evaluated in fp32 on the CPU against its float64 value, over the inputs of every case of
    PERSP x k_per_body: the kernel gets 4 times this (another, equally valid operation order and contraction)"""
    if 'persp' not in _MEASURED:
        worst = 0.0
        for B, N in PERSP:
            for pb in (0, 1):
                a = persp_inputs(B, N, pb)
                worst = max(worst, float((persp_eval(*a, torch.float32).double() - persp_eval(*a, torch.float64)).abs().max()))
        _MEASURED['persp'] = worst
    return _MEASURED['persp']


def targets_inputs(B, seed=700):
    joints = det((B, 90, 3), seed)
    cam_t = torch.cat((det((B, 2), seed + 1, -0.5, 0.5), det((B, 1), seed + 2, 2.0, 20.0)), 1)
    return joints, cam_t


def targets_eval(joints, cam_t, dtype):
    B = joints.shape[0]
    K = torch.from_numpy(O.intrinsics_matrix()).to(dtype)[None].expand(B, 3, 3)
    eye = torch.eye(3, dtype=dtype)[None].expand(B, 3, 3)
    return O.perspective_project(joints[:, COCO].to(dtype), eye, cam_t.to(dtype), K)


def targets_fp32_cpu_error():
    if 'targets' not in _MEASURED:
        _MEASURED['targets'] = max(float((targets_eval(*targets_inputs(B), torch.float32).double() - targets_eval(*targets_inputs(B), torch.float64)).abs().max())
                                   for B in TARGETS_B)
    return _MEASURED['targets']


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. straps_adam_step

ADAM_N = (1, 255, 256, 257, 1048576, 1048577)
ADAM_STEPS = (1, 2, 1000)
ADAM_GRAD_SCALES = (1.0, 0.5, 1.0 / 3.0)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-4, 0.9, 0.999, 1e-8
GRID_CAP = 4096


def capped_grid(n, cap=GRID_CAP):
    g = (n + 255) // 256
    return cap if g > cap else (1 if g < 1 else g)


def stride_reach(n, grid):
    """a grid-stride loop of `grid` workgroups of 256 over n elements -> (workgroups, a second trip runs, the last trip is partial)"""
    return grid, n > grid * 256, n % (grid * 256) != 0


def adam_data(n, step, seed=800):
    """p in [-1, 1]; g in [-1e-2, 1e-2] mixed with exact zeros, 1e4 and 1e-20 (g^2 underflows); m, v zero at step 1, random (v non-negative) later"""
    p = det((n,), seed)
    g = det((n,), seed + 1, -1e-2, 1e-2)
    i = torch.arange(n)
    g[i % 11 == 0] = 0.0
    g[i % 13 == 1] = 1e4
    g[i % 17 == 2] = 1e-20
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = det((n,), seed + 2, -1e-2, 1e-2), det((n,), seed + 3, 0.0, 1e-4)
    return p, g, m, v


def adam_reference(p, g, m, v, step, grad_scale, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """the header's formula in float64 from the fp32 inputs and the fp32 values of the scalars; 1.f - b1 and 1.f - b2 are exact in fp32 for the
    defaults, so the reference uses 1 - float32(b).  -> dict of m, v, p (float64) and the per-element bounds.

    Roundings counted (u = 2^-24, each relative to the term it falls on):
      m: g * scale, (1 - b1) * g, b1 * m, the sum: 4 on the larger term -> 4 u (|b1 m| + |(1 - b1) g|)
      v: g * scale twice (it is squared), (1 - b2) * g, * g, the sum: 5 on the g^2 term; b2 * v and the sum: 2 on the other -> 5 u (b2 v + (1 - b2) g^2);
         below 2^-126 the fp32 result may be a denormal or flushed to zero: only v >= 0 is asked there
      p: the final subtraction rounds p_new once: u |p_new|.  The update step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps) carries m's 4, v's 5 halved by
         the square root (2.5), the roundings of step_size and inv_sqrt_bc2 to fp32 (2), and one each for sqrt, the product with inv_sqrt_bc2, the sum
         with eps, the product with step_size and the quotient (5): 13.5 if nothing contracts; the two multiply-adds of m and v contract to fused
         operations on this target (one rounding less each) -> 12 u |update|, the figure the issue sets.  m's roundings are relative to its larger
         term: where b1 m and (1 - b1) g cancel they exceed u |m|, and only the first term covers such an element (|update| <= 1e-3 here against
         |p| of the order 1); tests/test_head_cases_cpu.py holds an uncontracted fp32 evaluation on the CPU to the same bounds"""
    lr, b1, b2, eps, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(grad_scale)
    gd = g.double() * gs
    m1 = b1 * m.double() + (1 - b1) * gd
    v1 = b2 * v.double() + (1 - b2) * gd * gd
    upd = lr / (1 - b1 ** step) * m1 / (v1.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    p1 = p.double() - upd
    return dict(m=m1, v=v1, p=p1, upd=upd, m_bound=4 * U * ((b1 * m.double()).abs() + ((1 - b1) * gd).abs()),
                v_bound=5 * U * (b2 * v.double() + (1 - b2) * gd * gd), p_bound=U * p1.abs() + 12 * U * upd.abs(),
                untouched=(g == 0) & (m == 0) & (v == 0))


# ------------------------------------------------------------------------------------------------------------------------------------
# 8. straps_mse_fwd / straps_mse_bwd

MSE = [(1, 1), (3, 34), (7, 10), (70, 216), (65535, 1), (65536, 1), (65537, 1), (4681, 14)]           # rows, cols; the last: 65534 elements
MSE_BWD_EXTRA = [(1048577, 1)]
MSE_MASKS = ('null', 'ones', 'half', 'one_row')
MSE_SCALES = ((1.0, 0.0), (2.0 / 256.0, -1.0))
MSE_STRIDE = 256 * 256


def mse_data(rows, cols, mask_kind, scale, seed=900):
    """pred in [-1, 1]; targets in [-1, 1] for (1, 0) and in [0, 256] for the 2 / 256 x - 1 normalisation; mask: uint8 per row | None"""
    pred = det((rows, cols), seed)
    tgt = det((rows, cols), seed + 1) if scale[0] == 1.0 else det((rows, cols), seed + 1, 0.0, 256.0)
    if mask_kind == 'null':
        mask = None
    elif mask_kind == 'ones':
        mask = torch.ones(rows, dtype=torch.uint8)
    elif mask_kind == 'half':
        mask = (det((rows,), seed + 2) > 0).to(torch.uint8)
        mask[rows // 2] = 1
    elif mask_kind == 'one_row':
        mask = torch.zeros(rows, dtype=torch.uint8)
        mask[(rows * 2) // 3] = 1
    else:
        mask = torch.zeros(rows, dtype=torch.uint8)
    return pred, tgt, mask


def mse_reference(pred, tgt, mask, scale):
    """float64 from the fp32 data and the fp32 values of scale and shift -> dict: d [rows][cols], keep [rows] bool, sum, count, mean, the bounds of
    sum and mean, mag = |p| + |t ts| + |tb| (the bound of the backward is 4 u |c| mag)"""
    ts, tb = f32(scale[0]), f32(scale[1])
    rows, cols = pred.shape
    keep = torch.ones(rows, dtype=torch.bool) if mask is None else mask != 0
    d = pred.double() - (tgt.double() * ts + tb)
    s = float((d[keep] ** 2).sum())
    cnt = int(keep.sum()) * cols
    n = rows * cols
    sb = (-(-n // MSE_STRIDE) + 20) * U * s
    mean = s / cnt if cnt else float('nan')
    return dict(d=d, keep=keep, sum=s, count=cnt, mean=mean, sum_bound=sb, mean_bound=(sb / cnt + 2 * U * abs(mean)) if cnt else 0.0,
                mag=pred.double().abs() + (tgt.double() * ts).abs() + abs(tb))
