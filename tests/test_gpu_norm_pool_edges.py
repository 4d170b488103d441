"""GPU: the BatchNorm, pooling and pooling-gradient kernels at their loop edges, behind redzones (tests/redzone.py) -- the cases of tests/norm_cases.py,
which also states which loop form, trip count and tail each case reaches (tests/test_norm_cases_cpu.py holds that statement together).

Common form of every case:
  * every output, workspace, bit-word and arg-max buffer comes from Zone.guarded: NaN-filled (0x7FC0 for planes), exactly the advertised size, sentinel
    margins on both sides; plane outputs with a stride larger than their extent come from Zone.guarded_planes, whose gaps must stay untouched;
  * every operand comes from Zone.at_end (poison directly behind its last element): a used over-read is a NaN in the result;
  * the reference is float64 arithmetic on the CPU from the SAME fp32 inputs the kernel gets (mean, invstd, scale, shift are inputs, not recomputed),
    never another kernel of the library; where the kernel rounds an intermediate to fp32 by its definition (k1 = gamma * invstd, the fp32 scale that
    the shift is computed from, the fp32 mean and unbiased variance that enter the running statistics, the fp32 product (1 - momentum) * running_* that
    they are added to) the reference rounds the same value at the same place.  For bn_stats_finalize this means: mean and invstd meet the issue's
    bound against the plain float64 formula; scale, shift and the running statistics meet it against the float64 formula WITH those fp32 roundings,
    not against the unrounded one -- where the two terms of a running mean cancel, the distance to the unrounded formula is up to 2^-24 of the kept
    term (1 - momentum) * running_mean, which the issue's bound would not allow.  The running update is fp32 arithmetic by definition (fp32 state,
    fp32 momentum); what the test pins is that nothing beyond these roundings is lost;
  * comparisons are per element, or per channel for per-channel outputs -- never one norm over a tensor.

Bounds (derived, not tuned):
  * max-pool values, arg-max taps, bit words, dz, the max-pool gradient: exact;
  * bn_apply: at most 1 ulp from the float64 evaluation rounded where the kernel rounds (once after the multiply-add, once after the residual add);
  * sums accumulated in double and rounded once (dgamma, dbeta, draw, the statistics): |got - want| <= 2^-23 |want| + 1e-12 sum|terms|.
Every such check prints `RATIO <family> <worst error / bound>`.
"""
import pytest
import torch
import torch.nn.functional as F

import norm_cases as N
import straps_amd  # noqa: F401
from detgen import det_uniform
from redzone import BF16_NAN, Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
P = hipabi.ptr
NAN = float('nan')
INF = float('inf')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    lib = hipabi.load()
    import os
    assert os.path.abspath(lib._name) == os.path.abspath(hipabi.LIB_PATH), 'these tests run on the product library, not %s' % lib._name
    return torch.device('cuda:0')


_PERIOD = (1 << 19) + 17          # (odd against every channel count and row length of the tables)


def _det(shape, seed, lo=-1.0, hi=1.0):
    """det_uniform data as a CPU tensor; beyond 2^19 elements one det_uniform block repeated"""
    n = 1
    for d in shape:
        n *= d
    if n <= _PERIOD:
        return torch.from_numpy(det_uniform(tuple(shape), seed, lo, hi))
    blk = torch.from_numpy(det_uniform((_PERIOD,), seed, lo, hi))
    return blk.repeat(-(-n // _PERIOD))[:n].view(tuple(shape)).contiguous()


def _ord(t):
    """fp32 -> integers in the order of the values (both zeros map to 0): the distance of two values in ulps is the difference"""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _assert_ulps(got, want, n, what):
    assert bool(torch.isfinite(got).all()), '%s: not finite (an element nobody wrote, or a read past an operand)' % what
    d = (_ord(got) - _ord(want)).abs()
    worst = int(d.max()) if d.numel() else 0
    print('RATIO %s %d ulp' % (what, worst))
    assert worst <= n, '%s: %d ulp at flat index %d' % (what, worst, int(d.argmax()))


def _assert_bound(got, want, terms, what):
    """|got - want| <= 2^-23 |want| + 1e-12 sum|terms| element by element; -> the worst error / bound"""
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), '%s: not finite (an element nobody wrote, or a read past an operand)' % what
    err = (got.double() - want).abs()
    bound = 2.0 ** -23 * want.abs() + 1e-12 * terms
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('RATIO %s %.4f' % (what, worst))
    assert worst <= 1.0, '%s: error %.3e against a bound of %.3e at flat index %d' % (what, float(err.flatten()[ratio.argmax()]),
                                                                                      float(bound.flatten()[ratio.argmax()]), int(ratio.argmax()))
    return worst


def _fma32(a, b, c):
    """fp32 fused multiply-add of fp32 tensors: the product is exact in float64, the sum is rounded to 53 bits and then to 24"""
    return (a.double() * b.double() + c.double()).float()


def _pack_bits(y):
    """[rows][C] -> int32 words [rows][C / 32], bit (c & 31) = (y > 0)  (what straps_bn_apply_bits_x3 writes)"""
    C = y.shape[-1]
    b = (y.reshape(-1, C // 32, 32) > 0).to(torch.int64)
    wd = (b << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(wd >= 2 ** 31, wd - 2 ** 32, wd).to(torch.int32).contiguous()


def _bf16_rn(x):
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def _decode_planes(planes, rows, C, what):
    """chunk-major planes [3][ps] (element (r, c) at ((c >> 5) * rows + r) * 32 + (c & 31)) -> the fp32 tensor [rows][C] they represent; also asserts
    that the leading plane is the bf16 rounding of that value (the canonical split the convolution kernels are tested with)"""
    pl = planes.detach().cpu()[:, :rows * C].to(torch.int64) & 0xFFFF
    assert not bool((pl == BF16_NAN).any()), '%s: a plane element was not written' % what
    f = (pl << 16).to(torch.int32).view(torch.float32).double()
    v = (f[0] + f[1] + f[2]).float()
    assert bool(((f[0] + f[1] + f[2]) == v.double()).all()), '%s: the planes do not sum to an fp32 value' % what
    nz = v != 0
    assert bool((_bf16_rn(v)[nz] == pl[0][nz]).all()), '%s: the leading plane is not the bf16 rounding of the value' % what
    return v.view(C // 32, rows, 32).permute(1, 0, 2).reshape(rows, C).contiguous()


def _planes_out(z, n, mode, name):
    """mode 1: plane stride = n rounded up to 8 (redzone directly behind plane 2); mode 2: a stride larger than the extent, gaps guarded"""
    if mode == 2:
        return z.guarded_planes(n, gap=1024, name=name)
    ps = (n + 7) // 8 * 8
    return z.guarded((3, ps), torch.int16, fill=BF16_NAN, name=name), ps


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_bn_apply, straps_bn_apply_x3, straps_bn_apply_bits_x3

FMA_X, FMA_SCALE, FMA_SHIFT = 1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12, -(1.0 + 2.0 ** -11)      # fused: 2^-24; product rounded first (a tie, to even): 0


def _apply_inputs(a):
    rows, C = a.rows, a.c
    x = _det((rows, C), 21)
    sc, sh = _det((C,), 22, 0.5, 1.5), _det((C,), 23, -0.5, 0.5)
    res = _det((rows, C), 24) if a.res else None
    special = sorted({0, 1, rows // 2, rows - 1})
    sc[1], sh[1], sh[2], sh[3] = FMA_SCALE, FMA_SHIFT, 0.0, -0.0
    for r in special:
        x[r, 1], x[r, 2], x[r, 3] = FMA_X, 0.0, -0.0
        if res is not None:
            res[r, 1], res[r, 2], res[r, 3] = 0.0, 0.0, -0.0
    return x, sc, sh, res, special


@pytest.mark.parametrize('a', N.APPLY, ids=lambda a: '%s-%dx%d-res%d-relu%d-y%d-planes%d' % (a.entry, a.rows, a.c, a.res, a.relu, a.y, a.planes))
def test_bn_apply_against_float64(dev, a):
    L = hipabi.lib()
    rows, C = a.rows, a.c
    x, sc, sh, res, special = _apply_inputs(a)
    z = Zone(dev)
    xd, scd, shd, resd = z.at_end(x), z.at_end(sc), z.at_end(sh), z.at_end(res)
    y = z.guarded((rows, C), name='y') if a.y else None
    planes, ps = _planes_out(z, rows * C, a.planes, 'y planes') if a.planes else (None, 0)
    bits = z.guarded((rows, C // 32), torch.int32, fill=None, name='relu bits') if a.entry == 'bits' else None
    if bits is not None:
        bits.fill_(0x55AA55AA)
    if a.entry == 'plain':
        rc = L.straps_bn_apply(P(xd), P(scd), P(shd), P(resd), int(a.relu), P(y), rows, C, None)
    elif a.entry == 'x3':
        rc = L.straps_bn_apply_x3(P(xd), P(scd), P(shd), P(resd), int(a.relu), P(y), P(planes), ps, rows, C, None)
    else:
        rc = L.straps_bn_apply_bits_x3(P(xd), P(scd), P(shd), P(resd), P(y), P(planes), ps, P(bits), rows, C, None)
    hipabi.check(rc, 'bn_apply ' + a.entry)
    z.check()
    # reference: the multiply-add rounded once, the residual add rounded once
    w1 = _fma32(x, sc[None, :], sh[None, :])
    want = w1 if res is None else (w1.double() + res.double()).float()
    exact = x.double() * sc.double()[None, :] + sh.double()[None, :] + (0 if res is None else res.double())
    if a.relu:
        want, exact = want.clamp_min(0), exact.clamp_min(0)
    what = 'bn_apply[%s %dx%d]' % (a.entry, rows, C)
    got = y.cpu() if a.y else None
    if planes is not None:
        dec = _decode_planes(planes, rows, C, what)
        if got is None:
            got = dec
        else:
            assert torch.equal(_ord(dec), _ord(got)), '%s: the planes are not the split of y' % what
    _assert_ulps(got, want, 1, what)
    # against the unrounded float64 value: one ulp of the result, plus the half ulp of the multiply-add where a residual follows it
    err = (got.double() - exact).abs()
    ulp = 2.0 ** -23 * exact.abs().clamp_min(2.0 ** -126)
    assert bool((err <= ulp + (2.0 ** -24 * w1.double().abs() if res is not None else 0)).all()), what
    # the constructed elements: the fused result, exact zeros, -0.0
    for r in special:
        assert float(got[r, 1]) == 2.0 ** -24, '%s: row %d: %.9e is not the fused multiply-add result 2^-24' % (what, r, float(got[r, 1]))
        assert float(got[r, 2]) == 0.0 and float(got[r, 3]) == 0.0
    if bits is not None:
        assert torch.equal(bits.cpu(), _pack_bits(got)), '%s: bit words != (y > 0) packed' % what
        wb = bits.cpu()[special, 0]
        assert bool((((wb >> 1) & 1) == 1).all()) and bool((((wb >> 2) & 3) == 0).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_bn_bwd, _x3, _bits_x3, _finish_x3, _finish_bits_x3

def _bwd_inputs(rows, C, mask):
    dy, raw = _det((rows, C), 31), _det((rows, C), 32)
    mean, invstd, gamma = _det((C,), 33, -0.2, 0.2), _det((C,), 34, 0.5, 2.0), _det((C,), 35, 0.5, 1.5)
    msc = (gamma.double() * invstd.double()).float()
    msh = _det((C,), 36, -0.3, 0.3)
    act = _fma32(raw, msc[None, :], msh[None, :]).clamp_min(0)
    if mask == 'none':
        m = torch.ones(rows, C, dtype=torch.bool)
    else:
        m = act > 0
    return dy, raw, mean, invstd, gamma, msc, msh, act, m


def _bwd_reference(dy, raw, mean, invstd, gamma, m, rows, flags, old_dg, old_db):
    """-> dict of float64 wants and sum|terms| for dgamma, dbeta, draw; g = the masked gradient (exact)"""
    g = torch.where(m, dy, torch.zeros_like(dy))
    g64, xc = g.double(), raw.double() - mean.double()[None, :]
    is64 = invstd.double()
    S1, S2 = g64.sum(0), (g64 * xc).sum(0) * is64
    A1, A2 = g64.abs().sum(0), (g64 * xc).abs().sum(0) * is64
    acc = flags & 1
    # (the kernel rounds the sum to fp32 and, when it accumulates, adds the old value in fp32: the second rounding is the bound's 2^-23)
    wdb = S1.float().double() + old_db.double() if acc else S1
    wdg = S2.float().double() + old_dg.double() if acc else S2
    cnt = INF if flags & 2 else float(rows)
    m1, m2 = S1 / cnt, S2 / cnt
    k1 = (gamma.double() * is64).float().double()
    xh = xc * is64[None, :]
    draw = k1[None, :] * ((g64 - m1[None, :]) - xh * m2[None, :])
    terms = k1.abs()[None, :] * (g64.abs() + (A1 / cnt)[None, :] + xh.abs() * (A2 / cnt)[None, :])
    return dict(g=g, S1=S1, S2=S2, A1=A1, A2=A2, k1=k1, xh=xh, cnt=cnt, dbeta=wdb, dgamma=wdg, tb=A1 + (old_db.double().abs() if acc else 0), tg=A2 + (old_dg.double().abs() if acc else 0), draw=draw, terms=terms)


def _partials(g, raw, mean, invstd, nblk):
    """the [nblk][C][2] partial sums (S1, invstd * S2) of the _finish forms, in float64, over nblk contiguous row ranges (some empty when nblk > rows)"""
    rows, C = g.shape
    bid = (torch.arange(rows, dtype=torch.int64) * nblk) // rows
    g64 = g.double()
    p = torch.zeros(nblk, C, 2, dtype=torch.float64)
    p[:, :, 0].index_add_(0, bid, g64)
    p[:, :, 1].index_add_(0, bid, g64 * (raw.double() - mean.double()[None, :]) * invstd.double()[None, :])
    return p


def _run_bwd(dev, b, what):
    L = hipabi.lib()
    rows, C = b.rows, b.c
    dy, raw, mean, invstd, gamma, msc, msh, act, m = _bwd_inputs(rows, C, b.mask)
    old_dg, old_db = _det((C,), 37, -3, 3), _det((C,), 38, -3, 3)
    z = Zone(dev)
    dyd, rawd, md, isd, gd = z.at_end(dy), z.at_end(raw), z.at_end(mean), z.at_end(invstd), z.at_end(gamma)
    yact = z.at_end(act) if b.mask == 'yact' else None
    bits = z.at_end(_pack_bits(act)) if b.mask == 'bits' else None
    mscd, mshd = (z.at_end(msc), z.at_end(msh)) if b.mask == 'rederived' else (None, None)
    dg, db = z.guarded((C,), name='dgamma'), z.guarded((C,), name='dbeta')
    if b.flags & 1:
        dg.copy_(old_dg)
        db.copy_(old_db)
    draw = z.guarded((rows, C), name='draw') if b.draw else None
    dz = z.guarded((rows, C), name='dz') if b.dz else None
    planes, ps = _planes_out(z, rows * C, b.planes, 'draw planes') if b.planes else (None, 0)
    ref = _bwd_reference(dy, raw, mean, invstd, gamma, m, rows, b.flags, old_dg, old_db)
    finish = b.entry in ('finish', 'finish_bits')
    if finish:
        ws = z.guarded((N.bn_bwd_finish_workspace_bytes(C) // 4,), name='workspace')
        part = z.at_end(_partials(ref['g'], raw, mean, invstd, b.nblk))
    else:
        nbytes = L.straps_bn_bwd_workspace_bytes(rows, C)
        assert nbytes == N.straps_bn_bwd_workspace_bytes(rows, C)
        ws = z.guarded((nbytes // 4,), name='workspace')
    if b.entry == 'plain':
        rc = L.straps_bn_bwd(P(dyd), P(yact), P(rawd), P(md), P(isd), P(gd), P(mscd), P(mshd), P(dg), P(db), P(draw), P(dz), P(ws), rows, C, b.flags, None)
    elif b.entry == 'x3':
        rc = L.straps_bn_bwd_x3(P(dyd), P(yact), P(rawd), P(md), P(isd), P(gd), P(mscd), P(mshd), P(dg), P(db), P(draw), P(dz), P(planes), ps, P(ws), rows, C,
                                b.flags, None)
    elif b.entry == 'bits':
        rc = L.straps_bn_bwd_bits_x3(P(dyd), P(bits), P(rawd), P(md), P(isd), P(gd), P(dg), P(db), P(draw), P(planes), ps, P(ws), rows, C, b.flags, None)
    elif b.entry == 'finish':
        rc = L.straps_bn_bwd_finish_x3(P(dyd), P(yact), P(rawd), P(md), P(isd), P(gd), P(mscd), P(mshd), P(dg), P(db), P(draw), P(dz), P(planes), ps, P(part),
                                       b.nblk, P(ws), rows, C, b.flags, None)
    else:
        rc = L.straps_bn_bwd_finish_bits_x3(P(dyd), P(bits), P(rawd), P(md), P(isd), P(gd), P(dg), P(db), P(draw), P(planes), ps, P(part), b.nblk, P(ws), rows, C,
                                            b.flags, None)
    hipabi.check(rc, what)
    z.check()
    _assert_bound(db, ref['dbeta'], ref['tb'], what + ' dbeta')
    _assert_bound(dg, ref['dgamma'], ref['tg'], what + ' dgamma')
    got = draw.cpu() if draw is not None else None
    if planes is not None:
        dec = _decode_planes(planes, rows, C, what)
        if got is None:
            got = dec
        else:
            assert torch.equal(_ord(dec), _ord(got)), '%s: the planes are not the split of draw' % what
    _assert_bound(got, ref['draw'], ref['terms'], what + ' draw')
    if dz is not None:
        assert torch.equal(_ord(dz.cpu()), _ord(ref['g'])), '%s: dz is not the masked dy' % what
    return got, dg.cpu(), db.cpu()


@pytest.mark.parametrize('b', N.BWD, ids=lambda b: '%s-%dx%d-%s-flags%d-dz%d-draw%d-planes%d-nblk%d' % (b.entry, b.rows, b.c, b.mask, b.flags, b.dz, b.draw, b.planes, b.nblk))
def test_bn_backward_against_float64(dev, b):
    _run_bwd(dev, b, 'bn_bwd[%s %dx%d]' % (b.entry, b.rows, b.c))


@pytest.mark.parametrize('B,H,C', N.AUTOGRAD)
def test_bn_backward_against_float64_autograd(dev, B, H, C):
    """the formula itself, independently: F.batch_norm + ReLU float64 autograd, at the bars of test_gpu_backward.py::test_bn_backward (5e-5 of the
    maximum).  The one norm over a tensor is deliberate and inherited from that test: this is the independent check of the formula the issue asks to keep at
    its existing bar; every other comparison of this file is per element or per channel -- do not copy `rel` elsewhere."""
    L = hipabi.lib()
    rows = B * H * H
    x = _det((B, C, H, H), 41).double().requires_grad_()
    g = _det((C,), 42, 0.5, 1.5).double().requires_grad_()
    bb = _det((C,), 43, -0.5, 0.5).double().requires_grad_()
    out = F.relu(F.batch_norm(x, None, None, g, bb, True, 0.1, 1e-5))
    dy = _det(tuple(out.shape), 44).double()
    out.backward(dy)
    xs = x.detach()
    mean, invstd = xs.mean(dim=(0, 2, 3)).float(), (1.0 / torch.sqrt(xs.var(dim=(0, 2, 3), unbiased=False) + 1e-5)).float()
    nhwc = lambda t: t.detach().float().permute(0, 2, 3, 1).contiguous()
    z = Zone(dev)
    dg, db, draw = z.guarded((C,), name='dgamma'), z.guarded((C,), name='dbeta'), z.guarded((rows, C), name='draw')
    ws = z.guarded((L.straps_bn_bwd_workspace_bytes(rows, C) // 4,), name='workspace')
    hipabi.check(L.straps_bn_bwd(P(z.at_end(nhwc(dy))), P(z.at_end(nhwc(out))), P(z.at_end(nhwc(xs))), P(z.at_end(mean)), P(z.at_end(invstd)), P(z.at_end(g.detach().float())),
                                 None, None, P(dg), P(db), P(draw), None, P(ws), rows, C, 0, None), 'bn_bwd')
    z.check()
    rel = lambda a, r: float((a.cpu().double() - r).abs().max() / r.abs().max())
    e = (rel(draw.view(B, H, H, C).permute(0, 3, 1, 2), x.grad), rel(dg, g.grad), rel(db, bb.grad))
    print('RATIO bn_bwd autograd[%dx%d] draw %.3e dgamma %.3e dbeta %.3e (bar 5e-5)' % (rows, C, e[0], e[1], e[2]))
    assert max(e) < 5e-5, e


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_bn_stats_finalize, straps_bn_fold, straps_bn_fold_stats

def _stat_partials(nblocks, C, per_block):
    """fp32 (sum, sum of squares) partials of `per_block` samples each; channel 0 is a CONSTANT channel whose rounded second sum falls below
    count x mean^2 (the variance clamp at zero)"""
    mu, sd = _det((C,), 51, -1, 1).double(), _det((C,), 52, 0.5, 1.5).double()
    p = torch.empty(nblocks, C, 2, dtype=torch.float64)
    p[:, :, 0] = per_block * (mu[None, :] + 0.1 * _det((nblocks, C), 53).double())
    p[:, :, 1] = per_block * (sd[None, :] ** 2 + mu[None, :] ** 2 + 0.1 * _det((nblocks, C), 54).double())
    p[:, 0, 0], p[:, 0, 1] = 3.0 * per_block, 9.0 * per_block * (1 - 2.0 ** -20)
    return p.float()


def _check_stats(dev, nblocks, C, count, per_block, running=True, save=True, what=''):
    L = hipabi.lib()
    eps, mom = 1e-5, 0.1
    part = _stat_partials(nblocks, C, per_block)
    if count == 1:
        part[0, :, 0], part[0, :, 1] = 1.5, 2.25
    gamma, beta = _det((C,), 55, 0.5, 1.5), _det((C,), 56, -0.5, 0.5)
    rm0, rv0 = _det((C,), 57, -1, 1), _det((C,), 58, 0.5, 2.0)
    z = Zone(dev)
    scale, shift = z.guarded((C,), name='scale'), z.guarded((C,), name='shift')
    smean, sinv = (z.guarded((C,), name='save_mean'), z.guarded((C,), name='save_invstd')) if save else (None, None)
    rm, rv = (z.guarded((C,), name='running_mean'), z.guarded((C,), name='running_var')) if running else (None, None)
    if running:
        rm.copy_(rm0)
        rv.copy_(rv0)
    hipabi.check(L.straps_bn_stats_finalize(P(z.at_end(part)), nblocks, C, count, P(z.at_end(gamma)), P(z.at_end(beta)), eps, mom, P(rm), P(rv), P(scale), P(shift),
                                            P(smean), P(sinv), None), 'bn_stats_finalize')
    z.check()
    # reference: the same fp32 partials summed in float64, the same formula
    e32, m32 = torch.tensor(eps, dtype=torch.float32).double(), torch.tensor(mom, dtype=torch.float32)
    p = part.double()
    s1, s2, a1, a2 = p[:, :, 0].sum(0), p[:, :, 1].sum(0), p[:, :, 0].abs().sum(0), p[:, :, 1].abs().sum(0)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    inv = 1.0 / torch.sqrt(var + e32)
    t_mean = a1 / count
    t_var = a2 / count + mean * mean + 2 * mean.abs() * t_mean
    t_inv = 0.5 * inv / (var + e32) * t_var
    assert float(var[0]) == 0.0 and bool((var[1:] > 0).all()) or count == 1
    sc = gamma.double() * inv.float().double()                       # (the kernel's scale is the fp32 gamma times the fp32 invstd)
    sh = beta.double() - mean.float().double() * sc.float().double()         # (one fused multiply-add of the fp32 mean and the fp32 scale)
    w = what or 'bn_stats_finalize[C=%d nblocks=%d]' % (C, nblocks)
    if save:
        _assert_bound(smean, mean, t_mean, w + ' mean')
        _assert_bound(sinv, inv, t_inv, w + ' invstd')
    _assert_bound(scale, sc, gamma.double().abs() * t_inv, w + ' scale')
    _assert_bound(shift, sh, beta.double().abs() + (mean * sc).abs() + sc.abs() * t_mean + mean.abs() * gamma.double().abs() * t_inv, w + ' shift')
    if running:
        unb = var * count / (count - 1.0) if count > 1 else var
        keep = (1.0 - m32)                                            # fp32
        k_rm, k_rv = (keep * rm0).double(), (keep * rv0).double()    # fp32 products, then one fused multiply-add each
        wm = m32.double() * mean.float().double() + k_rm
        wv = m32.double() * unb.float().double() + k_rv
        _assert_bound(rm, wm, k_rm.abs() + m32.double() * (mean.abs() + t_mean), w + ' running_mean')
        _assert_bound(rv, wv, k_rv.abs() + m32.double() * (unb.abs() + t_var), w + ' running_var')


@pytest.mark.parametrize('nblocks', N.STATS_NBLOCKS)
def test_bn_stats_finalize_against_float64(dev, nblocks):
    for C in N.STATS_C:
        _check_stats(dev, nblocks, C, 64 * nblocks, 64)


def test_bn_stats_finalize_options(dev):
    _check_stats(dev, 1, 6, 1, 1, what='bn_stats_finalize[count=1]')
    _check_stats(dev, 65, 130, 65 * 64, 64, running=False, what='bn_stats_finalize[no running]')
    _check_stats(dev, 961, 3, 961 * 64, 64, save=False, what='bn_stats_finalize[no save]')
    _check_stats(dev, 64, 64, 64 * 64, 64, running=False, save=False, what='bn_stats_finalize[scale and shift only]')


@pytest.mark.parametrize('C', N.STATS_C)
def test_bn_fold_against_float64(dev, C):
    """fp32 arithmetic: var + eps, the square root and the division are each correctly rounded (2^-24 relative, the first halved by the root): scale and
    invstd within 3 x 2^-24; the shift is one fused multiply-add of the rounded scale: 2^-24 |shift| + 3 x 2^-24 |mean x scale|"""
    L = hipabi.lib()
    eps = 1e-5
    gamma, beta, mean, var = _det((C,), 61, 0.5, 1.5), _det((C,), 62, -0.5, 0.5), _det((C,), 63, -1, 1), _det((C,), 64, 0.0, 2.0)
    var[0] = 0.0
    e32 = torch.tensor(eps, dtype=torch.float32).double()
    inv = 1.0 / torch.sqrt(var.double() + e32)
    sc = gamma.double() * inv
    sh = beta.double() - mean.double() * sc
    u = 2.0 ** -24
    for stats in (False, True):
        z = Zone(dev)
        scale, shift, smean, sinv = (z.guarded((C,), name=n) for n in ('scale', 'shift', 'save_mean', 'save_invstd'))
        args = (P(z.at_end(gamma)), P(z.at_end(beta)), P(z.at_end(mean)), P(z.at_end(var)), eps, P(scale), P(shift))
        if stats:
            hipabi.check(L.straps_bn_fold_stats(*args, P(smean), P(sinv), C, None), 'bn_fold_stats')
        else:
            hipabi.check(L.straps_bn_fold(*args, C, None), 'bn_fold')
        z.check()
        es, eh = (scale.cpu().double() - sc).abs() / (3 * u * sc.abs()), (shift.cpu().double() - sh).abs() / (u * sh.abs() + 3 * u * (mean.double() * sc).abs())
        print('RATIO bn_fold%s[C=%d] scale %.4f shift %.4f' % ('_stats' if stats else '', C, float(es.max()), float(eh.max())))
        assert float(es.max()) <= 1 and float(eh.max()) <= 1
        if stats:
            assert torch.equal(smean.cpu(), mean)
            ei = (sinv.cpu().double() - inv).abs() / (3 * u * inv)
            print('RATIO bn_fold_stats[C=%d] invstd %.4f' % (C, float(ei.max())))
            assert float(ei.max()) <= 1
        else:
            assert bool(torch.isnan(smean).all()) and bool(torch.isnan(sinv).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# pooling

def _pool_input(B, H, W, C, seed, content):
    """NHWC input: 'ties' = few distinct values (many exact ties) with an all-negative band along every border, '+inf' adds +-inf, '+nan' NaNs too"""
    x = (_det((B, H, W, C), seed) * 4).round() / 4
    x[:, :2], x[:, -2:], x[:, :, :2], x[:, :, -2:] = -1 - x[:, :2].abs(), -1 - x[:, -2:].abs(), -1 - x[:, :, :2].abs(), -1 - x[:, :, -2:].abs()
    f = x.view(-1)
    if content in ('+inf', '+nan'):
        f[3::97], f[11::101] = INF, -INF
        x[0, :2, :2, :] = -INF                                         # window (0, 0) covers input rows / columns 0..1 only: a window of nothing but -inf
    if content == '+nan':
        f[5::89] = NAN
    return x


def _pool_reference(x_nhwc):
    """CPU F.max_pool2d(3, 2, 1, return_indices=True) -> (values NHWC, tap numbers NHWC uint8: 3 x (row inside the window) + column inside the window)"""
    B, H, W, C = x_nhwc.shape
    y, flat = F.max_pool2d(x_nhwc.permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    Ho, Wo = y.shape[2], y.shape[3]
    hi, wi = flat // W, flat % W
    ho, wo = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    tap = (hi - (2 * ho - 1)) * 3 + (wi - (2 * wo - 1))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 8
    return y.permute(0, 2, 3, 1).contiguous(), tap.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def _same(a, b):
    """bit-for-bit as values: NaN equals NaN, the two zeros are one value"""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _pool_grad_reference(dy, tap, H, W):
    """the gradient of the un-pooled tensor: the <= 4 windows that cover an element added in fp32 in ascending (ho, wo) -- the order of maxpool_bwd_kernel
    and pool_grad, csrc/backward.hip -- and the same sum in float64"""
    B, Ho, Wo, C = dy.shape
    g32, g64 = torch.zeros(B, H, W, C), torch.zeros(B, H, W, C, dtype=torch.float64)
    for r in (2, 1, 0):                     # ascending ho is descending row-inside-the-window
        for s in (2, 1, 0):
            hi, wi = 2 * torch.arange(Ho) - 1 + r, 2 * torch.arange(Wo) - 1 + s
            vh, vw = (hi >= 0) & (hi < H), (wi >= 0) & (wi < W)
            d = torch.where(tap == r * 3 + s, dy, torch.zeros_like(dy))[:, vh][:, :, vw]
            ih, iw = hi[vh], wi[vw]
            g32[:, ih[:, None], iw[None, :]] += d
            g64[:, ih[:, None], iw[None, :]] += d.double()
    return g32, g64


POOL_FWD = [(s, c) for s, c in zip(N.POOL_SMALL, ('+inf', '+inf', '+nan', 'ties', '+nan', '+inf', 'ties', '+inf'))] + [(N.POOL_FWD_BIG, '+nan')]


@pytest.mark.parametrize('shape,content', POOL_FWD, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_maxpool_forward_equals_max_pool2d(dev, shape, content):
    L = hipabi.lib()
    B, H, W, C = shape
    Ho, Wo = N.pool_out(H), N.pool_out(W)
    x = _pool_input(B, H, W, C, 71, content)
    wy, wtap = _pool_reference(x)
    z = Zone(dev)
    xd = z.at_end(x)
    y0, y1 = z.guarded((B, Ho, Wo, C), name='y'), z.guarded((B, Ho, Wo, C), name='y (idx form)')
    idx = z.guarded((B, Ho, Wo, C), torch.uint8, fill=None, name='idx')
    idx.fill_(0xEE)
    hipabi.check(L.straps_maxpool_fwd(P(xd), P(y0), B, H, W, C, None), 'maxpool_fwd')
    hipabi.check(L.straps_maxpool_fwd_idx(P(xd), P(y1), P(idx), B, H, W, C, None), 'maxpool_fwd_idx')
    z.check()
    assert _same(y0.cpu(), wy), 'maxpool_fwd: values differ from F.max_pool2d'
    assert _same(y1.cpu(), wy), 'maxpool_fwd_idx: values differ from F.max_pool2d'
    assert torch.equal(idx.cpu(), wtap), 'maxpool_fwd_idx: arg-max taps differ from F.max_pool2d'


def _stem_tail_inputs(B, H, W, C, inf):
    raw = _pool_input(B, H, W, C, 72, '+inf' if inf else 'ties')
    sc, sh = _det((C,), 73, 0.5, 1.5), (_det((C,), 74, -2, 2) * 4).round() / 8
    act = _fma32(raw, sc.view(1, 1, 1, C), sh.view(1, 1, 1, C)).clamp_min(0)
    return raw, sc, sh, act


@pytest.mark.parametrize('shape', N.POOL_SMALL + [N.POOL_FWD_BIG], ids=lambda s: 'x'.join(map(str, s)))
def test_bn_relu_maxpool_forward_equals_max_pool2d(dev, shape):
    L = hipabi.lib()
    B, H, W, C = shape
    Ho, Wo = N.pool_out(H), N.pool_out(W)
    raw, sc, sh, act = _stem_tail_inputs(B, H, W, C, inf=True)
    wy, wtap = _pool_reference(act)
    for x3 in ((0,) if C % 32 else (0, 1, 2) if B * H * W * C < (1 << 20) else (0, 2)):
        z = Zone(dev)
        y = z.guarded((B, Ho, Wo, C), name='y_pool')
        idx = z.guarded((B, Ho, Wo, C), torch.uint8, fill=None, name='idx')
        idx.fill_(0xEE)
        args = (P(z.at_end(raw)), P(z.at_end(sc)), P(z.at_end(sh)), P(y), P(idx))
        if x3:
            planes, ps = _planes_out(z, B * Ho * Wo * C, x3, 'y planes')
            hipabi.check(L.straps_bn_relu_maxpool_fwd_x3(*args, P(planes), ps, B, H, W, C, None), 'bn_relu_maxpool_fwd_x3')
        else:
            hipabi.check(L.straps_bn_relu_maxpool_fwd(*args, B, H, W, C, None), 'bn_relu_maxpool_fwd')
        z.check()
        assert _same(y.cpu(), wy) and torch.equal(idx.cpu(), wtap), 'bn_relu_maxpool_fwd (planes %d): differs from F.max_pool2d of relu(fma(raw, scale, shift))' % x3
        if x3:
            dec = _decode_planes(planes, B * Ho * Wo, C, 'bn_relu_maxpool_fwd_x3')
            assert _same(dec.view(B, Ho, Wo, C), wy)


@pytest.mark.parametrize('shape', N.POOL_SMALL + N.POOL_BWD_BIG, ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_backward_and_pooled_bn_backward(dev, shape):
    """straps_maxpool_bwd: exact against the fp32 sum in the kernel's order (and within 3 roundings of the float64 sum); straps_bn_bwd_pooled: dgamma, dbeta
    and draw against float64 from that gradient, flags 0 and 3"""
    L = hipabi.lib()
    B, H, W, C = shape
    Ho, Wo = N.pool_out(H), N.pool_out(W)
    raw, msc, msh, act = _stem_tail_inputs(B, H, W, C, inf=False)
    _, tap = _pool_reference(act)
    dyp = _det((B, Ho, Wo, C), 75)
    g32, g64 = _pool_grad_reference(dyp, tap, H, W)
    z = Zone(dev)
    dyd, tapd = z.at_end(dyp), z.at_end(tap)
    dx = z.guarded((B, H, W, C), name='dx')
    hipabi.check(L.straps_maxpool_bwd(P(dyd), P(tapd), P(dx), B, H, W, C, None), 'maxpool_bwd')
    z.check()
    assert torch.equal(_ord(dx.cpu()), _ord(g32)), 'maxpool_bwd: differs from the fp32 sum over the covering windows in ascending (ho, wo)'
    assert bool(((dx.cpu().double() - g64).abs() <= 3 * 2.0 ** -24 * 4).all())            # (|dy| < 1, four terms, three additions)
    # the stem's BatchNorm backward from the pooled gradient
    rows = B * H * W
    mean, invstd, gamma = _det((C,), 76, -0.2, 0.2), _det((C,), 77, 0.5, 2.0), _det((C,), 78, 0.5, 1.5)
    m = (act > 0).view(rows, C)
    gm32 = torch.where(m, g32.view(rows, C), torch.zeros(rows, C)).double()             # the element's own gradient: the fp32 sum, exact by the check above
    for flags in ((0, 3) if rows * C < (1 << 20) else (0,)):
        old_dg, old_db = _det((C,), 37, -3, 3), _det((C,), 38, -3, 3)
        # S1, S2 are sums over the pooled grid of the routed gradient: in float64 that is the sum of the float64 gradient over the un-pooled grid
        ref = _bwd_reference(g64.view(rows, C), raw.view(rows, C), mean, invstd, gamma, m, rows, flags, old_dg, old_db)
        z = Zone(dev)
        dg, db, draw = z.guarded((C,), name='dgamma'), z.guarded((C,), name='dbeta'), z.guarded((rows, C), name='draw')
        if flags & 1:
            dg.copy_(old_dg)
            db.copy_(old_db)
        ws = z.guarded((L.straps_bn_bwd_workspace_bytes(rows, C) // 4,), name='workspace')
        hipabi.check(L.straps_bn_bwd_pooled(P(z.at_end(dyp)), P(z.at_end(tap)), P(z.at_end(raw)), P(z.at_end(mean)), P(z.at_end(invstd)), P(z.at_end(gamma)),
                                            P(z.at_end(msc)), P(z.at_end(msh)), P(dg), P(db), P(draw), P(ws), B, H, W, C, flags, None), 'bn_bwd_pooled')
        z.check()
        what = 'bn_bwd_pooled[%s flags %d]' % ('x'.join(map(str, shape)), flags)
        _assert_bound(db, ref['dbeta'], ref['tb'], what + ' dbeta')
        _assert_bound(dg, ref['dgamma'], ref['tg'], what + ' dgamma')
        k1, xh, cnt = ref['k1'], ref['xh'], ref['cnt']
        want = k1 * ((gm32 - ref['S1'] / cnt) - xh * (ref['S2'] / cnt))
        terms = k1.abs() * (gm32.abs() + ref['A1'] / cnt + xh.abs() * (ref['A2'] / cnt))
        _assert_bound(draw, want, terms, what + ' draw')


def test_sparse_pooled_bn_backward_leaves_inactive_tiles_untouched(dev):
    L = hipabi.lib()
    B, H, W, C = N.POOL_SPARSE
    Ho, Wo = N.pool_out(H), N.pool_out(W)
    ty, tx = (H + 1) // 2, (W + 31) // 32
    raw, msc, msh, act = _stem_tail_inputs(B, H, W, C, inf=False)
    _, tap = _pool_reference(act)
    dyp = _det((B, Ho, Wo, C), 75)
    g32, g64 = _pool_grad_reference(dyp, tap, H, W)
    rows = B * H * W
    mean, invstd, gamma = _det((C,), 76, -0.2, 0.2), _det((C,), 77, 0.5, 2.0), _det((C,), 78, 0.5, 1.5)
    tmap = (_det((B, ty, tx), 79) > 0).to(torch.uint8) * 7                                 # active tiles are marked with a non-zero byte
    tmap[0, 0, 0], tmap[-1, -1, -1], tmap[0, -1, 0] = 1, 255, 0
    assert 0 < int((tmap > 0).sum()) < tmap.numel()
    m = (act > 0).view(rows, C)
    zero = torch.zeros(C)
    ref = _bwd_reference(g64.view(rows, C), raw.view(rows, C), mean, invstd, gamma, m, rows, 0, zero, zero)
    z = Zone(dev)
    dg, db, draw = z.guarded((C,), name='dgamma'), z.guarded((C,), name='dbeta'), z.guarded((B, H, W, C), name='draw')
    ws = z.guarded((L.straps_bn_bwd_workspace_bytes(rows, C) // 4,), name='workspace')
    hipabi.check(L.straps_bn_bwd_pooled_sparse(P(z.at_end(dyp)), P(z.at_end(tap)), P(z.at_end(raw)), P(z.at_end(mean)), P(z.at_end(invstd)), P(z.at_end(gamma)),
                                               P(z.at_end(msc)), P(z.at_end(msh)), P(dg), P(db), P(draw), P(ws), B, H, W, C, 0, P(z.at_end(tmap)), None), 'bn_bwd_pooled_sparse')
    z.check()
    _assert_bound(db, ref['dbeta'], ref['tb'], 'bn_bwd_pooled_sparse dbeta')
    _assert_bound(dg, ref['dgamma'], ref['tg'], 'bn_bwd_pooled_sparse dgamma')
    on = (tmap > 0)[:, torch.arange(H) // 2][:, :, torch.arange(W) // 32]                  # [B][H][W]
    got = draw.cpu()
    assert bool(torch.isnan(got[~on]).all()), 'an inactive tile was written'
    k1 = (gamma.double() * invstd.double()).float().double()
    xh = (raw.double() - mean.double()) * invstd.double()
    g = torch.where(m.view(B, H, W, C), g32, torch.zeros_like(g32)).double()
    want = k1 * ((g - ref['dbeta'] / rows) - xh * (ref['dgamma'] / rows))
    terms = k1.abs() * (g.abs() + ref['tb'] / rows + xh.abs() * ref['tg'] / rows)
    _assert_bound(got[on], want[on], terms[on], 'bn_bwd_pooled_sparse draw (active tiles)')


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_gap_fwd, straps_gap_bwd, straps_masked_copy

@pytest.mark.parametrize('B,HW,C', N.GAP_FWD)
def test_gap_forward(dev, B, HW, C):
    """gap_kernel adds the HW values of a (batch, channel) in fp32 in ascending position and divides by (float)HW.  Bound: twice the error of the same fp32
    sum and division done on the CPU in that order, against the float64 mean -- no error at all where the CPU sum is exact (hw = 1).  Measured: the
    reference error is at most 4.43e-8 over these cases (|x| < 1, HW <= 64); the kernel's results equal the CPU's fp32 results bit for bit, which is
    asserted beside the bound: worst error / bound 0.5 wherever the reference has an error, 0 elsewhere."""
    L = hipabi.lib()
    x = _det((B, HW, C), 81)
    z = Zone(dev)
    y = z.guarded((B, C), name='y')
    hipabi.check(L.straps_gap_fwd(P(z.at_end(x)), P(y), B, HW, C, None), 'gap_fwd')
    z.check()
    s = torch.zeros(B, C)
    for k in range(HW):
        s = s + x[:, k]
    cpu32 = s / torch.tensor(float(HW))
    want = x.double().mean(1)
    ref_err = (cpu32.double() - want).abs()
    err = (y.cpu().double() - want).abs()
    bound = 2 * ref_err
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
    print('RATIO gap_fwd[%dx%dx%d] %.4f (reference error %.3e, kernel error %.3e)' % (B, HW, C, float(ratio.max()), float(ref_err.max()), float(err.max())))
    assert bool(torch.isfinite(y).all()) and bool((err <= bound).all())
    assert torch.equal(y.cpu(), cpu32), 'gap_fwd: not the fp32 sum in ascending position divided by (float)HW'


@pytest.mark.parametrize('B,HW,C', N.GAP_BWD)
def test_gap_backward(dev, B, HW, C):
    """dx = dfeat x fl(1 / HW): equal to that fp32 product, and within the two roundings (2^-23 relative) of dfeat / HW"""
    L = hipabi.lib()
    df = _det((B, C), 82)
    z = Zone(dev)
    dx = z.guarded((B, HW, C), name='dx')
    hipabi.check(L.straps_gap_bwd(P(z.at_end(df)), P(dx), B, HW, C, None), 'gap_bwd')
    z.check()
    inv = torch.tensor(1.0) / torch.tensor(float(HW))
    got = dx.cpu()
    assert torch.equal(got, (df * inv)[:, None, :].expand(B, HW, C))
    want = (df.double() / HW)[:, None, :].expand(B, HW, C)
    assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all())


@pytest.mark.parametrize('m,n,ldx,ldm,ldy', N.MASKED_COPY)
def test_masked_copy(dev, m, n, ldx, ldm, ldy):
    L = hipabi.lib()
    span = lambda ld: (m - 1) * ld + n                       # the buffers end with the last element the kernel may touch
    x, mk, y0 = _det((span(ldx),), 83), _det((span(ldm),), 84), _det((span(ldy),), 85)
    mk[::7] = 0.0
    mk[3::11] = -0.0
    view = lambda t, ld: torch.as_strided(t, (m, n), (ld, 1))
    for masked, acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
        z = Zone(dev)
        y = z.guarded((span(ldy),), name='y')
        y.copy_(y0)
        hipabi.check(L.straps_masked_copy(P(z.at_end(x)), ldx, P(z.at_end(mk)) if masked else None, ldm, P(y), ldy, m, n, acc, None), 'masked_copy')
        z.check()
        v = view(x, ldx)
        if masked:
            v = torch.where(view(mk, ldm) > 0, v, torch.zeros_like(v))
        want = y0.clone()
        wv = view(want, ldy)
        wv.copy_(wv + v if acc else v)                       # (one fp32 addition, as in the kernel; the columns between n and ldy keep what they held)
        assert torch.equal(_ord(y.cpu()), _ord(want)), (masked, acc)


# ----------------------------------------------------------------------------------------------------------------------------------------
# argument checks

@pytest.mark.parametrize('bad', ['batch', 'h', 'w', 'c'])
@pytest.mark.parametrize('value', [0, -1])
def test_pooling_entries_refuse_empty_shapes(dev, bad, value):
    """h = 0 gives Ho = (0 - 1) / 2 + 1 = 1 by C division: before the check maxpool_fwd_idx wrote a row of -inf into a zero-sized output.  The buffers
    here hold a 1 x 1 x 4-channel output, so the call is harmless either way."""
    L = hipabi.lib()
    shape = dict(batch=1, h=1, w=1, c=4)
    shape[bad] = value
    a = (shape['batch'], shape['h'], shape['w'], shape['c'])
    z = Zone(dev)
    x, sc, sh = z.at_end(torch.ones(16)), z.at_end(torch.ones(16)), z.at_end(torch.zeros(16))
    y, dx = z.guarded((16,), name='y'), z.guarded((16,), name='dx')
    idx = z.guarded((16,), torch.uint8, fill=None, name='idx')
    idx.fill_(0)
    for name, call in (('straps_maxpool_fwd_idx', lambda: L.straps_maxpool_fwd_idx(P(x), P(y), P(idx), *a, None)),
                       ('straps_maxpool_bwd', lambda: L.straps_maxpool_bwd(P(x), P(idx), P(dx), *a, None))):
        rc = call()
        msg = L.straps_last_error().decode() if rc else ''
        assert rc == 1 and name in msg and ('%s=%d' % (bad, value)) in msg, (name, rc, msg)
    rc = L.straps_bn_relu_maxpool_fwd_x3(P(x), P(sc), P(sh), P(y), P(idx), None, 0, *a, None)
    assert rc == 1 and b'straps_bn_relu_maxpool_fwd' in L.straps_last_error()
    rc = L.straps_maxpool_fwd(P(x), P(y), *a, None)
    assert rc == 1
    z.check()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(dx).all())
