"""GPU: the IEF regressor's GEMM kernels at their edges, behind redzones (tests/redzone.py) -- straps_linear_fwd, straps_gemm_multi,
straps_ief_pack, straps_broadcast_rows (csrc/ief.hip); the cases, the launch rules they reach and the float64 references are tests/head_cases.py,
held together by tests/test_head_cases_cpu.py (which also holds the argument checks: they return before a launch).

Common form of every case:
  * every output comes from Zone.guarded: NaN-filled, exactly the advertised size, sentinel margins; where the leading dimension is larger than
    the extent (ldo, ldc, ldc2) the columns beyond the extent must still hold the NaN fill bit for bit;
  * every operand comes from Zone.at_end (poison directly behind its last element); the padding columns of x and w (ldx, ldw > kdim) hold NaN and
    must never be read; w has exactly ceil(n / 32) * 32 rows, rows >= n zero -- the header's contract, which the kernel uses (it does not clamp the
    w row) and straps_ief_pack provides: test_pack_feeds_linear holds the two against each other;
  * the reference is float64 arithmetic on the CPU from the same fp32 values, never another kernel of the library; comparisons are per element.

Two kinds of data per shape:
  * exact tracer: integers in {-2, ..., 2}; every product and partial sum is an integer below 2^24, so the result must equal the integer result
    whatever the summation order -- a dropped, duplicated or misrouted K group, lane or tail element is a wrong integer;
  * real data: det_uniform in [-1, 1], |got - want| <= (K + 16) 2^-24 sum_k |x w| + 2^-23 (|bias| + |addend| + |want|)  (K + 24 for gemm_multi,
    with the old value of an accumulating output in the place of the bias): the worst-case forward error of an fp32 dot product in any order
    plus the epilogue's additions.  Worst error / bound seen on an MI355X: linear_fwd 0.055, gemm_multi 0.112 (both at the shortest sums, where the
    bound is a few roundings; the long sums stay below 1/64: bound loose by construction, worst case over orders).
ief_pack and broadcast_rows are exact, bit for bit (the padding is +0.0).
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


def _split(buf, n, what):
    """a guarded [m][ld] output -> its [m][n] extent on the CPU, after asserting that the columns beyond the extent still hold the NaN fill bit for bit"""
    b = buf.detach().cpu()
    nan_bits = H.bits(torch.full((1,), NAN))[0]
    assert bool((H.bits(b[:, n:]) == nan_bits).all()), '%s: a column beyond the extent was written' % what
    return b[:, :n].contiguous()


def _same_bits(a, b, what):
    assert torch.equal(H.bits(a), H.bits(b)), '%s: not bit-identical (%d elements differ)' % (what, int((H.bits(a) != H.bits(b)).sum()))


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_linear_fwd

def _run_linear(dev, c, x, w, bias, addend, alias):
    L = hipabi.lib()
    z = Zone(dev)
    xd, wd, bd = z.at_end(x), z.at_end(w), z.at_end(bias)
    out = z.guarded((c.m, c.ldo), name='out')
    if addend is not None and alias:
        out.copy_(addend)                                   # the in-place estimate update: the columns beyond n stay NaN
        ad = out
    else:
        ad = z.at_end(addend)
    hipabi.check(L.straps_linear_fwd(P(xd), x.shape[1], P(wd), w.shape[1], P(bd), P(ad), P(out), c.ldo, c.m, c.n, c.k, c.relu, None), 'straps_linear_fwd')
    z.check()
    return _split(out, c.n, 'linear_fwd %s' % (c,))


@pytest.mark.parametrize('c', H.LINEAR, ids=lambda c: 'm%d-n%d-k%d-w%d-x%d-ldo%d-b%d-r%d-a%d' % tuple(c))
def test_linear_fwd(dev, c):
    """every case with tracer and real data; with an addend additionally with out == addend, bit for bit against the separate-buffer form"""
    for kind in ('tracer', 'real'):
        x, w, bias, addend = H.linear_data(c, kind)
        want, pre, bound = H.linear_reference(c, x, w, bias, addend)
        got = _run_linear(dev, c, x, w, bias, addend, False)
        if kind == 'tracer':
            assert bool(torch.isfinite(got).all()), 'not finite: an element nobody wrote, or a padding column / a row past the operand was read'
            assert torch.equal(got.double(), want), 'tracer: %d of %d elements are not the integer result' % (int((got.double() != want).sum()), got.numel())
            if c.relu:
                assert bool((got[pre <= 0] == 0).all()) and bool((H.bits(got[pre <= 0]) == 0).all())          # +0.0, not -0.0
        else:
            H.check_ratio('linear_fwd', got, want, bound)
        if addend is not None:
            _same_bits(_run_linear(dev, c, x, w, bias, addend, True), got, 'out aliasing addend')


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_gemm_multi

class _Problem:
    """one problem on the device: operands at_end, outputs guarded"""

    def __init__(self, z, c, d):
        self.c, self.d = c, d
        self.a, self.b = z.at_end(d['a']), z.at_end(d['b'])
        self.addend, self.mask = z.at_end(d['addend']), z.at_end(d['mask'])
        self.out = z.guarded((c.m, d['ldc']), name='c')
        if c.acc:
            self.out.copy_(d['c_old'])
        self.out2 = z.guarded((c.m, d['ldc']), name='c2') if c.c2 else None
        if c.c2 == 2:
            self.out2.copy_(d['c2_old'])

    def desc(self):
        c, d = self.c, self.d
        return hipabi.gemm_desc(self.a, d['sam'], d['sak'], self.b, d['sbk'], d['sbn'], self.out, d['ldc'], c.m, c.n, c.k, accumulate=c.acc,
                                addend=self.addend, ldadd=d['ldadd'], mask=self.mask, ldmask=c.n, c2=self.out2, ldc2=d['ldc'], accumulate2=int(c.c2 == 2))

    def results(self):
        c, d = self.c, self.d
        got = _split(self.out, c.n, 'gemm c') if not c.acc else self.out.detach().cpu()[:, :c.n].contiguous()
        if c.acc:
            _same_bits(self.out.detach().cpu()[:, c.n:], d['c_old'][:, c.n:], 'columns of an accumulating c beyond the extent')
        got2 = None
        if c.c2 == 1:
            got2 = _split(self.out2, c.n, 'gemm c2')
        elif c.c2 == 2:
            got2 = self.out2.detach().cpu()[:, :c.n].contiguous()
            _same_bits(self.out2.detach().cpu()[:, c.n:], d['c2_old'][:, c.n:], 'columns of an accumulating c2 beyond the extent')
        return got, got2


def _launch(dev, cases, kind, order=None):
    z = Zone(dev)
    probs = [_Problem(z, c, H.gemm_data(c, kind)) for c in cases]
    order = list(range(len(probs))) if order is None else order
    hipabi.gemm_multi([probs[i].desc() for i in order])
    z.check()
    return [p.results() for p in probs], probs


def _gemm_id(c):
    return 'm%d-n%d-k%d-%s-%s-ldc+%d-acc%d-c2%d-add%d-mask%d' % tuple(c)


@pytest.mark.parametrize('c', H.GEMM, ids=_gemm_id)
def test_gemm_multi_one_problem(dev, c):
    """a one-problem launch per case: tracer exact, real data within the bound; accumulate = 0 onto a NaN-filled c (the NaN must be overwritten, not
    read); masks of 0.0, -0.0, negative and NaN give exactly 0 (an accumulating output keeps its old value bit for bit there)"""
    for kind in ('tracer', 'real'):
        (res,), (p,) = _launch(dev, [c], kind)
        got, got2 = res
        v, want, want2, bound, bound2 = H.gemm_reference(c, p.d)
        for g, w_, b_, old, name in ((got, want, bound, p.d['c_old'] if c.acc else None, 'c'), (got2, want2, bound2, p.d['c2_old'], 'c2')):
            if g is None:
                continue
            if kind == 'tracer':
                assert bool(torch.isfinite(g).all()), '%s not finite: an element nobody wrote, a NaN that was accumulated onto, or a read past an operand' % name
                assert torch.equal(g.double(), w_), 'tracer %s: %d of %d elements are not the integer result' % (name, int((g.double() != w_).sum()), g.numel())
            else:
                H.check_ratio('gemm_multi', g, w_, b_)
            if p.d['mask'] is not None:
                off = ~(p.d['mask'] > 0)
                ref = old[:, :c.n] if old is not None else torch.zeros(c.m, c.n)
                assert bool((g[off] == ref[off]).all()), '%s: a masked element is not exactly 0 (or its old value)' % name
                if old is None:
                    assert bool((H.bits(g[off]) == 0).all()), '%s: a masked element is not +0.0' % name


@pytest.mark.parametrize('kind', ['tracer', 'real'])
def test_gemm_multi_eight_problems_equal_their_own_launches(dev, kind):
    """eight problems of different sizes in one launch, problem 0 1x1x1 and problem 7 65x65x300 (most workgroups of the small problems take the early
    return), in table order and reversed: every problem's result is bit-identical to its own one-problem launch"""
    cases = [H.GEMM[i] for i in H.GEMM_MULTI]
    alone = [_launch(dev, [c], kind)[0][0] for c in cases]
    for order in (list(range(8)), list(range(7, -1, -1))):
        together, _ = _launch(dev, cases, kind, order)
        for c, (g, g2), (a, a2) in zip(cases, together, alone):
            _same_bits(g, a, 'c of %s in the 8-problem launch' % (c,))
            if g2 is not None:
                _same_bits(g2, a2, 'c2 of %s in the 8-problem launch' % (c,))


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_ief_pack, straps_broadcast_rows

def _pack(dev, z, fc1, fc3, f, p, h1, h2, ld_e):
    L = hipabi.lib()
    p_pad = (p + 31) // 32 * 32
    w1f, w1e, w3 = z.guarded((h1, f), name='w1f'), z.guarded((h1, ld_e), name='w1e'), z.guarded((p_pad, h2), name='w3')
    hipabi.check(L.straps_ief_pack(P(z.at_end(fc1)), P(z.at_end(fc3)), P(w1f), P(w1e), P(w3), f, p, h1, h2, ld_e, None), 'straps_ief_pack')
    z.check()
    return w1f, w1e, w3


@pytest.mark.parametrize('case', H.PACK, ids=lambda c: 'f%d-p%d-h1_%d-h2_%d-lde%d' % c)
def test_ief_pack(dev, case):
    """w1f, w1e with its zero padding columns, w3 with exactly ceil(p / 32) * 32 rows of which rows >= p are +0.0: bit for bit"""
    f, p, h1, h2, ld_e = case
    fc1, fc3 = H.det((h1, f + p), 301), H.det((p, h2), 302)
    z = Zone(dev)
    got = _pack(dev, z, fc1, fc3, *case)
    for g, w_, name in zip(got, H.pack_reference(fc1, fc3, *case), ('w1f', 'w1e', 'w3')):
        assert tuple(g.shape) == tuple(w_.shape)
        _same_bits(g, w_, name)
    assert bool((H.bits(got[2][p:]) == 0).all()) and bool((H.bits(got[1][:, p:]) == 0).all())


@pytest.mark.parametrize('i', H.PACK_LINEAR)
def test_pack_feeds_linear(dev, i):
    """the two contracts against each other: the w3 straps_ief_pack writes (zero rows up to a multiple of 32) as the weight of straps_linear_fwd, with
    tracer data -- the kernel reads rows n .. n_pad - 1 of w unclamped, so a pack that left them unwritten would put NaN into the last tile"""
    f, p, h1, h2, ld_e = H.PACK[i]
    L = hipabi.lib()
    fc1, fc3 = H.tracer((h1, f + p), 311), H.tracer((p, h2), 312)
    z = Zone(dev)
    _, _, w3 = _pack(dev, z, fc1, fc3, f, p, h1, h2, ld_e)
    m = 33
    x, bias = H.tracer((m, h2), 313), H.tracer((p,), 314)
    out = z.guarded((m, 160), name='out')
    hipabi.check(L.straps_linear_fwd(P(z.at_end(x)), h2, P(w3), h2, P(z.at_end(bias)), None, P(out), 160, m, p, h2, 0, None), 'straps_linear_fwd')
    z.check()
    got = _split(out, p, 'linear on the packed w3')
    assert torch.equal(got.double(), x.double() @ fc3.double().t() + bias.double())


@pytest.mark.parametrize('cols,ld_dst,m', H.BROADCAST)
def test_broadcast_rows(dev, cols, ld_dst, m):
    L = hipabi.lib()
    row = H.det((cols,), 321)
    z = Zone(dev)
    dst = z.guarded((m, ld_dst), name='dst')
    hipabi.check(L.straps_broadcast_rows(P(z.at_end(row)), cols, P(dst), ld_dst, m, None), 'straps_broadcast_rows')
    z.check()
    want = torch.zeros(m, ld_dst)
    want[:, :cols] = row
    _same_bits(dst, want, 'broadcast_rows')
