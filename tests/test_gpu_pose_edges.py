"""GPU: the rotation and projection kernels at their edges, behind redzones (tests/redzone.py) -- straps_rot6d_fwd / _bwd, straps_rodrigues_fwd,
straps_orthographic_project / _bwd, straps_perspective_project (csrc/pose.hip, rot6d_bwd_kernel of csrc/backward.hip) and straps_project_targets
(csrc/train.hip); cases, launch rules and float64 references are tests/head_cases.py, held together by tests/test_head_cases_cpu.py.

Common form: outputs from Zone.guarded (NaN-filled, exactly the advertised size; with ldd larger than the extent the columns outside the extent keep
the NaN fill bit for bit), operands from Zone.at_end with NaN in every column a kernel has no business reading (the rest of an estimate row around
the pose columns, the columns of a cam row beyond s, tx, ty), Zone.check() after every call, float64 references on the CPU from the same fp32
values, comparisons per element, per rotation or per body.

Bounds:
  * rot6d forward 2e-6 per element, |R^T R - I| <= 4e-6 and det > 0 per rotation; backward 2e-5 of the largest of a rotation's six float64 entries,
    per rotation -- the project's bars of test_rot6d_and_rodrigues and test_rot6d_backward; an fp32 evaluation of the same formula on the CPU reaches
    5.2e-7 and 2.8e-6 on this data (tests/test_head_cases_cpu.py prints them).  Worst error / bound seen on an MI355X: forward 0.152, orthogonality
    0.099, backward 0.091;
  * rot6d degenerate rows: see test_rot6d_degenerate;
  * rodrigues forward 2e-6 per element for every family of rows (see test_rodrigues_fwd for what was measured);
  * orthographic projection: at most 1 ulp from fl32(s * fl32(x + tx)) (worst seen: 0); its gradient: dpoints exact, dcam within
    (ceil(N / 256) + 12) 2^-24 sum |terms| per entry (worst seen 0.058);
  * perspective projection and project_targets: 4 times the worst error of the oracle evaluated in fp32 on the CPU, measured over the inputs of all
    cases (tests/test_head_cases_cpu.py: 3.164e-04 and 1.783e-04 pixels at coordinates of a few thousand); worst error / bound seen: 0.2500 and 0.2500 -- the kernel's worst element
    has exactly the error of the fp32 evaluation on the CPU.
"""
import ctypes as C

import pytest
import torch

import head_cases as H
import straps_amd  # noqa: F401
import straps_oracle as O
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
P = hipabi.ptr
NAN = float('nan')
NAN_BITS = H.bits(torch.full((1,), NAN))[0]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    lib = hipabi.load()
    import os
    assert os.path.abspath(lib._name) == os.path.abspath(hipabi.LIB_PATH), 'these tests run on the product library, not %s' % lib._name
    return torch.device('cuda:0')


def _at(t, off):
    return C.c_void_p(t.data_ptr() + 4 * off)


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_rot6d_fwd / straps_rot6d_bwd

def _rot6d_run(dev, x, g, rows, per, ld, ldd):
    """x [rows * per][6], g [rows * per][3][3] | None -> R [rows * per][3][3], dx6 [rows * per][6] | None (CPU).  The x6 rows live at their offset
    inside [rows][ld] rows of NaN; dx6 is a guarded [rows][ldd] whose columns outside the pose columns must keep the NaN fill"""
    L = hipabi.lib()
    z = Zone(dev)
    off, offd = H.rot6d_offset(ld), H.rot6d_offset(ldd)
    buf = torch.full((rows, ld), NAN)
    buf[:, off:off + 6 * per] = x.view(rows, 6 * per)
    xd = z.at_end(buf)
    R = z.guarded((rows * per, 3, 3), name='rotmats')
    hipabi.check(L.straps_rot6d_fwd(_at(xd, off), ld, per, P(R), rows, None), 'straps_rot6d_fwd')
    z.check()
    dx = None
    if g is not None:
        dbuf = z.guarded((rows, ldd), name='dx6')
        hipabi.check(L.straps_rot6d_bwd(_at(xd, off), ld, per, P(z.at_end(g)), _at(dbuf, offd), ldd, rows, None), 'straps_rot6d_bwd')
        z.check()
        d = dbuf.detach().cpu()
        outside = torch.ones(ldd, dtype=torch.bool)
        outside[offd:offd + 6 * per] = False
        assert bool((H.bits(d[:, outside]) == NAN_BITS).all()), 'rot6d_bwd wrote a column outside [0, 6 * per_row)'
        dx = d[:, offd:offd + 6 * per].reshape(rows * per, 6)
    return R.detach().cpu(), dx


@pytest.mark.parametrize('i', range(len(H.ROT6D)), ids=lambda i: 'rows%d-per%d-ld%d-ldd%d' % H.ROT6D[i])
def test_rot6d_well_conditioned(dev, i):
    rows, per, ld, ldd = H.ROT6D[i]
    x, _ = H.rot6d_well_conditioned(rows, per, H.ROT6D_SEEDS[i])
    g = H.det((rows * per, 3, 3), 16 + i)
    R, dx = _rot6d_run(dev, x, g, rows, per, ld, ldd)
    Rw, dxw = H.rot6d_autograd(x, g)
    H.check_ratio('rot6d_fwd', R, Rw, 2e-6)
    Rd = R.double()
    H.check_ratio('rot6d_fwd orthogonality', Rd.transpose(1, 2) @ Rd, torch.eye(3, dtype=torch.float64).expand_as(Rd), 4e-6)
    assert bool((torch.linalg.det(Rd) > 0).all())
    H.check_ratio('rot6d_bwd', dx, dxw, (2e-5 * dxw.abs().max(1, keepdim=True).values).expand_as(dxw))


def test_rot6d_degenerate(dev):
    """a1 = 0, a2 = 0, a2 = 2 a1 and a2 = a1 + 1e-7 e, against the float64 formula with its clamp_min(1e-12) (autograd of the oracle).

    Rows built on the coordinate axes with dyadic entries ('exact' in head_cases.rot6d_degenerate) reach the clamped branch in fp32 and in float64
    alike, and every intermediate up to the final division is exact: the forward must equal the float64 value exactly (a1 = 0: b1 = 0,
    b2 = a2 / |a2|, b3 = 0 x b2 = 0 -- the first and third column are zero, the second is not; a2 = 0 and collinear: b2 = b3 = 0), the backward is
    compared to 1e-5 of the float64 value per entry (the clamped branches give g / 1e-12 without the projection term, entries of 1e12).
    With u = 0 (or a1 = 0) exactly the clamped quotient is zero and the projection term vanishes whichever branch runs, so rows with
    0 < |u| <= 1e-12 and 0 < |a1| <= 1e-12 are added ('tiny-u', 'tiny-a1': b2 or b1 of length 1/2 or 1/4): there a kernel that took the projected branch
    would be wrong by a quarter of the gradient (the mutation check showed that the exact-zero rows alone do not see it).
    Rows in a generic direction are ill-conditioned -- u = a2 - (b1.a2) b1 is rounding noise, another noise in float64 -- so of them only what is
    well defined is asked: finite forward and backward, and b1 equal to the well-conditioned value (2e-6); for a1 = 0 and a2 = 0 in a generic
    direction additionally the forward (2e-6) and the backward to 1e-5 of the largest float64 entry of d a1 and of d a2 (one of the two is of the
    order 1e12, the other of 1)."""
    deg = H.rot6d_degenerate()
    n = len(deg)
    x = torch.stack([r for _, r, _ in deg])
    g = H.dyadic((n, 3, 3), 41)
    R, dx = _rot6d_run(dev, x, g, n, 1, 6, 6)
    Rw, dxw = H.rot6d_autograd(x, g)
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(dx).all())
    exact = torch.tensor([e is True for _, _, e in deg])
    bwd = torch.tensor([e is True or e == 'bwd' for _, _, e in deg])
    assert torch.equal(R[exact].double(), Rw[exact]), 'the forward of an exact degenerate row is not the float64 value'
    H.check_ratio('rot6d_fwd clamped', R[bwd], Rw[bwd], 2e-6)
    H.check_ratio('rot6d_bwd clamped', dx[bwd], dxw[bwd], 1e-5 * dxw[bwd].abs())
    a1 = x.double()[:, 0::2]
    for i, (kind, _, e) in enumerate(deg):
        if kind not in ('a1=0', 'tiny-a1'):
            assert float((R[i][:, 0].double() - a1[i] / a1[i].norm()).abs().max()) <= 2e-6, 'b1 of row %d' % i
        if e is False and kind in ('a1=0', 'a2=0'):
            assert float((R[i].double() - Rw[i]).abs().max()) <= 2e-6
            for half in (slice(0, 6, 2), slice(1, 6, 2)):          # d a1 and d a2 apart: one of them is of the order 1e12, the other of 1
                assert float((dx[i][half].double() - dxw[i][half]).abs().max()) <= 1e-5 * float(dxw[i][half].abs().max()), 'backward of row %d' % i
    print('RATIO rot6d_degenerate generic rows checked for finiteness and b1')


# ----------------------------------------------------------------------------------------------------------------------------------------
# straps_rodrigues_fwd

@pytest.mark.parametrize('n', H.RODRIGUES_N)
def test_rodrigues_fwd(dev, n):
    """2e-6 absolute per element against O.batch_rodrigues in float64, per family of rows: random in [-3, 3], one component 1e-4 or 1e-3 (the
    1 - cos cancellation), |r| = pi and 2 pi along an axis and along (1,1,1)/sqrt3, |r| = 10 and 50 (argument reduction of sinf / cosf), negative
    axes.  The zero row gives the identity exactly.  Rows whose three components are all within 1e-7 of -1e-8 are left out: angle = ||r + 1e-8||
    vanishes there and d = r / angle is singular, in the reference too (the zero row lies inside that neighbourhood and is the one marked
    exception: d = 0 / angle = 0 exactly).  An fp32 evaluation of the oracle on the CPU reaches 5.3e-7 on the random rows.
    Worst error / bound seen on an MI355X: random 0.179, small 0.012 (below 1/64: the bar is absolute and these entries are within 1e-3 of 0 or 1),
    pi 0.146, r10 0.090, r50 0.119: the |r| = 50 rows meet the bar (worst error 2.4e-7), so no family has a bound of its own."""
    L = hipabi.lib()
    aa, fam = H.rodrigues_rows(n)
    z = Zone(dev)
    R = z.guarded((n, 3, 3), name='rotmats')
    hipabi.check(L.straps_rodrigues_fwd(P(z.at_end(aa)), P(R), n, None), 'straps_rodrigues_fwd')
    z.check()
    R = R.detach().cpu()
    want = O.batch_rodrigues(aa.double())
    for f in sorted(set(fam)):
        sel = torch.tensor([x == f for x in fam])
        if f == 'zero':
            assert torch.equal(R[sel].double(), torch.eye(3, dtype=torch.float64)[None].expand(int(sel.sum()), 3, 3))
            continue
        assert not bool(H.rodrigues_excluded(aa[sel]).any())
        H.check_ratio('rodrigues_fwd[%s]' % f, R[sel], want[sel], 2e-6)


# ----------------------------------------------------------------------------------------------------------------------------------------
# projections

def _assert_ulps(got, want, n, what):
    assert bool(torch.isfinite(got).all()), '%s: not finite (an element nobody wrote, or a read past an operand)' % what
    d = (H.ordv(got) - H.ordv(want)).abs()
    worst = int(d.max()) if d.numel() else 0
    print('RATIO %s %d ulp' % (what, worst))
    assert worst <= n, '%s: %d ulp at flat index %d' % (what, worst, int(d.argmax()))


@pytest.mark.parametrize('B,N,ld_cam', H.ORTHO)
def test_orthographic_project(dev, B, N, ld_cam):
    L = hipabi.lib()
    pts, cam = H.det((B, N, 3), 500), H.cam_rows(B, ld_cam, 501)
    z = Zone(dev)
    out = z.guarded((B, N, 2), name='out')
    hipabi.check(L.straps_orthographic_project(P(z.at_end(pts)), P(z.at_end(cam)), ld_cam, P(out), B, N, None), 'straps_orthographic_project')
    z.check()
    _assert_ulps(out.detach().cpu(), H.ortho_reference(pts, cam), 1, 'orthographic_project')


@pytest.mark.parametrize('N', H.ORTHO_BWD_N)
def test_orthographic_project_bwd(dev, N):
    """both outputs, dpoints only, dcam only, for B in 1, 3 and ld_cam in 3, 160: shared outputs are bit-identical between the forms; dpoints is
    exact (fl32(s du), fl32(s dv), +0.0); dcam per entry within (ceil(N / 256) + 12) 2^-24 sum |terms|"""
    L = hipabi.lib()
    for B in H.ORTHO_BWD_B:
        for ld_cam in (3, 160):
            pts, cam, dout = H.det((B, N, 3), 510 + B), H.cam_rows(B, ld_cam, 520 + B), H.det((B, N, 2), 530 + B)
            dp_want, dcam_want, bound = H.ortho_bwd_reference(pts, cam, dout)
            res = {}
            for form in ('both', 'dpoints', 'dcam'):
                z = Zone(dev)
                dp = z.guarded((B, N, 3), name='dpoints') if form != 'dcam' else None
                dc = z.guarded((B, 3), name='dcam') if form != 'dpoints' else None
                hipabi.check(L.straps_orthographic_project_bwd(P(z.at_end(pts)), P(z.at_end(cam)), ld_cam, P(z.at_end(dout)), P(dp), P(dc), B, N, None),
                             'straps_orthographic_project_bwd')
                z.check()
                res[form] = (None if dp is None else H.bits(dp), None if dc is None else dc.detach().cpu())
            assert torch.equal(res['both'][0], res['dpoints'][0]) and torch.equal(H.bits(res['both'][1]), H.bits(res['dcam'][1]))
            assert torch.equal(res['both'][0], H.bits(dp_want)), 'dpoints is not (fl32(s du), fl32(s dv), +0.0)'
            H.check_ratio('orthographic_project_bwd dcam', res['both'][1], dcam_want, bound)


@pytest.mark.parametrize('B,N', H.PERSP)
@pytest.mark.parametrize('per_body', [0, 1])
def test_perspective_project(dev, B, N, per_body):
    """against O.perspective_project in float64.  The bound is measured, not derived: the worst per-element error of O.perspective_project evaluated
    in fp32 on the CPU against its float64 value over the inputs of all eight cases is 3.164e-04 (pixels; coordinates reach a few thousand at a focal
    length of 5000), and the kernel gets 4 times that for its different but equally valid operation order and contraction.
    Worst error / bound seen on an MI355X: 0.2500."""
    L = hipabi.lib()
    pts, rot, tr, K = H.persp_inputs(B, N, per_body)
    z = Zone(dev)
    out = z.guarded((B, N, 2), name='out')
    hipabi.check(L.straps_perspective_project(P(z.at_end(pts)), P(z.at_end(rot)), P(z.at_end(tr)), P(z.at_end(K)), per_body, P(out), B, N, None),
                 'straps_perspective_project')
    z.check()
    bound = 4 * H.persp_fp32_cpu_error()
    print('MEASURED perspective_project fp32 CPU evaluation %.3e' % (bound / 4))
    H.check_ratio('perspective_project', out, H.persp_eval(pts, rot, tr, K, torch.float64), bound)


@pytest.mark.parametrize('B', H.TARGETS_B)
def test_project_targets(dev, B):
    """joints3d is an exact copy of the H36M-to-LSP rows; joints2d against O.perspective_project in float64 (identity rotation, the oracle's
    intrinsics) within 4 times the worst error of its fp32 evaluation on the CPU over the inputs of all four cases (1.783e-04 pixels).
    Worst error / bound seen on an MI355X: 0.2500."""
    L = hipabi.lib()
    joints, cam_t = H.targets_inputs(B)
    z = Zone(dev)
    j2d, j3d = z.guarded((B, 17, 2), name='joints2d'), z.guarded((B, 14, 3), name='joints3d')
    hipabi.check(L.straps_project_targets(P(z.at_end(joints)), P(z.at_end(cam_t)), float(O.FOCAL_LENGTH), float(O.FOCAL_LENGTH), O.REGRESSOR_IMG_WH / 2.0,
                                          O.REGRESSOR_IMG_WH / 2.0, P(j2d), P(j3d), B, None), 'straps_project_targets')
    z.check()
    assert torch.equal(H.bits(j3d), H.bits(joints[:, H.H36M14])), 'joints3d is not a copy of the H36M-to-LSP rows'
    bound = 4 * H.targets_fp32_cpu_error()
    print('MEASURED project_targets fp32 CPU evaluation %.3e' % (bound / 4))
    H.check_ratio('project_targets joints2d', j2d, H.targets_eval(joints, cam_t, torch.float64), bound)
