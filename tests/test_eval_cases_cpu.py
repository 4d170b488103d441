"""CPU: the on-device evaluation without a GPU -- the float64 restatement of the aligned points (tests/eval_cases.py) reproduces what the
reference's EvalMetricsTracker computed (tests/golden/eval_metrics_golden.npz, written by tools/make_eval_metrics_golden.py); a numpy
emulation of the KERNEL's algorithm agrees with it, N = 3 included; the golden's silhouette numbers are a three-line numpy count; the mask
restatement gives the hand-counted masks; the three new entries are exported, bound, and check their arguments before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import eval_cases as EC
import straps_amd
from straps_amd import hipabi

EINVAL = 1


@pytest.fixture(scope='module')
def gold():
    return np.load(EC.GOLD)


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


# ---- points ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', EC.POINT_CASES)
def test_restatement_reproduces_the_references_aligned_points(gold, name):
    """aligned points to 1e-12, sums to 1e-10 (absolute; coordinates are O(1), sums up to a few hundred)"""
    s = EC.check_point_case(name)
    assert 0.05 <= (s[:, 1] / s[:, 0]).min() <= 1.0
    pred, target = EC.point_case(name)
    sums, sc, pa = EC.aligned_points64(pred, target)
    idx = gold['%s_idx' % name]
    assert np.abs(sc[:, idx] - gold['%s_sc' % name]).max() <= 1e-12
    assert np.abs(pa[:, idx] - gold['%s_pa' % name]).max() <= 1e-12
    assert np.abs(sums - gold['%s_sums' % name]).max() <= 1e-10


def test_point_case_table_covers_what_it_promises():
    shapes = {EC.point_case(n)[0].shape[:2] for n in EC.POINT_CASES}
    assert {s[0] for s in shapes} == {1, 3} and {s[1] for s in shapes} == {4, 14, 255, 256, 257, 6890}
    p, t = EC.point_case('hand_identical')
    assert np.array_equal(p, t)
    p, t = EC.point_case('hand_flat_pred')
    assert np.ptp(p[:, :, 2]) == 0
    s = EC.check_point_case('hand_flat_pred')
    assert (s[:, 2] / s[:, 0]).max() < 1e-12                          # rank 2
    p, t = EC.point_case('hand_mirrored')
    X1, X2 = (p[0] - p[0].mean(0)).astype(np.float64), (t[0] - t[0].mean(0)).astype(np.float64)
    U, _, Vh = np.linalg.svd(X1.T.dot(X2))
    assert np.linalg.det(U.dot(Vh)) < 0                               # the reflection fix is exercised
    sums, _, _ = EC.aligned_points64(*EC.point_case('hand_similarity'))
    assert sums[:, 2].max() < 1e-5 < sums[:, 1].min()                 # aligned error = the target's float32 rounding only


@pytest.mark.parametrize('name', EC.POINT_CASES)
def test_kernel_algorithm_emulated_in_float64_agrees_with_the_reference(name):
    """the kernel's route to the rotation (Jacobi on K^T K, u_i = K v_i, cross-product completion) against the reference's SVD route: the
    emulation, rounded once to float32 as the kernel rounds, stays within 1 fp32 ulp of the frame's largest coordinate"""
    pred, target = EC.point_case(name)
    sums, sc, pa = EC.aligned_points64(pred, target)
    ks, ksc, kpa = EC.kernel_emulation64(pred, target)
    for got, want in ((ksc, sc), (kpa, pa)):
        err = np.abs(got.astype(np.float32).astype(np.float64) - want).reshape(len(want), -1).max(1)
        assert (err <= EC.ulp32_of_largest(want)).all(), (name, err / EC.ulp32_of_largest(want))
    EC.assert_sums_close(ks, sums, name, pred, target)


def test_kernel_algorithm_at_the_conditioning_limit_the_header_states():
    """include/straps_hip.h: the aligned points stay within one fp32 ulp of the SVD route while sigma2 / sigma1 >= 5e-5.  The eigenvectors
    of K^T K carry an error of about eps64 * (sigma1 / sigma2)^2 = 1.1e-16 * 4e8 = 4.4e-8 of a unit vector there, below fp32's 2^-24 =
    6e-8; the emulation is asserted against that bound on points squeezed towards a line, and on the way there."""
    for eps in (0.3, 0.05, 8e-3):
        pred, target = EC.near_collinear_case(eps)
        s = EC.cross_covariance_singular_values(pred, target)
        ratio = s[:, 1] / s[:, 0]
        assert (ratio >= 4.5e-5).all() and (eps > 8e-3 or (ratio <= 7e-5).all()), (eps, ratio)
        _, sc, pa = EC.aligned_points64(pred, target)
        _, ksc, kpa = EC.kernel_emulation64(pred, target)
        for got, want in ((ksc, sc), (kpa, pa)):
            ulps = np.abs(got - want).reshape(3, -1).max(1) / EC.ulp32_of_largest(want)
            print('eps %g sigma2/sigma1 %s: %s fp32 ulp' % (eps, ratio, ulps))
            assert (ulps <= 1.0).all(), (eps, ratio, ulps)


def test_three_points_need_no_special_path():
    """N = 3: three centred points give a rank-2 cross-covariance in BOTH sets (sigma3 = 0 up to rounding).  The kernel's construction never
    divides by sigma3 -- the third singular pair is the cross product of the first two -- and its emulation agrees with the reference's SVD
    to 1e-12 on twenty deterministic triangles whose second singular value is not itself negligible."""
    from detgen import det_metrics_case
    seen = 0
    for seed in range(300, 320):
        pred, target = det_metrics_case(3, seed, batch=3)
        s = EC.cross_covariance_singular_values(pred, target)
        assert (s[:, 2] / s[:, 0]).max() < 1e-14
        if (s[:, 1] / s[:, 0]).min() < 1e-3:
            continue
        seen += 1
        sums, sc, pa = EC.aligned_points64(pred, target)
        ks, ksc, kpa = EC.kernel_emulation64(pred, target)
        assert np.abs(ksc - sc).max() <= 1e-12 and np.abs(kpa - pa).max() <= 1e-12 and np.abs(ks - sums).max() <= 1e-12, seed
    assert seen >= 15


# ---- silhouette numbers ------------------------------------------------------------------------------------------------------------
def test_golden_silhouette_numbers_are_a_numpy_count(gold):
    c = np.concatenate([EC.counts_numpy(p['silhouettes'], t['silhouettes']) for p, t, _ in EC.tracker_batches()])
    keys = ('num_true_positives', 'num_false_positives', 'num_true_negatives', 'num_false_negatives')
    assert [int(gold['sum_%s' % k]) for k in keys] == c.sum(0).tolist()
    with np.errstate(invalid='ignore'):
        iou = c[:, 0] / (c[:, 0] + c[:, 1] + c[:, 3])
    assert np.isnan(iou[1]) and np.array_equal(np.isnan(iou), np.isnan(gold['frame_silhouette_ious']))
    assert np.array_equal(iou[~np.isnan(iou)], gold['frame_silhouette_ious'][~np.isnan(iou)])
    assert float(gold['final_silhouette_ious']) == c[:, 0].sum() / (c[:, 0].sum() + c[:, 1].sum() + c[:, 3].sum())
    assert c.sum(1).tolist() == [EC.TRACKER_SIL_WH ** 2] * 5


def test_golden_lists_the_references_files_and_keys(gold):
    assert sorted(gold['frame_files'].tolist()) == sorted('%s_per_frame.npy' % m for m in EC.PER_FRAME_METRICS)
    assert gold['returned_keys'].tolist() == ['pred_joints3D_h36mlsp_pa', 'pred_joints3D_h36mlsp_sc', 'pred_reposed_vertices_sc', 'pred_vertices_pa',
                                              'pred_vertices_sc']
    assert len(EC.ALL_METRICS) == 13 and set(EC.ALL_METRICS) - set(EC.REFERENCE_METRICS) == {'pve-ts_pa'}
    assert tuple(straps_amd.metrics.EvalMetricsTracker.METRICS) == EC.ALL_METRICS
    for m in EC.ALL_METRICS:
        if m != 'silhouette_ious':
            want = [v for k, v in EC.DIVISORS.items() if k in m]
            assert [straps_amd.metrics.EvalMetricsTracker.num_per_sample(m)] == want, m


# ---- mask restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(EC.hand_mesh_cases()))
def test_mask_restatement_on_hand_counted_cases(name):
    verts, faces, cam, want = EC.hand_mesh_cases(16)[name]
    got = EC.wp_silhouette(verts, faces, cam, 16)
    assert got.dtype == np.uint8 and np.array_equal(got, want), name
    if name == 'right_triangle':
        assert int(got.sum()) == 45 and got[0, 2, 2] == 1 and got[0, 2, 10] == 1 and got[0, 10, 2] == 1 and got[0, 6, 6] == 1 and got[0, 6, 7] == 0


def test_mask_restatement_pixel_convention_and_clipping():
    """rows run with +v, columns with +u, no flip; a camera scales about the origin after the shift; border faces reach the border"""
    v = EC._tri_verts(16, [(12, 1), (14, 1), (12, 3)])                  # right of centre, near the TOP rows
    m = EC.wp_silhouette(v, np.array([[0, 1, 2]], np.int32), EC.IDENTITY_CAM, 16)[0]
    rows, cols = np.nonzero(m)
    assert rows.min() == 1 and rows.max() == 3 and cols.min() == 12 and cols.max() == 14
    half = EC.wp_silhouette(v, np.array([[0, 1, 2]], np.int32), np.array([[0.5, 0.0, 0.0]], np.float32), 16)[0]
    rows, cols = np.nonzero(half)
    assert rows.min() >= 4 and cols.max() <= 11                          # pulled towards the centre
    verts, faces = EC.border_mesh()
    for wh in (16, 20, 256):
        m = EC.wp_silhouette(verts, faces, EC.IDENTITY_CAM, wh)[0]
        assert m[:, 0].any() and m[:, -1].any() and m[0].any() and m[-1].any() and m[-1, -1] == 1 and not m[0, 0], wh
    verts, faces, cams = EC.camera_batch_case()
    m = EC.wp_silhouette(verts, faces, cams, 20)
    frac = m.reshape(3, -1).mean(1)
    assert frac[0] < frac[1] < frac[2] and (m[2, 0].any() or m[2, -1].any() or m[2, :, 0].any() or m[2, :, -1].any())      # s = 2.5 leaves the image


# ---- the library, without a GPU ----------------------------------------------------------------------------------------------------
def test_symbols_exported_and_bound(lib):
    assert 'eval.hip' in hipabi.SOURCES
    for n in ('straps_point_align', 'straps_silhouette_counts', 'straps_wp_silhouette', 'straps_wp_silhouette_workspace_bytes'):
        assert hasattr(lib, n) and n in hipabi.SIGNATURES, n
    assert lib.straps_abi_version() == 12
    assert all(hasattr(straps_amd, n) for n in ('EvalMetricsTracker', 'WeakPerspectiveSilhouetteRenderer'))
    assert all(hasattr(straps_amd.metrics, n) for n in ('aligned_points', 'silhouette_counts', 'EvalMetricsTracker'))


def test_workspace_formula(lib):
    ws = lib.straps_wp_silhouette_workspace_bytes
    assert ws(64, 6890) == 64 * 6890 * 2 * 4 and ws(1, 1) == 8 and ws(3, 49) == 3 * 49 * 8
    assert ws(0, 6890) == 0 and ws(4, 0) == 0 and ws(-1, 5) == 0
    assert ws(1 << 20, 6890) == (1 << 20) * 6890 * 8                     # 64-bit arithmetic


def test_argument_validation_without_gpu(lib):
    """every failure returns STRAPS_EINVAL before any HIP call (the pointers are never dereferenced) and names the argument"""
    err = lambda: lib.straps_last_error().decode()
    p = lambda v: C.c_void_p(v)
    A = 8192

    def align(pred=A, target=A, out3=A, sc=A, pa=A, batch=2, n=14):
        return lib.straps_point_align(p(pred), p(target), p(out3), p(sc), p(pa), batch, n, None)
    assert align(pred=None) == EINVAL and '`pred`' in err() and 'null pointer' in err()
    assert align(target=None) == EINVAL and '`target`' in err()
    assert align(out3=None, sc=None, pa=None) == EINVAL and '`out3`' in err() and '`pred_pa`' in err()
    for batch in (0, -1, 1 << 31):
        assert align(batch=batch) == EINVAL and '`batch`' in err(), batch
    for n in (2, 0, -5, 0x7fffffff // 3 + 1):
        assert align(n=n) == EINVAL and '`npoints`' in err(), n

    def counts(pred=A, target=A, c=A, batch=2, npix=65536):
        return lib.straps_silhouette_counts(p(pred), p(target), p(c), batch, npix, None)
    for name, text in (('pred', 'pred'), ('target', 'target'), ('c', 'counts4')):
        assert counts(**{name: None}) == EINVAL and '`%s`' % text in err() and 'null pointer' in err(), name
    for batch in (0, -3):
        assert counts(batch=batch) == EINVAL and '`batch`' in err()
    for npix in (0, -1, 1 << 31, 1 << 40):
        assert counts(npix=npix) == EINVAL and '`npix`' in err(), npix
    assert counts(batch=1 << 31, npix=16385) == EINVAL and 'grid limit' in err()

    def sil(verts=A, faces=A, cam=A, mask=A, ws=A, batch=2, nv=6890, nf=13776, wh=256):
        return lib.straps_wp_silhouette(p(verts), p(faces), p(cam), p(mask), p(ws), batch, nv, nf, wh, None)
    for name, text in (('verts', 'verts'), ('faces', 'faces'), ('cam', 'cam_wp'), ('mask', 'mask'), ('ws', 'workspace')):
        assert sil(**{name: None}) == EINVAL and '`%s`' % text in err() and 'null pointer' in err(), name
    assert sil(ws=A + 2) == EINVAL and '`workspace`' in err() and 'aligned' in err()
    for wh in (0, -1, 4097):
        assert sil(wh=wh) == EINVAL and '`wh`' in err(), wh
    for kw in ({'batch': 0}, {'nv': 0}, {'nf': 0}, {'batch': -2}):
        assert sil(**kw) == EINVAL and '`batch`' in err(), kw
    assert sil(batch=1 << 36) == EINVAL and 'too large' in err()
    assert sil(batch=1, nf=0x7fffffff // 3 + 1) == EINVAL and '`nfaces`' in err()
