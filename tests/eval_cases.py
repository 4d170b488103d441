"""On-device evaluation (straps_point_align, straps_silhouette_counts, straps_wp_silhouette, metrics.EvalMetricsTracker): deterministic case
tables and the numpy restatements the CPU and GPU tests compare against.

  * point cases           : (pred, target) float32 [B,N,3] from detgen.det_metrics_case plus four hand-made ones; every case is checked here,
                            on the CPU, for the conditioning that makes its aligned points well defined (check_point_case).
  * aligned_points64      : float64 restatement of the kernel's three sums and two transformed point sets, through the oracle's helpers.
  * kernel_emulation64    : the KERNEL's algorithm (sums, Jacobi on K^T K, cross-product completion) in numpy float64 -- what showed that
                            N = 3 needs no special path.
  * wp_silhouette         : float32 restatement of straps_wp_silhouette, unfused, in csrc/eval.hip's order, with a per-face loop.
  * mesh cases            : hand-made meshes + cameras for the mask tests, with hand-counted masks where the test counts by hand.
  * tracker_batches       : the two batches tools/make_eval_metrics_golden.py feeds the reference's EvalMetricsTracker.
No GPU, no torch."""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, 'oracle') not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, 'oracle'))
import straps_oracle as O                      # noqa: E402
from detgen import det_metrics_case, det_uniform      # noqa: E402

GOLD = os.path.join(_ROOT, 'tests', 'golden', 'eval_metrics_golden.npz')
F32 = np.float32

# --------------------------------------------------------------------------------------------------------------------------------
# point cases
# --------------------------------------------------------------------------------------------------------------------------------
# name -> (batch, npoints, seed): detgen.det_metrics_case.  N sits around the kernel's 256-thread stride; 4 is the smallest compared size.
DET_POINT_CASES = {
    'det_b3_n4': (3, 4, 410), 'det_b1_n4': (1, 4, 411), 'det_b3_n14': (3, 14, 72), 'det_b1_n14': (1, 14, 73),
    'det_b3_n255': (3, 255, 255), 'det_b1_n256': (1, 256, 256), 'det_b3_n256': (3, 256, 2560), 'det_b3_n257': (3, 257, 257),
    'det_b3_n6890': (3, 6890, 70), 'det_b1_n6890': (1, 6890, 71),
}
HAND_POINT_CASES = ('hand_identical', 'hand_similarity', 'hand_flat_pred', 'hand_mirrored')
POINT_CASES = tuple(sorted(DET_POINT_CASES)) + HAND_POINT_CASES
GOLD_STRIDE = 13                # the golden keeps every 13th aligned point of a 6890-point case (file size); smaller cases whole


def _hand_base(seed, batch=3):
    """[batch,14,3] float64 points with an anisotropic spread (1 : 0.7 : 0.45): three well separated singular values"""
    return det_uniform((batch, 14, 3), seed, -1.0, 1.0).astype(np.float64) * np.array([1.0, 0.7, 0.45])


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K.dot(K)


def point_case(name):
    """-> (pred, target) float32 [B,N,3]"""
    if name in DET_POINT_CASES:
        b, n, seed = DET_POINT_CASES[name]
        return det_metrics_case(n, seed, batch=b)
    if name == 'hand_identical':                      # pred == target
        p = _hand_base(500).astype(F32)
        return p, p.copy()
    if name == 'hand_similarity':                     # target an exact similarity copy of pred (up to its rounding to float32)
        p = _hand_base(510).astype(F32)
        t = 1.7 * p.astype(np.float64).dot(_rot([1.0, 2.0, -0.5], 0.9).T) + np.array([0.3, -0.2, 0.15])
        return p, t.astype(F32)
    if name == 'hand_flat_pred':                      # pred flattened to a plane: a rank-2 cross-covariance
        t = _hand_base(520)
        p = t.dot(_rot([0.2, 1.0, 0.1], 0.5).T) + 0.02 * det_uniform((3, 14, 3), 521).astype(np.float64)
        p[:, :, 2] = 0.25
        return p.astype(F32), t.astype(F32)
    if name == 'hand_mirrored':                       # target mirrored in z, plus 2 cm of noise: det(U V^T) = -1, the Z fix decides
        p = _hand_base(530)
        t = p * np.array([1.0, 1.0, -1.0]) + 0.02 * det_uniform((3, 14, 3), 531).astype(np.float64)
        return p.astype(F32), t.astype(F32)
    raise KeyError(name)


def near_collinear_case(eps, seed=700):
    """[3,14,3] float32 points squeezed towards a line (spread 1 : eps : eps / 2) and a noisy similarity copy: sigma2 / sigma1 of the
    cross-covariance is about 0.8 eps^2.  Not a GPU case (it breaks the condition every compared point case asserts): it probes, on the
    CPU, where the kernel's route to the rotation loses precision."""
    p = det_uniform((3, 14, 3), seed, -1.0, 1.0).astype(np.float64) * np.array([1.0, eps, 0.5 * eps])
    t = 1.3 * p.dot(_rot([1.0, 2.0, -0.5], 0.9).T) + np.array([0.3, -0.2, 0.15]) + 0.1 * eps * det_uniform((3, 14, 3), seed + 1).astype(np.float64)
    return p.astype(F32), t.astype(F32)


def cross_covariance_singular_values(pred, target):
    """[B,3] singular values (descending) of K = X1 X2^T per sample, float64"""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    out = []
    for b in range(p.shape[0]):
        X1, X2 = (p[b] - p[b].mean(0)).T, (t[b] - t[b].mean(0)).T
        out.append(np.linalg.svd(X1.dot(X2.T), compute_uv=False))
    return np.stack(out)


def check_point_case(name):
    """the conditions under which the aligned points are well defined: sigma2 / sigma1 >= 0.05 (the two leading singular pairs fix the
    rotation), and for the mirrored case (sigma2 - sigma3) / sigma1 >= 0.02 (WHICH singular vector the reflection fix flips is then
    not in doubt).  -> the [B,3] singular values."""
    pred, target = point_case(name)
    assert pred.dtype == F32 and target.dtype == F32 and pred.shape == target.shape and pred.shape[2] == 3
    s = cross_covariance_singular_values(pred, target)
    assert (s[:, 1] / s[:, 0] >= 0.05).all(), (name, s)
    if name == 'hand_mirrored':
        assert ((s[:, 1] - s[:, 2]) / s[:, 0] >= 0.02).all(), (name, s)
    return s


def aligned_points64(pred, target):
    """float64 restatement: -> (sums [B,3], pred_sc [B,N,3], pred_pa [B,N,3]) of float32 inputs taken to float64"""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    sc = O.scale_and_translation_transform(p, t)
    pa = np.stack([O.similarity_transform(p[i], t[i]) for i in range(p.shape[0])])
    sums = np.stack([np.linalg.norm(p - t, axis=-1).sum(1), np.linalg.norm(sc - t, axis=-1).sum(1), np.linalg.norm(pa - t, axis=-1).sum(1)], axis=1)
    return sums, sc, pa


def _jacobi_eig3(A):
    """csrc/metrics.hip::jacobi_eig3, statement for statement"""
    A = A.copy()
    V = np.eye(3)
    for _ in range(16):
        off = A[0, 1] * A[0, 1] + A[0, 2] * A[0, 2] + A[1, 2] * A[1, 2]
        if off < 1e-300:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if abs(A[p, q]) < 1e-300:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                with np.errstate(over='ignore'):      # (a huge theta squares to inf: t = 0, the rotation is the identity -- as on the GPU)
                    t2 = theta * theta
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(t2 + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    akp, akq = A[k, p], A[k, q]
                    A[k, p], A[k, q] = c * akp - s * akq, s * akp + c * akq
                for k in range(3):
                    apk, aqk = A[p, k], A[q, k]
                    A[p, k], A[q, k] = c * apk - s * aqk, s * apk + c * aqk
                for k in range(3):
                    vkp, vkq = V[k, p], V[k, q]
                    V[k, p], V[k, q] = c * vkp - s * vkq, s * vkp + c * vkq
    return A, V


def kernel_emulation64(pred, target):
    """point_metrics_kernel's algorithm in numpy float64 (its sums are taken in numpy's order, not the kernel's: last-bit differences):
    raw moment sums -> means, variances, K = X1 X2^T; Jacobi eigenvectors of K^T K; u_i = K v_i orthonormalised; third pair by cross
    products; R = sum v_i u_i^T; scale = tr(R K) / var1.  -> (sums [B,3], pred_sc, pred_pa) float64"""
    P, T = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    B, N = P.shape[0], P.shape[1]
    sums, SC, PA = np.zeros((B, 3)), np.zeros_like(P), np.zeros_like(P)
    for b in range(B):
        x, y = P[b], T[b]
        n = float(N)
        mu1, mu2 = x.sum(0) / n, y.sum(0) / n
        var1 = (x * x).sum() - n * mu1.dot(mu1)
        var2 = (y * y).sum() - n * mu2.dot(mu2)
        K = x.T.dot(y) - n * np.outer(mu1, mu2)
        A, V = _jacobi_eig3(K.T.dot(K))
        o = [0, 1, 2]
        if A[o[0], o[0]] < A[o[1], o[1]]:
            o[0], o[1] = o[1], o[0]
        if A[o[0], o[0]] < A[o[2], o[2]]:
            o[0], o[2] = o[2], o[0]
        if A[o[1], o[1]] < A[o[2], o[2]]:
            o[1], o[2] = o[2], o[1]
        v1, v2 = V[:, o[0]], V[:, o[1]]
        v3 = np.cross(v1, v2)
        u1, u2 = K.dot(v1), K.dot(v2)
        l1 = np.sqrt(u1.dot(u1))
        u1 = u1 / (l1 if l1 > 0 else 1.0)
        u2 = u2 - u1.dot(u2) * u1
        l2 = np.sqrt(u2.dot(u2))
        u2 = u2 / (l2 if l2 > 0 else 1.0)
        u3 = np.cross(u1, u2)
        R = np.outer(v1, u1) + np.outer(v2, u2) + np.outer(v3, u3)
        scale = np.trace(R.dot(K)) / var1
        t = mu2 - scale * R.dot(mu1)
        ratio = np.sqrt(var2 / n) / np.sqrt(var1 / n)
        SC[b] = (x - mu1) * ratio + mu2
        PA[b] = scale * x.dot(R.T) + t
        sums[b] = [np.linalg.norm(x - y, axis=-1).sum(), np.linalg.norm(SC[b] - y, axis=-1).sum(), np.linalg.norm(PA[b] - y, axis=-1).sum()]
    return sums, SC, PA


def ulp32_of_largest(a):
    """[B] float64: one fp32 ulp at each frame's largest |coordinate| of a [B,N,3] array"""
    m = np.abs(np.asarray(a, np.float64)).reshape(a.shape[0], -1).max(1)
    return np.spacing(m.astype(F32)).astype(np.float64)


def sums_atol(name, pred, target):
    """[3] absolute floor beside the rtol of 5e-5 on the three error sums of point case `name`: ZERO -- the plain rtol -- except for the
    sums that are zero by construction: all three of 'hand_identical' (pred == target) and the aligned one of 'hand_similarity' (an exact
    similarity copy, up to the target's rounding to float32).  Such a sum is float64 rounding noise in the kernel and in the restatement
    alike, and two noises do not agree to a relative bound.  Each of the N point errors carries at most a few hundred float64 roundings of
    values no larger than the largest coordinate: N * 2^-40 * max|coordinate| is about 4 000 float64 roundings per point -- and nine
    orders of magnitude below what fp32 sums of these cases (0.1 .. 1e3) resolve."""
    floor = pred.shape[1] * 2.0 ** -40 * float(max(np.abs(pred).max(), np.abs(target).max()))
    zero_columns = {'hand_identical': (0, 1, 2), 'hand_similarity': (2,)}.get(name, ())
    atol = np.zeros(3)
    atol[list(zero_columns)] = floor
    return atol


def assert_sums_close(got, want, name, pred, target):
    """[B,3] error sums against the float64 restatement: rtol 5e-5, plus sums_atol's floor in the columns that are zero by construction"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = 5e-5 * np.abs(want) + sums_atol(name, pred, target)[None]
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all(), (name, got, want, np.abs(got - want) / np.maximum(np.abs(want), 1e-300))


# --------------------------------------------------------------------------------------------------------------------------------
# weak-perspective silhouette: restatement + mesh cases
# --------------------------------------------------------------------------------------------------------------------------------
def wp_silhouette(verts, faces, cam_wp, wh):
    """straps_wp_silhouette in numpy float32, unfused, in csrc/eval.hip's order; per-face Python loop: small cases.
    verts [B,N,3], faces [F,3] int, cam_wp [B,3] -> uint8 [B,wh,wh]"""
    verts = np.asarray(verts, F32)
    faces = np.asarray(faces, np.int64)
    cam = np.asarray(cam_wp, F32)
    B, N = verts.shape[0], verts.shape[1]
    fw = F32(wh)
    mask = np.zeros((B, wh, wh), np.uint8)
    sample = ((2 * np.arange(wh) + 1 - wh).astype(F32)) / fw
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(B):
            U = cam[b, 0] * (verts[b, :, 0] + cam[b, 1])
            V = cam[b, 0] * (verts[b, :, 1] + cam[b, 2])
            for f in range(faces.shape[0]):
                i0, i1, i2 = faces[f]
                if not (0 <= i0 < N and 0 <= i1 < N and 0 <= i2 < N):
                    continue
                x0, y0, x1, y1, x2, y2 = U[i0], V[i0], U[i1], V[i1], U[i2], V[i2]
                area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
                if not (abs(area) > F32(1e-12)):
                    continue
                xmin, xmax, ymin, ymax = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)
                if not (xmax >= -1 and xmin <= 1 and ymax >= -1 and ymin <= 1):
                    continue
                xa = max(int(np.floor((max(xmin, F32(-1)) * fw + fw - F32(1)) * F32(0.5))), 0)
                xb = min(int(np.ceil((min(xmax, F32(1)) * fw + fw - F32(1)) * F32(0.5))), wh - 1)
                ya = max(int(np.floor((max(ymin, F32(-1)) * fw + fw - F32(1)) * F32(0.5))), 0)
                yb = min(int(np.ceil((min(ymax, F32(1)) * fw + fw - F32(1)) * F32(0.5))), wh - 1)
                if xb < xa or yb < ya:
                    continue
                xp = sample[None, xa:xb + 1]
                yp = sample[ya:yb + 1, None]
                e0 = (xp - x1) * (y2 - y1) - (yp - y1) * (x2 - x1)
                e1 = (xp - x2) * (y0 - y2) - (yp - y2) * (x0 - x2)
                e2 = (xp - x0) * (y1 - y0) - (yp - y0) * (x1 - x0)
                inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                mask[b, ya:yb + 1, xa:xb + 1] |= inside.astype(np.uint8)
    return mask


def centre(k, wh):
    """coordinate of pixel centre k (exact in float32 for the power-of-two sizes the hand-counted cases use)"""
    return (2 * k + 1 - wh) / float(wh)


IDENTITY_CAM = np.array([[1.0, 0.0, 0.0]], F32)


def _tri_verts(wh, pix):
    """three (col, row) pixel centres -> verts [1,3,3] with z = 0"""
    return np.array([[[centre(c, wh), centre(r, wh), 0.0] for c, r in pix]], F32)


def right_triangle_mask(wh=16):
    """hand count: corners at the pixel centres (col, row) = (2,2), (10,2), (2,10); every sample ON an edge counts: rows 2..10, row r holds
    columns 2 .. 12 - r: 9 + 8 + ... + 1 = 45 pixels"""
    m = np.zeros((wh, wh), np.uint8)
    for r in range(2, 11):
        m[r, 2:12 - r + 1] = 1
    assert int(m.sum()) == 45
    return m


def hand_mesh_cases(wh=16):
    """name -> (verts [1,N,3], faces [F,3] int32, cam [1,3], expected mask [1,wh,wh] or None): the wh = 16 cases counted by hand"""
    tri = _tri_verts(wh, [(2, 2), (10, 2), (2, 10)])
    empty = np.zeros((1, wh, wh), np.uint8)
    cases = {
        'right_triangle': (tri, np.array([[0, 1, 2]], np.int32), IDENTITY_CAM, right_triangle_mask(wh)[None]),
        'reversed_winding': (tri, np.array([[0, 2, 1]], np.int32), IDENTITY_CAM, right_triangle_mask(wh)[None]),
        'off_screen': (np.array([[[1.2, -0.5, 0.0], [3.0, -0.5, 0.0], [1.2, 0.9, 0.0]]], F32), np.array([[0, 1, 2]], np.int32), IDENTITY_CAM, empty),
        'degenerate': (np.array([[[-0.5, -0.5, 0.0], [0.0, 0.0, 1.0], [0.5, 0.5, 2.0]]], F32), np.array([[0, 1, 2], [0, 0, 1]], np.int32), IDENTITY_CAM, empty),
        'index_out_of_range': (tri, np.array([[0, 1, 3], [-1, 1, 2], [0, 2 ** 31 - 1, 2]], np.int32), IDENTITY_CAM, empty),
    }
    return cases


def border_mesh():
    """one face clipped at each of the four borders (left, right, top, bottom), one across a corner, and one wholly inside: verts [1,18,3]"""
    v = [(-1.4, -0.3), (-0.7, -0.1), (-1.1, 0.35),          # left
         (0.62, -0.2), (1.7, 0.05), (0.8, 0.4),             # right
         (-0.2, -1.5), (0.3, -0.72), (-0.35, -0.8),         # top (v < -1)
         (-0.1, 0.66), (0.45, 1.9), (0.2, 0.7),             # bottom
         (0.8, 0.8), (1.3, 0.9), (0.9, 1.4),                # corner
         (-0.31, -0.22), (0.27, -0.13), (0.02, 0.33)]       # inside
    verts = np.array([[[x, y, 0.1 * k] for k, (x, y) in enumerate(v)]], F32)
    faces = np.arange(18, dtype=np.int32).reshape(6, 3)
    return verts, faces


def blob_mesh(n=7, seed=77):
    """an n x n jittered grid (2 (n-1)^2 faces, both windings mixed) spanning about [-0.8, 0.8]^2: verts [1,n*n,3], faces"""
    g = np.linspace(-0.8, 0.8, n)
    xy = np.stack(np.meshgrid(g, g, indexing='xy'), -1).reshape(-1, 2) + 0.08 * det_uniform((n * n, 2), seed).astype(np.float64)
    verts = np.concatenate([xy, 0.3 * det_uniform((n * n, 1), seed + 1).astype(np.float64)], 1).astype(F32)[None]
    faces = []
    for r in range(n - 1):
        for c in range(n - 1):
            a, b, d, e = r * n + c, r * n + c + 1, (r + 1) * n + c, (r + 1) * n + c + 1
            faces += [[a, b, e], [a, d, e]] if (r + c) % 2 else [[a, b, d], [e, d, b]]
    return verts, np.array(faces, np.int32)


CAMERAS = np.array([[0.5, 0.3, -0.2], [0.9, -0.15, 0.1], [2.5, 0.55, 0.5]], F32)      # s in {0.5, 0.9, 2.5}: under the last, part of the mesh leaves the image


def camera_batch_case():
    """the blob mesh under the three cameras: verts [3,N,3] (the same mesh, a small per-body offset), faces, cam [3,3]"""
    verts, faces = blob_mesh()
    verts = np.concatenate([verts, verts + F32(0.01), verts - F32(0.02)], 0)
    return verts, faces, CAMERAS.copy()


# --------------------------------------------------------------------------------------------------------------------------------
# silhouette counts
# --------------------------------------------------------------------------------------------------------------------------------
def counts_numpy(pred, target):
    """the three-line numpy count: [B,...] masks (non-zero = foreground) -> int64 [B,4] = TP, FP, TN, FN"""
    p, t = np.asarray(pred).reshape(len(pred), -1) != 0, np.asarray(target).reshape(len(target), -1) != 0
    return np.stack([(p & t).sum(1), (p & ~t).sum(1), (~p & ~t).sum(1), (~p & t).sum(1)], axis=1).astype(np.int64)


def random_mask(shape, seed, density=0.4, values=(1,)):
    """uint8 mask: `density` of the bytes non-zero, the non-zero bytes cycling through `values`"""
    u = det_uniform(shape, seed, 0.0, 1.0)
    pick = (det_uniform(shape, seed + 1, 0.0, 1.0) * len(values)).astype(np.int64)
    return np.where(u < density, np.asarray(values, np.uint8)[pick], 0).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------------------
# tracker batches (the golden's inputs)
# --------------------------------------------------------------------------------------------------------------------------------
TRACKER_SIL_WH = 48
REFERENCE_METRICS = ('pves', 'pves_sc', 'pves_pa', 'pve-ts', 'pve-ts_sc', 'mpjpes', 'mpjpes_sc', 'mpjpes_pa', 'pose_mses', 'shape_mses', 'joints2D_l2es',
                     'silhouette_ious')                   # the twelve the reference can run; 'pve-ts_pa' raises KeyError there
ALL_METRICS = REFERENCE_METRICS[:5] + ('pve-ts_pa',) + REFERENCE_METRICS[5:]
PER_FRAME_METRICS = tuple(m for m in REFERENCE_METRICS if m not in ('pose_mses', 'shape_mses'))      # the ones the reference can save per frame
DIVISORS = {'pve': 6890, 'mpjpe': 14, 'joints2D': 17, 'shape_mse': 10, 'pose_mse': 216}


def tracker_batches():
    """-> [(pred_dict, target_dict, num_samples)] x 2 (3 frames, then 2), numpy float32 / uint8.  Frame 1 of the first batch has an empty
    union (both silhouettes empty): its per-frame IoU is 0 / 0."""
    out = []
    for k, B in enumerate((3, 2)):
        s = 900 + 40 * k
        pv, tv = det_metrics_case(6890, s, batch=B)
        pr, tr = det_metrics_case(6890, s + 2, batch=B)
        pj, tj = det_metrics_case(14, s + 4, batch=B)
        pred = {'verts': pv, 'reposed_verts': pr, 'joints3D': pj, 'joints2D': det_uniform((B, 17, 2), s + 6), 'shape_params': det_uniform((B, 10), s + 7, -2.0, 2.0),
                'pose_params_rot_matrices': det_uniform((B, 24, 3, 3), s + 8), 'silhouettes': random_mask((B, TRACKER_SIL_WH, TRACKER_SIL_WH), s + 9, 0.45)}
        target = {'verts': tv, 'reposed_verts': tr, 'joints3D': tj, 'joints2D': det_uniform((B, 17, 2), s + 16), 'shape_params': det_uniform((B, 10), s + 17, -2.0, 2.0),
                  'pose_params_rot_matrices': det_uniform((B, 24, 3, 3), s + 18), 'silhouettes': random_mask((B, TRACKER_SIL_WH, TRACKER_SIL_WH), s + 19, 0.5)}
        # blobs, so that prediction and label overlap like silhouettes do
        rr, cc = np.mgrid[0:TRACKER_SIL_WH, 0:TRACKER_SIL_WH]
        for b in range(B):
            pred['silhouettes'][b] |= (((rr - 22 - b) ** 2 + (cc - 20) ** 2) < 150).astype(np.uint8)
            target['silhouettes'][b] |= (((rr - 24) ** 2 + (cc - 23 + b) ** 2) < 170).astype(np.uint8)
        if k == 0:
            pred['silhouettes'][1] = 0
            target['silhouettes'][1] = 0
        out.append((pred, target, B))
    return out
