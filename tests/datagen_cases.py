"""Data-generation kernels (straps_rasterize_parts, straps_crop_resize, straps_augment_seg, the two deviation kernels): the brute-force
definition of the part rasteriser, deterministic scene families that sit on its edges, and the crop / occlusion case tables the CPU and
GPU tests share.

  * rasterize_brute      : the algorithm oracle/straps_oracle.py::rasterize_parts STATES -- every pixel centre against every face -- in the
                           same unfused float32 arithmetic, without the per-face bounding box and cull that the oracle and csrc/raster.hip
                           both use.  The oracle and the kernel are the fast forms of this; a box that drops a covered sample is wrong in
                           both of them and only here not.
  * zero_edge_pairs      : how many (face, sample) pairs are inside with an edge function of exactly 0.0 (what `on_centre` is for).
  * scene families       : geometry built in PIXEL space (column, z-buffer row; the sample k sits at k + 0.5) and mapped back through
                           K = [[wh,0,wh/2],[0,wh,wh/2],[0,0,1]], R = I, t = 0 (`depth` translates by 0.5 in z).  Vertices meant to sit ON
                           a sample are snapped so that the float32 projection gives the sample's coordinate bit for bit.
  * crop_cases / seg_cases: silhouettes and part maps for the crop and the occlusion kernel.
Inputs come from detgen.det_uniform.  No GPU, no torch."""
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, 'oracle') not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, 'oracle'))
import straps_oracle as O                      # noqa: E402
from detgen import det_uniform                 # noqa: E402

F32 = np.float32
NEAR, FAR = 0.1, 100.0
RASTER_WH = (1, 2, 5, 33, 48, 64, 100)
RASTER_B = (1, 3)
FAMILIES = ('on_centre', 'slivers', 'tiny', 'huge', 'strips', 'depth', 'bad_indices')
LAST_DRAW = F32(1.0 - 2.0 ** -24)              # the largest value a 24-bit uniform draw takes


# --------------------------------------------------------------------------------------------------------------------------------
# the definition
# --------------------------------------------------------------------------------------------------------------------------------
def _project(verts, cam_K, cam_R, cam_t, wh):
    """-> (X, Y, zc) float32 [B,N]: oracle/straps_oracle.py::rasterize_parts' projection, statement for statement"""
    verts = np.asarray(verts, F32)
    B = verts.shape[0]
    K = np.broadcast_to(np.asarray(cam_K, F32), (B, 3, 3))
    R = np.broadcast_to(np.asarray(cam_R, F32), (B, 3, 3))
    t = np.asarray(cam_t, F32).reshape(B, 3)
    orig = F32(wh)
    half = orig / F32(2)
    X, Y, Z = np.zeros(verts.shape[:2], F32), np.zeros(verts.shape[:2], F32), np.zeros(verts.shape[:2], F32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for b in range(B):
            x, y, z = verts[b, :, 0], verts[b, :, 1], verts[b, :, 2]
            xc = ((R[b, 0, 0] * x + R[b, 0, 1] * y) + R[b, 0, 2] * z) + t[b, 0]
            yc = ((R[b, 1, 0] * x + R[b, 1, 1] * y) + R[b, 1, 2] * z) + t[b, 1]
            zc = ((R[b, 2, 0] * x + R[b, 2, 1] * y) + R[b, 2, 2] * z) + t[b, 2]
            den = zc + F32(1e-9)
            xn, yn = xc / den, yc / den
            u = (K[b, 0, 0] * xn + K[b, 0, 1] * yn) + K[b, 0, 2]
            v = orig - ((K[b, 1, 0] * xn + K[b, 1, 1] * yn) + K[b, 1, 2])
            X[b] = F32(2) * (u - half) / orig
            Y[b] = F32(2) * (v - half) / orig
            Z[b] = zc
    return X, Y, Z


def _face_tests(X, Y, faces, wh):
    """one body: -> (e0, e1, e2 [F,wh,wh], area [F,1,1], inside [F,wh,wh]) over the WHOLE sample grid; a degenerate (or NaN) face is inside nowhere"""
    sample = ((2 * np.arange(wh) + 1 - wh).astype(F32)) / F32(wh)
    xp, yp = sample[None, None, :], sample[None, :, None]
    c = lambda a, k: a[faces[:, k]][:, None, None]
    x0, y0, x1, y1, x2, y2 = c(X, 0), c(Y, 0), c(X, 1), c(Y, 1), c(X, 2), c(Y, 2)
    area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
    e0 = (xp - x1) * (y2 - y1) - (yp - y1) * (x2 - x1)
    e1 = (xp - x2) * (y0 - y2) - (yp - y2) * (x0 - x2)
    e2 = (xp - x0) * (y1 - y0) - (yp - y0) * (x1 - x0)
    inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
    inside &= np.abs(area) > F32(1e-12)
    return e0, e1, e2, area, inside


def rasterize_brute(verts, faces, face_parts, cam_K, cam_R, cam_t, wh, near=NEAR, far=FAR, return_depth=False, return_faces=False):
    """Arguments and returns of O.rasterize_parts (plus, with return_faces, the int64 [B,wh,wh] winning face ids, -1 = background, in the
    image's orientation).  Same float32 projection, edge functions, clamped and renormalised weights, depth, near / far test,
    first-face-on-ties rule and final flip -- and NO bounding box and NO cull: every face is tested at all wh x wh pixel centres."""
    faces = np.asarray(faces, np.int64)
    face_parts = np.asarray(face_parts)
    X, Y, Z = _project(verts, cam_K, cam_R, cam_t, wh)
    B = X.shape[0]
    assert faces.min() >= 0 and faces.max() < X.shape[1], 'rasterize_brute: face indices must be valid (see degenerate_bad_faces)'
    parts, depth, fids = np.zeros((B, wh, wh), F32), np.full((B, wh, wh), F32(far), F32), np.full((B, wh, wh), -1, np.int64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for b in range(B):
            e0, e1, e2, area, inside = _face_tests(X[b], Y[b], faces, wh)
            z0, z1, z2 = (Z[b][faces[:, k]][:, None, None] for k in range(3))
            w0 = np.minimum(np.maximum(e0 / area, F32(0)), F32(1))
            w1 = np.minimum(np.maximum(e1 / area, F32(0)), F32(1))
            w2 = np.minimum(np.maximum(e2 / area, F32(0)), F32(1))
            ws = (w0 + w1) + w2
            w0, w1, w2 = w0 / ws, w1 / ws, w2 / ws
            zp = F32(1) / ((w0 / z0 + w1 / z1) + w2 / z2)
            ok = inside & (zp > F32(near)) & (zp < F32(far))
            zp = np.where(ok, zp, F32(np.inf))
            fi = np.argmin(zp, axis=0)                                      # the first face among equal depths
            zmin = np.take_along_axis(zp, fi[None], 0)[0]
            hit = ok.any(axis=0)
            fids[b] = np.where(hit, fi, -1)[::-1]
            parts[b] = np.where(hit, face_parts[fi].astype(F32), F32(0))[::-1]
            depth[b] = np.where(hit, zmin, F32(far))[::-1]
    out = (parts,) + ((depth,) if return_depth else ()) + ((fids,) if return_faces else ())
    return out if len(out) > 1 else parts


def zero_edge_pairs(verts, faces, face_parts, cam_K, cam_R, cam_t, wh):
    """-> number of (body, face, sample) triples that are inside with at least one edge function exactly 0.0"""
    faces = np.asarray(faces, np.int64)
    X, Y, _ = _project(verts, cam_K, cam_R, cam_t, wh)
    n = 0
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(X.shape[0]):
            e0, e1, e2, _, inside = _face_tests(X[b], Y[b], faces, wh)
            n += int((inside & ((e0 == 0) | (e1 == 0) | (e2 == 0))).sum())
    return n


def coverage(verts, faces, cam_K, cam_R, cam_t, wh, body=0):
    """-> bool [F,wh,wh] in Z-BUFFER orientation (row k = sample k, before the final flip): the samples each face of `body` is inside,
    whatever its depth"""
    X, Y, _ = _project(verts, cam_K, cam_R, cam_t, wh)
    with np.errstate(invalid='ignore', over='ignore'):
        return _face_tests(X[body], Y[body], np.asarray(faces, np.int64), wh)[4]


def sample_boxes(verts, faces, cam_K, cam_R, cam_t, wh, body=0):
    """-> int [F,4] = xa, xb, ya, yb: the sample box the kernel and the oracle walk for each face of `body` (their shared formula; a culled
    or empty box is (0, -1, 0, -1)).  Only the CPU test uses it, to show that a scene has the box widths it was built for."""
    X, Y, _ = _project(verts, cam_K, cam_R, cam_t, wh)
    fw, out = F32(wh), []
    for i0, i1, i2 in np.asarray(faces, np.int64):
        xs, ys = (X[body, i0], X[body, i1], X[body, i2]), (Y[body, i0], Y[body, i1], Y[body, i2])
        xmin, xmax, ymin, ymax = min(xs), max(xs), min(ys), max(ys)
        if not (xmax >= -1 and xmin <= 1 and ymax >= -1 and ymin <= 1):
            out.append((0, -1, 0, -1))
            continue
        lo = lambda m: max(int(np.floor((max(m, F32(-1)) * fw + fw - F32(1)) * F32(0.5))), 0)
        hi = lambda m: min(int(np.ceil((min(m, F32(1)) * fw + fw - F32(1)) * F32(0.5))), wh - 1)
        box = (lo(xmin), hi(xmax), lo(ymin), hi(ymax))
        out.append(box if box[1] >= box[0] and box[3] >= box[2] else (0, -1, 0, -1))
    return np.array(out, np.int64)


# --------------------------------------------------------------------------------------------------------------------------------
# pixel space -> vertices
# --------------------------------------------------------------------------------------------------------------------------------
def pixel_camera(wh, B=1, t=(0.0, 0.0, 0.0)):
    """-> (K [3,3], R [3,3], t [B,3]) float32 of the scene builders"""
    K = np.array([[wh, 0, wh / 2.0], [0, wh, wh / 2.0], [0, 0, 1]], F32)
    return K, np.eye(3, dtype=F32), np.tile(np.asarray(t, F32)[None], (B, 1))


def _snapped(target, wh, flip):
    """normalised camera coordinates xn (float64 array `target` in pixels -> float32) whose float32 projection u = wh * xn + wh / 2 (v is
    then flipped: wh - v) lands as close to `target` as float32 allows -- EXACTLY on it wherever some neighbour of the rounded quotient does,
    which is every pixel centre of the sizes used here (asserted by the CPU test through zero_edge_pairs)"""
    target = np.asarray(target, np.float64)
    raw = (wh - target) if flip else target                                  # the value K's row has to produce
    xn = ((raw - wh / 2.0) / wh).astype(F32)
    fw, half = F32(wh), F32(wh / 2.0)
    best, err = xn.copy(), np.full(xn.shape, np.inf)
    for step in (0, 1, -1, 2, -2, 3, -3):
        cand = xn.copy()
        for _ in range(abs(step)):
            cand = np.nextafter(cand, F32(np.inf if step > 0 else -np.inf))
        got = (fw * cand + half).astype(np.float64)
        e = np.abs(got - raw)
        better = e < err
        best[better], err[better] = cand[better], e[better]
    return best


def verts_from_pixels(px, py, zc, wh, tz=0.0):
    """pixel coordinates (column px, z-buffer row py: sample k sits at k + 0.5) and camera depth zc -> float32 [...,3] vertices for
    pixel_camera(wh, t=(0,0,tz)).  With zc a power of two the products below are exact and a pixel centre projects onto its sample."""
    zc = np.asarray(zc, F32)
    xn, yn = _snapped(px, wh, False), _snapped(py, wh, True)
    return np.stack([xn * zc, yn * zc, zc - F32(tz)], -1).astype(F32)


def _ints(shape, seed, lo, hi):
    """integers uniform on [lo, hi)"""
    return np.minimum(np.floor(det_uniform(shape, seed, float(lo), float(hi))).astype(np.int64), hi - 1)


def _parts(F, seed):
    return (1 + _ints((F,), seed, 0, 6)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------------------
# scene families
# --------------------------------------------------------------------------------------------------------------------------------
def on_centre(wh, B, seed=100):
    """90 vertices AT pixel centres k + 0.5, k in [-2, wh + 2), z in {1, 2}; 121 random index triples: edges pass exactly through samples,
    vertices sit on and just outside the frame"""
    N, F = 90, 121
    k = _ints((B, N, 2), seed, -2, wh + 2)
    z = F32(1) + _ints((B, N), seed + 1, 0, 2).astype(F32)
    verts = verts_from_pixels(k[..., 0] + 0.5, k[..., 1] + 0.5, z, wh)
    faces = _ints((F, 3), seed + 2, 0, N).astype(np.int32)
    return (verts, faces, _parts(F, seed + 3)) + pixel_camera(wh, B)


def slivers(wh, B, seed=200):
    """61 faces of three own vertices each: the third lies on the segment between the first two, moved by at most 0.02 px in each axis.
    Every second face has its two end points on pixel centres, so that its long edges run through samples"""
    F = 61
    a = det_uniform((B, F, 2), seed, -2.0, wh + 2.0).astype(np.float64)
    b = det_uniform((B, F, 2), seed + 1, -2.0, wh + 2.0).astype(np.float64)
    a[:, ::2], b[:, ::2] = np.floor(a[:, ::2]) + 0.5, np.floor(b[:, ::2]) + 0.5
    s = det_uniform((B, F, 1), seed + 2, 0.1, 0.9).astype(np.float64)
    c = a + s * (b - a) + det_uniform((B, F, 2), seed + 3, -0.02, 0.02).astype(np.float64)
    p = np.stack([a, b, c], 2).reshape(B, 3 * F, 2)
    z = np.repeat(F32(1) + _ints((B, F), seed + 4, 0, 2).astype(F32), 3, axis=1)
    verts = verts_from_pixels(p[..., 0], p[..., 1], z, wh)
    return (verts, np.arange(3 * F, dtype=np.int32).reshape(F, 3), _parts(F, seed + 5)) + pixel_camera(wh, B)


def tiny(wh, B, seed=300):
    """121 faces of three own vertices within 1.2 px of each other (the SMPL case: a box of 1 to 9 samples, narrower than the 16 lanes
    that share a face); every second one is centred within 0.15 px of a sample, so that enough of them cover one"""
    F = 121
    c = det_uniform((B, F, 1, 2), seed, 0.0, float(wh)).astype(np.float64)
    c[:, ::2] = np.floor(c[:, ::2]) + 0.5 + det_uniform((B, (F + 1) // 2, 1, 2), seed + 4, -0.15, 0.15)      # every second face around a sample
    p = (c + det_uniform((B, F, 3, 2), seed + 1, -0.42, 0.42).astype(np.float64)).reshape(B, 3 * F, 2)      # 0.84 * sqrt(2) < 1.2
    z = det_uniform((B, 3 * F), seed + 2, 1.0, 3.0)
    verts = verts_from_pixels(p[..., 0], p[..., 1], z, wh)
    return (verts, np.arange(3 * F, dtype=np.int32).reshape(F, 3), _parts(F, seed + 3)) + pixel_camera(wh, B)


def huge(wh, B, seed=400):
    """20 vertices spread over 40 frames, 41 random triples: most vertices are far off the frame and a few faces cover the whole image
    (the box is the whole frame: 16 lanes walk wh * wh samples)"""
    N, F = 20, 41
    p = wh / 2.0 + 40.0 * wh * det_uniform((B, N, 2), seed, -0.5, 0.5).astype(np.float64)
    z = det_uniform((B, N), seed + 1, 1.0, 3.0)
    verts = verts_from_pixels(p[..., 0], p[..., 1], z, wh)
    faces = _ints((F, 3), seed + 2, 0, N).astype(np.int32)
    return (verts, faces, _parts(F, seed + 3)) + pixel_camera(wh, B)


def strips_faces(wh):
    """-> [(name, three (px, py) pixel-space corners, zc)]: the hand-made faces of `strips`.  zc is a power of two, so a corner given at
    a pixel centre projects onto its sample."""
    w = float(wh)
    f = [('full', [(-1.0, -1.0), (2 * w + 2, -1.0), (-1.0, 2 * w + 2)], 4.0),
         # an edge ALONG the centres of column 0 / row 0: the box is clamped to one column / one row, every sample in it is ON the edge
         ('col0_strip', [(0.5, -1.5), (0.5, w + 1.5), (-1.25, w / 2)], 2.0),
         ('row0_strip', [(-1.5, 0.5), (w + 1.5, 0.5), (w / 2, -1.25)], 2.0),
         # a thin wedge whose median runs along the centres of one inner column
         ('mid_col_wedge', [(wh // 2 + 0.5 - 0.3, -1.0), (wh // 2 + 0.5 + 0.3, -1.0), (wh // 2 + 0.5, w + 1.0)], 1.0)]
    if wh >= 33:       # right triangles with corners on pixel centres: legs of bw - 1 and 11 samples (coprime: no sample on the hypotenuse)
        for i, bw in enumerate((15, 16, 17)):
            c0, r0 = 2 + 5 * i, 3 + 9 * i
            f.append(('box_width_%d' % bw, [(c0 + 0.5, r0 + 0.5), (c0 + bw - 0.5, r0 + 0.5), (c0 + 0.5, r0 + 11.5)], 2.0))
    f += [('cross_left', [(-2.25, 0.2 * w), (0.35 * w + 0.77, 0.47 * w + 0.31), (-1.25, 0.8 * w)], 1.0),
          ('cross_right', [(w + 2.25, 0.15 * w), (0.6 * w - 0.77, 0.53 * w + 0.31), (w + 1.25, 0.85 * w)], 1.0),
          ('cross_row0', [(0.2 * w, -2.25), (0.47 * w + 0.31, 0.35 * w + 0.77), (0.8 * w, -1.25)], 1.0),
          ('cross_last_row', [(0.15 * w, w + 2.25), (0.53 * w + 0.31, 0.6 * w - 0.77), (0.85 * w, w + 1.25)], 1.0),
          ('outside_left', [(-5.25, 0.2 * w), (-0.25, 0.5 * w), (-4.25, 0.9 * w)], 1.0),
          ('outside_right', [(w + 5.25, 0.2 * w), (w + 0.25, 0.5 * w), (w + 4.25, 0.9 * w)], 1.0),
          ('outside_row0', [(0.2 * w, -5.25), (0.5 * w, -0.25), (0.9 * w, -4.25)], 1.0),
          ('outside_last_row', [(0.2 * w, w + 5.25), (0.5 * w, w + 0.25), (0.9 * w, w + 4.25)], 1.0),
          ('before_first_sample', [(-3.0, 0.2 * w), (0.25, 0.5 * w), (-2.0, 0.9 * w)], 1.0),      # inside the frame, left of column 0's centre
          ('xmax_is_minus_one', [(-3.0, 0.1 * w), (0.0, 0.4 * w), (-2.0, 0.7 * w)], 1.0)]          # pixel 0.0 is NDC -1 exactly
    return f


# float32 places a projected corner within a few ulp of 1 in NDC: 4e-7 * wh / 2 = 2e-5 px at wh = 100; ten times that
EDGE_MARGIN_PX = 2e-4


def strips_expected(wh):
    """-> {name: bool [wh,wh] in z-buffer orientation}: the samples each hand-made face covers BY CONSTRUCTION -- float64 edge functions on
    the pixel-space corners, where a pixel centre and a corner given in quarters are exact.  A sample closer than EDGE_MARGIN_PX to an edge without
    lying on it, where that edge decides, would make the float32 result a matter of rounding: asserted not to occur."""
    k = np.arange(wh) + 0.5
    px, py = k[None, :], k[:, None]
    out = {}
    for name, ((ax, ay), (bx, by), (cx, cy)), _ in strips_faces(wh):
        es, near = [], []
        for (x0, y0), (x1, y1) in (((bx, by), (cx, cy)), ((cx, cy), (ax, ay)), ((ax, ay), (bx, by))):
            e = (px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)
            dist = np.abs(e) / np.hypot(x1 - x0, y1 - y0)
            es.append(e)
            near.append((dist > 0) & (dist < EDGE_MARGIN_PX))
        for i in range(3):          # ... where that edge decides: the other two edge functions agree in sign
            a, b = es[(i + 1) % 3], es[(i + 2) % 3]
            assert not (near[i] & (((a >= 0) & (b >= 0)) | ((a <= 0) & (b <= 0)))).any(), (name, wh, 'a sample within EDGE_MARGIN_PX of an edge')
        out[name] = (np.stack(es) >= 0).all(0) | (np.stack(es) <= 0).all(0)
    return out


def strips(wh, B, seed=500):
    """the hand-made faces of strips_faces; bodies 1, 2, .. are body 0 shifted by whole pixels (b columns right, b rows down)"""
    spec = strips_faces(wh)
    p = np.array([c for _, corners, _ in spec for c in corners], np.float64)
    z = np.repeat(np.array([zc for _, _, zc in spec], F32), 3)
    verts = np.stack([verts_from_pixels(p[:, 0] + b, p[:, 1] + b, z, wh) for b in range(B)])
    F = len(spec)
    return (verts, np.arange(3 * F, dtype=np.int32).reshape(F, 3), _parts(F, seed)) + pixel_camera(wh, B)


DEPTH_FACES = ('duplicate_low', 'duplicate_high', 'vertex_behind_camera', 'straddles_near', 'beyond_far', 'at_zc_zero', 'nan_z', 'nan_x', 'backdrop')
DEPTH_INVALID = ('beyond_far', 'at_zc_zero', 'nan_z', 'nan_x')      # faces that must not contribute a single pixel
DEPTH_TZ = 0.5


def depth(wh, B, seed=600):
    """hand-made faces around the depth test, under t = (0, 0, 0.5): two coplanar duplicates with different parts (faces 0 and 1 index the
    same vertices), a vertex behind the camera, a face straddling `near`, one beyond `far`, one at exactly zc = 0 after the translation,
    one with a NaN z, one with a NaN x, and a backdrop behind them all"""
    w = float(wh)
    tri = lambda cx, cy, r: [(cx * w - r * w, cy * w - 0.6 * r * w), (cx * w + r * w, cy * w - 0.4 * r * w), (cx * w + 0.1 * r * w, cy * w + r * w)]
    spec = [(tri(0.3, 0.3, 0.25), (1.5, 2.0, 2.5)),                  # the duplicated pair's vertices
            (tri(0.7, 0.3, 0.2), (3.0, -1.0, 2.0)),                  # one vertex behind the camera
            (tri(0.3, 0.7, 0.2), (0.05, 0.05, 0.4)),                 # straddles near = 0.1
            (tri(0.7, 0.7, 0.2), (150.0, 160.0, 170.0)),             # beyond far = 100
            (tri(0.5, 0.5, 0.2), (0.0, 0.0, 0.0)),                   # zc = z + 0.5 = 0 exactly
            (tri(0.5, 0.25, 0.2), (2.0, 2.0, 2.0)),                  # -> NaN z
            (tri(0.5, 0.75, 0.2), (2.0, 2.0, 2.0)),                  # -> NaN x
            ([(-1.0, -1.0), (2 * w + 2, -1.0), (-1.0, 2 * w + 2)], (50.0, 50.0, 50.0))]
    p = np.array([c for corners, _ in spec for c in corners], np.float64)
    z = np.array([zc for _, zs in spec for zc in zs], F32)
    verts = np.stack([verts_from_pixels(p[:, 0] + b, p[:, 1] - b, z, wh, tz=DEPTH_TZ) for b in range(B)])
    verts[:, 5 * 3 + 1, 2] = np.nan
    verts[:, 6 * 3 + 2, 0] = np.nan
    faces = np.array([[0, 1, 2]] + [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(len(spec))], np.int32)
    assert len(faces) == len(DEPTH_FACES)
    parts = np.array([1, 6, 2, 3, 4, 5, 4, 3, 2], np.uint8)
    return (verts, faces, parts) + pixel_camera(wh, B, t=(0.0, 0.0, DEPTH_TZ))


BAD_FACES = ((5, 1, -1), (17, 0, None), (40, 2, None), (120, 0, -1))      # (face, corner, index; None = nverts)


def bad_indices(wh, B, seed=300):
    """`tiny` with a vertex index of -1 or nverts in four faces.  The kernel must skip them; the REFERENCE for this family is the same scene
    with those faces made degenerate (degenerate_bad_faces), which keeps the ids of the other faces"""
    verts, faces, parts, K, R, t = tiny(wh, B, seed)
    faces = faces.copy()
    for f, c, idx in BAD_FACES:
        faces[f, c] = verts.shape[1] if idx is None else idx
    return verts, faces, parts, K, R, t


def degenerate_bad_faces(faces, nverts):
    """faces with an index outside [0, nverts) -> (0, 0, 0)"""
    faces = np.array(faces, copy=True)
    faces[((faces < 0) | (faces >= nverts)).any(1)] = 0
    return faces


_BUILDERS = {'on_centre': on_centre, 'slivers': slivers, 'tiny': tiny, 'huge': huge, 'strips': strips, 'depth': depth, 'bad_indices': bad_indices}


@functools.lru_cache(maxsize=None)
def scene(family, wh, B):
    """-> (verts [B,N,3], faces [F,3] int32, face_parts [F] uint8, K [3,3], R [3,3], t [B,3]); cached: do not modify"""
    out = _BUILDERS[family](wh, B)
    for a in out:
        a.setflags(write=False)
    return out


def single_face_scene(wh=5):
    """B = F = 1: the full-frame face of `strips` alone"""
    verts, faces, parts, K, R, t = scene('strips', wh, 1)
    return verts[:, :3].copy(), faces[:1].copy(), parts[:1].copy(), K, R, t


def reference_scene(family, wh, B):
    """the scene the references are run on: `scene`, with the faces of bad_indices made degenerate"""
    verts, faces, parts, K, R, t = scene(family, wh, B)
    return verts, degenerate_bad_faces(faces, verts.shape[1]), parts, K, R, t


@functools.lru_cache(maxsize=None)
def brute_reference(family, wh, B):
    """-> (parts, depth) of rasterize_brute on reference_scene; computed once per process and shared: do not modify"""
    verts, faces, parts, K, R, t = reference_scene(family, wh, B)
    out = rasterize_brute(verts, faces, parts, K, R, t, wh, return_depth=True)
    for a in out:
        a.setflags(write=False)
    return out


def rotated_camera_scene(wh=48, B=3, seed=700):
    """world-space scene under PER-BODY cameras with R != I and t != 0: 60 vertices, 95 random faces, three focal lengths, three rotations
    about y, three translations (body 2 crosses the near plane)"""
    N, F = 60, 95
    verts = det_uniform((B, N, 3), seed, -1.0, 1.0) * np.array([0.5, 0.9, 0.3], F32)
    faces = _ints((F, 3), seed + 1, 0, N).astype(np.int32)
    K = np.stack([O.intrinsics_matrix(wh, wh, f) for f in (0.9 * wh, 1.4 * wh, 2.2 * wh)]).astype(F32)[:B]
    R = np.stack([np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F32) for a in (0.25, 0.4, -0.7)])[:B]
    t = np.array([[0.0, 0.0, 2.5], [0.1, -0.2, 3.0], [-0.3, 0.1, 1.2]], F32)[:B]
    return verts, faces, _parts(F, seed + 2), K, R, t


# --------------------------------------------------------------------------------------------------------------------------------
# crop cases
# --------------------------------------------------------------------------------------------------------------------------------
CROP_CASES = ('empty', 'first_pixel', 'last_pixel', 'centre_pixel', 'full_row', 'full_col', 'full_frame', 'blob_row0', 'blob_last_row', 'blob_col0',
              'blob_last_col', 'blob_inside')
CROP_UNPINNED = ('empty', 'first_pixel', 'last_pixel', 'centre_pixel')      # np.amin of nothing / a crop of zero size: the reference raises


def crop_cases(wh, seed=800):
    """-> {name: float32 [wh,wh] silhouette with part ids 1..6 (0 = background)}"""
    ids = (1 + _ints((wh, wh), seed + wh, 0, 6)).astype(F32)
    a, b = wh // 3, max(wh // 3 + 1, (2 * wh) // 3)
    regions = {'empty': None, 'first_pixel': (slice(0, 1), slice(0, 1)), 'last_pixel': (slice(wh - 1, wh), slice(wh - 1, wh)),
               'centre_pixel': (slice(wh // 2, wh // 2 + 1), slice(wh // 2, wh // 2 + 1)), 'full_row': (slice(a, a + 1), slice(0, wh)),
               'full_col': (slice(0, wh), slice(b - 1, b)), 'full_frame': (slice(0, wh), slice(0, wh)),
               'blob_row0': (slice(0, b), slice(a, b)), 'blob_last_row': (slice(a, wh), slice(a, b)), 'blob_col0': (slice(a, b), slice(0, b)),
               'blob_last_col': (slice(a, b), slice(a, wh)), 'blob_inside': (slice(a, b), slice(a, b + 1 if b + 1 < wh else b))}
    out = {}
    for name in CROP_CASES:
        seg = np.zeros((wh, wh), F32)
        if regions[name] is not None:
            seg[regions[name]] = ids[regions[name]]
        out[name] = seg
    return out


def crop_joints(B, nj, wh, seed=810):
    """[B,nj,2] float32 joints, some outside the frame"""
    return det_uniform((B, nj, 2), seed + 31 * nj + B, -0.2 * wh, 1.2 * wh)


def crop_draws(B, seed=820):
    """[B,3] float32 jitter draws (scale, centre row, centre column) in [0, 1): 0 and 1 - 2**-24 included"""
    u = det_uniform((B, 3), seed + B, 0.0, 1.0)
    u[0] = (0.0, LAST_DRAW, 0.0)
    if B > 1:
        u[1] = (LAST_DRAW, 0.0, LAST_DRAW)
    return u


def crop_expected(seg, joints, u, out_wh):
    """one image [wh,wh], its joints [nj,2] and draws [3] (or None) -> (map [out_wh,out_wh], joints float64 [nj,2], box r0,c0,r1,c1, pinned).
    pinned: O.crop_resize could process it (a box of positive height and width).  Otherwise the KERNEL's documented behaviour, which the
    reference does not pin: an empty frame keeps the whole frame as its box, gives an all-zero map and rescales the joints by out_wh / wh;
    a crop of zero size gives an all-zero map and joints (j - corner) * out_wh (a crop with ONE empty side, which the centre jitter of
    +-5 px can produce in a frame of 6 or 7 pixels: an all-zero map, the empty side counted as one pixel) -- its box is still the
    reference's arithmetic (O.crop_boxes)."""
    wh = seg.shape[-1]
    u64 = None if u is None else np.asarray(u, F32).astype(np.float64)[None]
    if not seg.any():
        return np.zeros((out_wh, out_wh), F32), joints.astype(np.float64) * (out_wh / float(wh)), np.array([0, 0, wh, wh]), False
    boxes, cj = O.crop_boxes(seg[None], joints[None].astype(np.float64), u64)
    r0, c0, r1, c1 = boxes[0]
    if r1 - r0 > 0 and c1 - c0 > 0:
        out, oj, boxes = O.crop_resize(seg[None], joints[None], u64, out_wh=out_wh)
        return out[0], oj[0], boxes[0], True
    scale = np.array([out_wh / float(max(c1 - c0, 1)), out_wh / float(max(r1 - r0, 1))])      # an empty side counts as one pixel
    return np.zeros((out_wh, out_wh), F32), cj[0] * scale, boxes[0], False


# --------------------------------------------------------------------------------------------------------------------------------
# occlusion cases
# --------------------------------------------------------------------------------------------------------------------------------
REMOVE_PROBS = np.array([0.1, 0.1, 0.1, 0.1, 0.05, 0.05], F32)
OCCLUDE_PROB = 0.5
SEG_CASES = ('all_removed', 'nothing_removed', 'box_first_last', 'box_last_first', 'draw_equals_prob', 'random')


def seg_cases(B, wh, seed=900):
    """-> {name: (seg float32 [B,wh,wh] with part ids 0..8, draws float32 [B,9])}; the named draw is body 0's, the other bodies draw at
    random.  Draws as in test_augment_seg_bit_exact_vs_oracle: 6 removal draws, the occlusion draw, the two box-centre draws."""
    out = {}
    for i, name in enumerate(SEG_CASES):
        seg = _ints((B, wh, wh), seed + 10 * i + wh, 0, 9).astype(F32)
        seg[:, 0, 0], seg[:, -1, -1] = 7.0, 8.0                       # two pixels no occlusion box of these cases reaches
        u = det_uniform((B, 9), seed + 10 * i + 1 + B, 0.0, 1.0)
        if name == 'all_removed':
            u[0, :7] = 0.0
        elif name == 'nothing_removed':
            u[0, :7] = 0.99
        elif name == 'box_first_last':
            u[0, :6], u[0, 6], u[0, 7], u[0, 8] = 0.99, 0.0, 0.0, LAST_DRAW
        elif name == 'box_last_first':
            u[0, :6], u[0, 6], u[0, 7], u[0, 8] = 0.99, 0.0, LAST_DRAW, 0.0
        elif name == 'draw_equals_prob':
            u[0, :6] = REMOVE_PROBS                                   # equal to float32(prob): not removed
            u[0, 6] = F32(OCCLUDE_PROB)                               # equal to the occlusion probability: not occluded
        out[name] = (seg, u)
    return out
