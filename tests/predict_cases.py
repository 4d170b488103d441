"""Predict-side proxy input (straps_predict_proxy_input): a numpy restatement of the semantics include/straps_hip.h states, and the
case table of tests/golden/predict_proxy_golden.npz.

The restatement is written from the header's text, not from the reference; tools/make_predict_proxy_golden.py runs the reference itself
on `inputs()` and stores what it returns, and tests/test_predict_proxy_cpu.py holds the two against each other.

GROUPS: one kernel call takes one (H, W, nj, ld_joint), so the samples are grouped by it; a group's samples form one mixed batch.
Every sample names the properties it is in the table for; `check_properties` asserts them on the computed window, so that a change of
the table cannot silently lose a case."""
import numpy as np

SCALE, STD = 1.2, 4


# ---------------------------------------------------------------- restatement ----------------------------------------------------------------
def _i16(v):
    """float64 -> int16 as numpy's astype: truncation toward zero (values stay inside int16 here)"""
    return int(np.float64(v).astype(np.int16))


def window(sil, scale=SCALE):
    """-> (wr0, wc0, wr1, wc1, valid) of one [H,W] silhouette"""
    rows, cols = np.nonzero(sil.any(axis=1))[0], np.nonzero(sil.any(axis=0))[0]
    if rows.size == 0:
        return 0, 0, 0, 0, 0
    rmin, rmax, cmin, cmax = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    cr, cc = (rmin + rmax) / 2.0, (cmin + cmax) / 2.0
    side = max(rmax - rmin, cmax - cmin) * scale
    wr0, wc0, wr1, wc1 = _i16(cr - side / 2.0), _i16(cc - side / 2.0), _i16(cr + side / 2.0), _i16(cc + side / 2.0)
    return wr0, wc0, wr1, wc1, int(wr1 - wr0 > 0 and wc1 - wc0 > 0)


def _nearest(n_out, n_src):
    return np.minimum(np.floor(np.arange(n_out) * (1.0 / (n_out / float(n_src)))).astype(np.int64), n_src - 1)


def proxy_input(sil, joints, patch, out_wh, scale=SCALE, std=STD):
    """sil [B,H,W] uint8, joints [B,nj,ld>=2] float32, patch [4 std, 4 std] float32
    -> (out [B,1+nj,out_wh,out_wh] float32, joints [B,nj,2] float64, boxes [B,6] int32).  The float32 joints output is np.float32 of these."""
    B, H, W = sil.shape
    nj, size = joints.shape[1], 2 * std
    out = np.zeros((B, 1 + nj, out_wh, out_wh), np.float32)
    jout = np.zeros((B, nj, 2), np.float64)
    boxes = np.zeros((B, 6), np.int32)
    for b in range(B):
        wr0, wc0, wr1, wc1, valid = window(sil[b], scale)
        boxes[b, :5] = wr0, wc0, wr1, wc1, valid
        if not valid:
            continue
        ch, cw = wr1 - wr0, wc1 - wc0
        ys, xs = wr0 + _nearest(out_wh, ch), wc0 + _nearest(out_wh, cw)
        inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        out[b, 0] = np.where(inside, sil[b][np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)], 0)
        shifted = joints[b, :, :2].astype(np.float32) - np.array([wc0, wr0], np.float32)          # float32 - int16 -> float32
        assert shifted.dtype == np.float32
        jout[b] = shifted.astype(np.float64) * np.array([out_wh / float(cw), out_wh / float(ch)])
        for j in range(nj):
            jx, jy = _i16(jout[b, j, 0]), _i16(jout[b, j, 1])
            if not (jx > -size and jy > -size and jx < out_wh - 1 + size and jy < out_wh - 1 + size):
                continue
            for y in range(max(0, jy - size), min(out_wh - 1, jy + size)):
                for x in range(max(0, jx - size), min(out_wh - 1, jx + size)):
                    out[b, 1 + j, y, x] = patch[y - jy + size, x - jx + size]
    return out, jout, boxes


# ---------------------------------------------------------------- case table ----------------------------------------------------------------
def _blob(h, w, r0, r1, c0, c1, seed):
    """label image whose non-zero pixels span exactly rows r0..r1, cols c0..c1: labels 0..3 with holes, two opposite corners set"""
    rng = np.random.RandomState(seed)
    s = np.zeros((h, w), np.uint8)
    s[r0:r1 + 1, c0:c1 + 1] = rng.randint(0, 4, (r1 - r0 + 1, c1 - c0 + 1))
    s[r0, c0], s[r1, c1] = 1, 7
    return s


def _scatter_joints(h, w, nj, ld, seed):
    """joints spread over and around the frame: some inside, some clipped, some far outside"""
    rng = np.random.RandomState(seed)
    j = np.empty((nj, ld), np.float32)
    j[:, 0] = rng.uniform(-0.3 * w, 1.3 * w, nj)
    j[:, 1] = rng.uniform(-0.3 * h, 1.3 * h, nj)
    if ld > 2:
        j[:, 2:] = rng.uniform(0, 1, (nj, ld - 2))
    return j


def _targets(wr0, wc0, scale_to_out, targets, ld, seed):
    """input joints that land on `targets` (x', y') in the output of a window at (wr0, wc0) with a power-of-two scale: exact in float32"""
    t = np.asarray(targets, np.float64)
    j = np.empty((t.shape[0], ld), np.float32)
    j[:, 0], j[:, 1] = wc0 + t[:, 0] / scale_to_out, wr0 + t[:, 1] / scale_to_out
    if ld > 2:
        j[:, 2:] = np.random.RandomState(seed).uniform(0, 1, (t.shape[0], ld - 2))
    return j


# the 32 x 32 window of rows / cols 17..44 in a 64 x 64 frame: [14, 46) both ways, so out_wh 32 scales by 1 and out_wh 64 by 2, exactly
W32 = (17, 44, 17, 44)
# targets in the out_wh = 32 output (visible iff -8 < j < 39, both coordinates)
TARGETS_32 = [(16, 16), (10.7, 20.3), (-8, 16), (-7, 16), (16, -8), (16, -7), (39, 16), (38, 16), (16, 39), (16, 38), (-7.5, 5.5), (-0.5, 12.25),
              (3, 28), (28, 3), (31, 31), (-100, 16), (500, -3000)]
# targets in the out_wh = 64 output (visible iff -8 < j < 71); in the out_wh = 32 output they are halved
TARGETS_64 = [(32, 32), (-8, 32), (-7, 32), (32, -8), (32, -7), (71, 32), (70, 32), (32, 71), (32, 70), (-7.5, 11), (-0.5, 24.5), (5, 60), (60, 5),
              (63, 63), (0, 0), (-200, 32), (1000, 2000)]

# group -> (H, W, nj, ld_joint, out_whs, [(sample name, silhouette, joints, properties)])
def _groups():
    g = {}
    g['a'] = (64, 64, 17, 3, (32, 64), [
        ('corner_top_left', _blob(64, 64, 0, 30, 0, 25, 1), _scatter_joints(64, 64, 17, 3, 11), ('top', 'left', 'ch!=cw', 'upsample64')),
        ('small_interior', _blob(64, 64, 20, 29, 30, 37, 2), _scatter_joints(64, 64, 17, 3, 12), ('interior', 'upsample32')),
        ('corner_truncates_to_zero', _blob(64, 64, 3, 34, 20, 40, 3), _scatter_joints(64, 64, 17, 3, 13), ('interior', 'row0_from_fraction')),
        ('joints_on_bounds_32', _blob(64, 64, *W32, 4), _targets(14, 14, 1.0, TARGETS_32, 3, 14), ('interior', 'window32')),
        ('joints_on_bounds_64', _blob(64, 64, *W32, 5), _targets(14, 14, 2.0, TARGETS_64, 3, 15), ('interior', 'window32')),
    ])
    g['b'] = (80, 96, 17, 3, (32,), [
        ('top_and_bottom', _blob(80, 96, 2, 77, 30, 66, 6), _scatter_joints(80, 96, 17, 3, 16), ('top', 'bottom', 'ch!=cw', 'downsample32')),
        ('large_interior', _blob(80, 96, 10, 66, 20, 80, 7), _scatter_joints(80, 96, 17, 3, 17), ('interior', 'downsample32')),
    ])
    g['c'] = (96, 80, 17, 3, (64,), [
        ('left_and_right', _blob(96, 80, 30, 66, 2, 77, 8), _scatter_joints(96, 80, 17, 3, 18), ('left', 'right', 'ch!=cw', 'downsample64')),
        ('large_interior', _blob(96, 80, 18, 78, 20, 60, 9), _scatter_joints(96, 80, 17, 3, 19), ('interior', 'downsample64')),
    ])
    g['d'] = (64, 64, 1, 2, (32,), [
        ('corner_bottom_right', _blob(64, 64, 40, 63, 35, 63, 10), np.array([[50.2, 55.9]], np.float32), ('bottom', 'right')),
        ('negative_joint', _blob(64, 64, *W32, 11), _targets(14, 14, 1.0, [(-7.5, 5.5)], 2, 0), ('interior', 'window32')),
        ('joint_far_outside', _blob(64, 64, 20, 29, 30, 37, 12), np.array([[-30.0, 200.0]], np.float32), ('interior',)),
    ])
    return g


GROUPS = _groups()


def inputs(group):
    """-> (sil [B,H,W] uint8, joints [B,nj,ld] float32) of a group"""
    samples = GROUPS[group][5]
    return np.stack([s[1] for s in samples]), np.stack([s[2] for s in samples])


def check_properties(group):
    """the windows of a group's samples have the properties the table claims"""
    H, W, _, _, outs, samples = GROUPS[group]
    for name, sil, _, props in samples:
        wr0, wc0, wr1, wc1, valid = window(sil)
        ch, cw = wr1 - wr0, wc1 - wc0
        assert valid, name
        leaves = {'top': wr0 < 0, 'bottom': wr1 > H, 'left': wc0 < 0, 'right': wc1 > W}
        for side, out_of_frame in leaves.items():
            assert out_of_frame == (side in props), (name, side, (wr0, wc0, wr1, wc1))
        assert ('interior' in props) == (not any(leaves.values())), name
        if 'ch!=cw' in props:
            assert ch != cw, name
        if 'window32' in props:
            assert (wr0, wc0, wr1, wc1) == (14, 14, 46, 46), name
        if 'row0_from_fraction' in props:      # the exact corner lies in (-1, 0): truncation gives 0 (floor would give -1), so no padding
            rows = np.nonzero(sil.any(axis=1))[0]
            exact = (rows[0] + rows[-1]) / 2.0 - (max(rows[-1] - rows[0], 0) * SCALE) / 2.0
            assert -1 < exact < 0 and wr0 == 0, (name, exact)
        for o in (32, 64):
            if 'upsample%d' % o in props:
                assert o in outs and max(ch, cw) < o, name
            if 'downsample%d' % o in props:
                assert o in outs and min(ch, cw) > o, name


# the two samples the reference cannot complete (it raises): defined output = all zeros, valid 0
def invalid_silhouettes(h=64, w=64):
    empty = np.zeros((h, w), np.uint8)
    one_pixel = np.zeros((h, w), np.uint8)
    one_pixel[20, 30] = 1                         # side 0: the window truncates to zero height and width
    return {'empty': empty, 'one_pixel': one_pixel}
