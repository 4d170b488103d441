"""CPU: the data-generation case tables (tests/datagen_cases.py) without a GPU -- the oracle's rasteriser, which walks a per-face bounding
box with the kernel's own float32 formula, equals the brute force that tests every face at every pixel centre, in parts and depth, on
every scene of every family; each family exercises what it was built for (conditions on the REFERENCES alone, so that a case cannot
pass while exercising nothing); the crop reference gives the boxes the crop cases name; the occlusion cases keep ids 7 and 8."""
import numpy as np
import pytest

import datagen_cases as DC
import straps_oracle as O


def _covered(family, wh, B):
    return DC.brute_reference(family, wh, B)[0] > 0


# ---- the box formula loses no sample -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wh', DC.RASTER_WH)
@pytest.mark.parametrize('family', DC.FAMILIES)
def test_oracle_with_boxes_equals_brute_force(family, wh):
    for B in DC.RASTER_B:
        verts, faces, parts, K, R, t = DC.reference_scene(family, wh, B)
        want, wdepth = DC.brute_reference(family, wh, B)
        got, gdepth = O.rasterize_parts(verts, faces, parts, K, R, t, wh=wh, near=DC.NEAR, far=DC.FAR, return_depth=True)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (B, wh, wh)
        assert np.array_equal(got, want), '%s wh %d B %d: %d part pixels differ' % (family, wh, B, int((got != want).sum()))
        assert np.array_equal(gdepth, wdepth), '%s wh %d B %d: %d depth pixels differ' % (family, wh, B, int((gdepth != wdepth).sum()))
        assert not np.isnan(wdepth).any() and set(np.unique(want).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0}


def test_oracle_equals_brute_force_under_rotated_per_body_cameras_and_on_one_face():
    verts, faces, parts, K, R, t = DC.rotated_camera_scene()
    want = DC.rasterize_brute(verts, faces, parts, K, R, t, 48, return_depth=True)
    got = O.rasterize_parts(verts, faces, parts, K, R, t, wh=48, return_depth=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert ((want[0] > 0).mean(axis=(1, 2)) > 0.1).all() and not np.array_equal(want[0][0], want[0][1])
    assert not np.array_equal(R[1], np.eye(3)) and t[:, :2].any() and K.shape == R.shape == (3, 3, 3)
    verts, faces, parts, K, R, t = DC.single_face_scene()
    assert verts.shape[0] == 1 and faces.shape == (1, 3)                        # B = F = 1
    want = DC.rasterize_brute(verts, faces, parts, K, R, t, 5, return_depth=True)
    got = O.rasterize_parts(verts, faces, parts, K, R, t, wh=5, return_depth=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[0] == parts[0]).all()


# ---- conditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', DC.FAMILIES)
def test_no_scene_fills_whole_groups_of_sixteen_lanes(family):
    """B * F is no multiple of 16: the last workgroup of raster_face_kernel is ragged in every scene"""
    for wh in DC.RASTER_WH:
        for B in DC.RASTER_B:
            verts, faces, parts, K, R, t = DC.scene(family, wh, B)
            assert verts.shape[0] == B and verts.dtype == np.float32 and faces.dtype == np.int32 and parts.dtype == np.uint8
            assert (B * faces.shape[0]) % 16 != 0 and parts.shape == (faces.shape[0],) and t.shape == (B, 3)


def test_on_centre_puts_samples_exactly_on_edges():
    """at least 30 inside pairs with an edge function of exactly 0.0 at every wh >= 2 (measured, B = 1 / 3: 78 / 256 at wh 2, 190 / 729 at 5,
    692 / 2144 at 33, 672 / 1956 at 48, 1112 / 2923 at 64, 919 / 2139 at 100)"""
    for wh in DC.RASTER_WH[1:]:
        for B in DC.RASTER_B:
            assert DC.zero_edge_pairs(*DC.scene('on_centre', wh, B), wh) >= 30, (wh, B)


def test_tiny_slivers_and_huge_cover_what_they_should():
    """tiny and slivers: at least one sample, less than 20 % of the frame, at wh >= 33 (measured: tiny 11 .. 46 samples, slivers 98 .. 351
    samples and at most 9.6 %); huge: at least 90 % (measured: every sample at every size)"""
    for wh in DC.RASTER_WH:
        for B in DC.RASTER_B:
            if wh >= 33:
                for family in ('tiny', 'slivers', 'bad_indices'):
                    c = _covered(family, wh, B)
                    assert c.any(axis=(1, 2)).all() and c.mean() < 0.2, (family, wh, B, c.mean())
            assert _covered('huge', wh, B).mean() >= 0.9, (wh, B)
    for wh in (33, 64):           # the boxes of tiny are narrower than the 16 lanes of a face, those of huge are the frame
        bx = DC.sample_boxes(*DC.scene('tiny', wh, 1)[:2], *DC.scene('tiny', wh, 1)[3:], wh)
        assert (bx[:, 1] - bx[:, 0] + 1).max() <= 4 and (bx[:, 3] - bx[:, 2] + 1).max() <= 4
        bx = DC.sample_boxes(*DC.scene('huge', wh, 1)[:2], *DC.scene('huge', wh, 1)[3:], wh)
        assert ((bx[:, 1] - bx[:, 0] + 1 == wh) & (bx[:, 3] - bx[:, 2] + 1 == wh)).sum() >= 5


@pytest.mark.parametrize('wh', DC.RASTER_WH)
def test_each_strips_face_covers_exactly_the_samples_of_its_construction(wh):
    verts, faces, parts, K, R, t = DC.scene('strips', wh, 1)
    names = [n for n, _, _ in DC.strips_faces(wh)]
    want = DC.strips_expected(wh)
    got = DC.coverage(verts, faces, K, R, t, wh)
    for f, name in enumerate(names):
        assert np.array_equal(got[f], want[name]), (wh, name, int(got[f].sum()), int(want[name].sum()))
        alone = DC.rasterize_brute(verts, faces[f:f + 1], parts[f:f + 1], K, R, t, wh)[0] > 0       # the face alone, through the depth test and the flip
        assert np.array_equal(alone[::-1], want[name]), (wh, name)
    assert want['full'].all() and want['col0_strip'][:, 0].all() and not want['col0_strip'][:, 1:].any()
    assert want['row0_strip'][0].all() and not want['row0_strip'][1:].any()
    assert want['mid_col_wedge'][:, wh // 2].all() and want['mid_col_wedge'].sum() == wh
    for name in names:
        if name.startswith('outside') or name in ('before_first_sample', 'xmax_is_minus_one'):
            assert not want[name].any(), name
    if wh >= 5:
        assert want['cross_left'][:, 0].any() and want['cross_right'][:, -1].any() and want['cross_row0'][0].any() and want['cross_last_row'][-1].any()
    X = DC._project(verts, K, R, t, wh)[0][0]
    assert X[faces[names.index('xmax_is_minus_one')]].max() == np.float32(-1.0)
    boxes = dict(zip(names, DC.sample_boxes(verts, faces, K, R, t, wh)))
    width = lambda n: boxes[n][1] - boxes[n][0] + 1
    assert tuple(boxes['xmax_is_minus_one'][:2]) == (0, 0) and tuple(boxes['outside_left']) == (0, -1, 0, -1)
    assert width('full') == wh and width('row0_strip') == wh
    if wh >= 33:                  # 11-sample legs: 12 + 11 + .. lattice points below a hypotenuse that passes through none
        for bw in (15, 16, 17):
            n = 'box_width_%d' % bw
            assert want[n].sum() == sum(int(np.floor((bw - 1) * (11 - j) / 11.0)) + 1 for j in range(12)) and want[n].any(axis=0).sum() == bw
            assert width(n) >= bw
    if wh == 64:                  # a power of two: the box formula is exact, and the widths sit around the 16 lanes of a face
        assert [width('box_width_%d' % bw) for bw in (15, 16, 17)] == [15, 16, 17]
        assert width('col0_strip') == 1 and boxes['row0_strip'][3] - boxes['row0_strip'][2] + 1 == 1


def test_depth_family_decides_ties_and_rejects_invalid_faces():
    for wh in DC.RASTER_WH:
        for B in DC.RASTER_B:
            verts, faces, parts, K, R, t = DC.scene('depth', wh, B)
            assert np.array_equal(faces[0], faces[1]) and parts[0] != parts[1]
            got, depth, fid = DC.rasterize_brute(verts, faces, parts, K, R, t, wh, return_depth=True, return_faces=True)
            pair = DC.rasterize_brute(verts, faces[1:2], parts[1:2], K, R, t, wh) > 0      # where the higher id of the pair would show alone
            both = DC.rasterize_brute(verts, faces[:2], parts[:2], K, R, t, wh, return_faces=True)
            assert ((both[1] == 0) == pair).all() and (both[0][pair] == parts[0]).all()         # ... the lower id shows, on every shared pixel
            assert not (fid == 1).any()
            if wh >= 5:
                assert pair[0].any() and (fid == 0).any() and (got[fid == 0] == parts[0]).all()
            for name in DC.DEPTH_INVALID:
                f = DC.DEPTH_FACES.index(name)
                assert not (fid == f).any(), (wh, B, name)
                alone = DC.rasterize_brute(verts, faces[f:f + 1], parts[f:f + 1], K, R, t, wh, return_depth=True)
                assert not alone[0].any() and (alone[1] == np.float32(DC.FAR)).all(), (wh, B, name)
            if wh >= 33:          # the near plane cuts its face: some of it shows, and less than the face covers
                f = DC.DEPTH_FACES.index('straddles_near')
                cov = DC.coverage(verts, faces, K, R, t, wh)[f]
                assert 0 < (fid[0] == f).sum() < cov.sum()
            zc = verts[0, faces[DC.DEPTH_FACES.index('at_zc_zero')], 2] + np.float32(DC.DEPTH_TZ)
            assert (zc == 0).all() and np.isnan(verts[0, faces[6], 2]).sum() == 1 and np.isnan(verts[0, faces[7], 0]).sum() == 1


def test_bad_indices_reference_keeps_the_other_faces():
    for wh in (5, 64):
        verts, faces, parts, K, R, t = DC.scene('bad_indices', wh, 3)
        N = verts.shape[1]
        bad = ((faces < 0) | (faces >= N)).any(1)
        assert bad.sum() == len(DC.BAD_FACES) and set(faces[bad].ravel().tolist()) >= {-1, N}
        ref = DC.reference_scene('bad_indices', wh, 3)[1]
        assert (ref[bad] == 0).all() and np.array_equal(ref[~bad], faces[~bad]) and np.array_equal(ref[~bad], DC.scene('tiny', wh, 3)[1][~bad])


# ---- crop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wh', (6, 7, 30, 33, 64, 68))
def test_crop_reference_on_the_crop_cases(wh):
    cases = DC.crop_cases(wh)
    assert tuple(cases) == DC.CROP_CASES
    j = DC.crop_joints(1, 17, wh)[0]
    for name, seg in cases.items():
        assert seg.dtype == np.float32 and seg.shape == (wh, wh) and set(np.unique(seg).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0}
        for u in (None, DC.crop_draws(1)[0], DC.crop_draws(3)[1]):
            out, oj, box, pinned = DC.crop_expected(seg, j, u, 5)
            if u is None or wh >= 30:                               # (in a frame of 6 or 7 pixels the +-5 px centre jitter can empty a crop)
                assert pinned == (name not in DC.CROP_UNPINNED), (name, box)
            assert out.shape == (5, 5) and oj.shape == (17, 2) and np.isfinite(oj).all()
            if pinned:                                             # a nearest resize only picks pixels of the crop
                r0, c0, r1, c1 = box
                assert 0 <= r0 < r1 <= wh and 0 <= c0 < c1 <= wh and set(np.unique(out).tolist()) <= set(np.unique(seg[r0:r1, c0:c1]).tolist())
    box = lambda name: tuple(int(v) for v in DC.crop_expected(cases[name], j, None, 5)[2])
    # the reference measures a silhouette by max - min = wh - 1 pixels, times 1.2: the box reaches the far edge from wh = 11 on
    assert box('full_frame') == ((0, 0, wh, wh) if wh >= 11 else (0, 0, wh - 1, wh - 1)) and box('empty') == (0, 0, wh, wh)
    # border blobs: the scaled box leaves the frame on the blob's side and is clamped there
    assert box('blob_row0')[0] == 0 and box('blob_col0')[1] == 0 and box('full_row')[1] == 0 and box('full_col')[0] == 0
    if wh >= 11:
        assert box('blob_last_row')[2] == wh and box('blob_last_col')[3] == wh and box('full_row')[3] == wh and box('full_col')[2] == wh
    r0, c0, r1, c1 = box('blob_inside')
    ys, xs = np.nonzero(cases['blob_inside'])
    assert r0 <= ys.min() and ys.max() < r1 + (wh < 11) and c0 <= xs.min() and xs.max() < c1 + (wh < 11)
    assert np.flatnonzero(cases['first_pixel']).tolist() == [0] and np.flatnonzero(cases['last_pixel']).tolist() == [wh * wh - 1]
    assert cases['full_row'].astype(bool).sum(1).max() == wh and cases['full_col'].astype(bool).sum(0).max() == wh
    u = DC.crop_draws(3)
    assert u.dtype == np.float32 and 0.0 in u and DC.LAST_DRAW in u and u.max() < 1.0


# ---- occlusion -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wh', (5, 33, 64, 100))
def test_occlusion_cases_keep_ids_seven_and_eight(wh):
    for B in (1, 3):
        cases = DC.seg_cases(B, wh)
        assert tuple(cases) == DC.SEG_CASES
        for box in (0, 1, 3, int(np.floor(0.7 * wh))):
            for name, (seg, u) in cases.items():
                assert seg.shape == (B, wh, wh) and u.shape == (B, 9) and u.dtype == np.float32 and set(np.unique(seg).tolist()) <= set(range(9))
                out = O.augment_seg(seg, u, remove_probs=DC.REMOVE_PROBS, occlude_probability=DC.OCCLUDE_PROB, occlude_box_dim=box)
                changed = out[0] != seg[0]
                assert (out[0][changed] == 0).all()
                if name == 'all_removed':
                    assert not np.isin(out[0], (1, 2, 3, 4, 5, 6)).any() and changed[seg[0] >= 7].sum() <= box * box
                    assert (out[0] == 7).any() and (out[0] == 8).any()
                elif name in ('nothing_removed', 'draw_equals_prob'):
                    assert np.array_equal(out[0], seg[0])
                elif name.startswith('box_'):
                    ys, xs = np.nonzero(changed | (seg[0] == 0))
                    gone = np.zeros((wh, wh), bool)
                    # corners as the reference forms them; the extreme draws put the box against the ends of the centre range
                    lo, hi = wh / 2 + 0.3 * wh / 2, wh / 2 - 0.3 * wh / 2
                    cx, cy = ((hi - lo) * np.float64(u[0, 7]) + lo, (hi - lo) * np.float64(u[0, 8]) + lo)
                    gone[int(cx - box / 2):int(cx + box / 2), int(cy - box / 2):int(cy + box / 2)] = True
                    assert cx - box / 2 >= 0 and cy - box / 2 >= 0 and cx + box / 2 <= wh and cy + box / 2 <= wh
                    assert np.array_equal(changed, gone & (seg[0] != 0)) and gone.sum() == box * box
