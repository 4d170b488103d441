"""CPU: the restatements of tests/render_cases.py stand on their own feet before the GPU is held against them -- the float32 restatement
equals the hand counts and, as a mask, the silhouette restatement of tests/eval_cases.py; the host's vertex-to-face table equals a
brute-force one; the depth key orders floats as floats; and every mesh whose colours are compared meets the condition the one-level
colour bound rests on."""
import numpy as np
import pytest

import eval_cases as EC
import render_cases as RC
import straps_amd


@pytest.mark.parametrize('name', RC.HAND_COUNTED)
def test_restatement_equals_the_hand_counts(name):
    c = RC.case(name)
    ref = c['ref']
    assert c['wh'] == 16 and c['expected_ids'] is not None
    assert np.array_equal(ref['face_ids'], c['expected_ids']), name
    assert np.array_equal(ref['mask'], (c['expected_ids'] >= 0).astype(np.uint8))
    assert np.isposinf(ref['depth'][ref['mask'] == 0]).all() and np.isfinite(ref['depth'][ref['mask'] == 1]).all()


def test_hand_counts_cover_both_depth_orders_and_the_tie():
    b_front, a_front = RC.case('pair_b_in_front'), RC.case('pair_negative_a_in_front')
    assert (b_front['ref']['face_ids'] == 1).sum() == 45 and (b_front['ref']['face_ids'] == 0).sum() == 30
    assert (a_front['ref']['face_ids'] == 0).sum() == 45 and (a_front['ref']['face_ids'] == 1).sum() == 30
    d = a_front['ref']['depth'][0]
    assert (d[a_front['ref']['face_ids'][0] == 0] < 0).all() and (d[a_front['ref']['face_ids'][0] == 1] > 0).all()      # a negative depth is nearer
    tie = RC.case('coincident')['ref']
    assert set(np.unique(tie['face_ids']).tolist()) == {-1, 0}                                                        # equal depths: the lower id
    both = RC.case('interpenetrating_wh16')['ref']
    overlap = (RC.pair_expected_ids(0)[0] == 0) & (RC.pair_expected_ids(1)[0] == 1)
    assert overlap.sum() == 15 and set(np.unique(both['face_ids'][0][overlap]).tolist()) == {0, 1}                  # each face in front somewhere


@pytest.mark.parametrize('name', [n for n in RC.CASES if n != 'smpl_wh64'])
def test_mask_equals_the_silhouette_restatement(name):
    c = RC.case(name)
    if c['rotation'] is not None:
        pt = c['ref']['pt']                                  # (the silhouette of the rotated vertices)
        want = EC.wp_silhouette(pt, c['faces'], c['cam'], c['wh'])
    else:
        want = EC.wp_silhouette(c['verts'], c['faces'], c['cam'], c['wh'])
    assert np.array_equal(c['ref']['mask'], want), name
    assert np.array_equal(c['ref']['face_ids'] >= 0, want != 0)


def test_mask_of_the_synthetic_smpl_mesh_equals_the_silhouette_restatement():
    c = RC.case('smpl_wh64')
    assert c['faces'].shape == (13776, 3) and c['rotation'] is None
    assert np.array_equal(c['ref']['mask'], EC.wp_silhouette(c['verts'], c['faces'], c['cam'], 64))
    assert 0 < c['ref']['mask'].sum() < 64 * 64 and (c['ref']['depth'] < 0).any() and ((c['ref']['depth'] > 0) & np.isfinite(c['ref']['depth'])).any()


def _brute_force_table(faces, N):
    offsets, table = [0], []
    for v in range(N):
        for f in range(len(faces)):
            tri = [int(i) for i in faces[f]]
            if v in tri and all(0 <= i < N for i in tri):
                table.append(f)
        offsets.append(len(table))
    return np.array(offsets, np.int32), np.array(table, np.int32)


@pytest.mark.parametrize('name', ['hand_index_out_of_range_wh16', 'hand_degenerate_wh16', 'blob_wh16', 'sphere_wh16', 'grid257_wh16', 'unreferenced_vertex',
                                  'out_of_range_face', 'no_normal'])
def test_host_table_equals_brute_force(name):
    c = RC.case(name)
    N = c['num_vertices']
    want = _brute_force_table(c['faces'], N)
    for got in (straps_amd.vertex_face_table(c['faces'], N), RC.csr_table(c['faces'], N)):
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].shape == (N + 1,)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    if name == 'unreferenced_vertex':
        assert want[0][5] == want[0][6] and want[0][N - 1] == want[0][N]
    if name == 'out_of_range_face':
        assert not set(want[1].tolist()) & {7, 16, 17} and want[0][N] == 3 * (len(c['faces']) - 3)
    if name == 'hand_degenerate_wh16':
        assert want[1].tolist() == [0, 1, 0, 1, 0]                    # face 1 = (0, 0, 1) is listed once for vertex 0
    # more vertices than the mesh has (a face that was out of range may now be in range: the brute-force table says)
    off, tab = straps_amd.vertex_face_table(c['faces'], N + 3)
    wide = _brute_force_table(c['faces'], N + 3)
    assert off.shape == (N + 4,) and np.array_equal(off, wide[0]) and np.array_equal(tab, wide[1])


def test_depth_key_orders_floats_and_round_trips():
    z = np.array([-np.inf, -3.4e38, -1.0, -1e-30, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 0.5, 1.0, 3.4e38, np.inf], np.float32)
    k = RC.depth_key32(z)
    assert (np.diff(k.astype(np.int64)) > 0).all()                  # -0 sorts directly below +0: distinct keys, the order of the bits
    assert np.array_equal(RC.key_depth32(k).view(np.uint32), z.view(np.uint32))
    assert (k != 0xFFFFFFFF).all()
    r = EC.det_uniform((4096,), 5, -2.0, 2.0)
    assert np.array_equal(np.argsort(RC.depth_key32(r), kind='stable'), np.argsort(r, kind='stable'))


def test_flip_is_the_winding_seen_from_the_camera():
    """the two windings of the same triangle draw the same pixels at the same depth; one of them is flipped, and the float64 colours agree"""
    a, b = RC.case('hand_right_triangle_wh16'), RC.case('hand_reversed_winding_wh16')
    assert np.array_equal(a['ref']['mask'], b['ref']['mask'])
    assert a['ref']['flip'][a['ref']['mask'] == 1].all() and not b['ref']['flip'].any()
    assert np.array_equal(RC.oracle('hand_right_triangle_wh16', 'other')['rgb'], RC.oracle('hand_reversed_winding_wh16', 'other')['rgb'])
    out, inw = RC.case('sphere_wh20'), RC.case('sphere_inward_wh20')
    assert np.array_equal(out['ref']['mask'], inw['ref']['mask']) and not out['ref']['flip'].any() and inw['ref']['flip'][inw['ref']['mask'] == 1].all()
    assert np.array_equal(RC.oracle('sphere_wh20', 'other')['rgb'], RC.oracle('sphere_inward_wh20', 'other')['rgb'])
    lit = RC.oracle('sphere_wh20', 'other')['rgb'][0][out['ref']['mask'][0] == 1]
    assert len(np.unique(lit[:, 1])) > 30 and lit[:, 1].max() < 255      # a shaded ball, not a flat disc, nowhere saturated


@pytest.mark.parametrize('name', [n for n in RC.SHADED_CASES if n != 'no_normal'])
def test_shaded_meshes_meet_the_condition_of_the_colour_bound(name):
    """at every covered pixel the interpolated (un-normalised) normal is at least half as long as the longest of the winning face's three
    vertex normals: normalising it amplifies the float32 error of the vertex normals (some 1e-7 of their length) by at most 2, which keeps
    the float32 colour within about 1e-6 of the float64 one -- far below the 3.9e-3 between two byte levels, so the byte differs by at
    most one.  Mixed-winding meshes (the blob, the synthetic SMPL mesh) are not in this list: their colours are not compared."""
    c, o = RC.case(name), RC.oracle(name)
    hit = c['ref']['mask'] == 1
    assert c['shaded'] and not o['fallback'].any()
    if hit.any():
        ratio = o['normal_len'][hit] / o['incident_len'][hit]
        assert np.isfinite(ratio).all() and ratio.min() >= 0.5, (name, float(ratio.min()))
    assert np.isnan(o['normal_len'][~hit]).all()


def test_geometry_only_meshes_do_fail_that_condition():
    for name in ('blob_wh20', 'smpl_wh64'):
        c = RC.case(name)
        assert not c['shaded'] and name not in RC.SHADED_CASES
        o = RC.shade64(c['verts'], c['faces'], c['cam'], c['wh'], c['ref']['face_ids'], c['ref']['flip'])
        hit = c['ref']['mask'] == 1
        assert (o['normal_len'][hit] / o['incident_len'][hit]).min() < 0.5, name


def test_no_normal_case_takes_the_fallback_everywhere():
    c, o = RC.case('no_normal'), RC.oracle('no_normal', 'other')
    hit = c['ref']['mask'][0] == 1
    assert hit.sum() == 45 and not c['ref']['normals'].any()          # n + (-n) == 0 exactly, in float32 as well
    assert o['fallback'][0][hit].all()
    # the fallback (0, 0, -1) faces the viewer; where the winning face's own normal has positive z it is turned away like any other normal, and
    # only the ambient term is left there
    flip = c['ref']['flip'][0]
    assert flip[hit].any() and (~flip)[hit].any()
    amb = RC.quantise(np.float64(np.float32(RC.OTHER_OPTS['ambient'])) * np.asarray(RC.OTHER_OPTS['colour'], np.float32).astype(np.float64))
    assert (o['rgb'][0][hit & flip] == amb).all() and (o['rgb'][0][hit & ~flip] != amb).any()


def test_quantisation_and_background():
    assert RC.quantise([0.0, 1.0, 0.5, -3.0, 7.0, 0.3 * 0.8]).tolist() == [0, 255, 128, 0, 255, 61]
    assert RC.quantise32(np.float32(0.8) * np.float32(0.3)) == 61
    o = RC.oracle('hand_off_screen_wh16', 'other')
    assert (o['rgb'] == RC.quantise(np.asarray(RC.OTHER_OPTS['background'], np.float32))).all()
    bg = RC.background_image(1, 16)
    ob = RC.oracle('pair_b_in_front', 'default', True)
    hit = RC.case('pair_b_in_front')['ref']['mask'] == 1
    assert np.array_equal(ob['rgb'][~hit], bg[~hit]) and (ob['rgb'][hit] == (204, 77, 77)).all()      # 0.8, 0.3, 0.3 at full light (76.5 rounds up)
