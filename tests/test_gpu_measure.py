"""GPU: straps_measure_mesh (csrc/measure.hip) against the float64 restatement of tests/measure_cases.py.

The bound is derived, not measured: both sides read the same fp32 inputs and compute every term in double, so they differ by the summation
order and fused multiply-adds -- at most about nfaces * 2^-52 * S, S the sum of the absolute values of the terms -- and by the one rounding
to float: |gpu - oracle| <= 2^-23 |oracle| + 1e-10 S for every measurement of every case.  Every output and the workspace sit between
redzone margins; the operands end directly in front of poison.  Then isolation and reproducibility (bit for bit), and the module surface:
BodyMeasurer, from_smpl, Predictor.measure on the committed predict fixtures."""
import numpy as np
import pytest
import torch

import measure_cases as MC
import predict_cases as PC
import straps_amd
from measure_cases import AREA, EXTENT, GIRTH, PATH, VOLUME, measurement
from redzone import Zone
from straps_amd import hipabi, measure

pytestmark = pytest.mark.gpu
FPB, VPB = hipabi.MEASURE_FACES_PER_BLOCK, hipabi.MEASURE_VERTS_PER_BLOCK
MP = straps_amd.synthetic_mean_params(0)
MODEL = straps_amd.synthetic_smpl_model(0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _structs(meas):
    arr = (hipabi.MeasureStruct * len(meas))()
    for q, m in zip(arr, meas):
        q.kind = m['kind']
        q.anchor[:] = m['anchor']
        q.dir[:] = m['dir']
        q.part_mask = m['part_mask']
    return arr


def _measure(dev, verts, points, faces, parts, meas):
    """the raw call on a guarded output + workspace, operands ending in front of poison -> float32 [B,M] numpy"""
    B, N = verts.shape[0], verts.shape[1]
    F, M = faces.shape[0], len(meas)
    L = hipabi.lib()
    z = Zone(dev)
    out = z.guarded((B, M), name='out')
    ws_bytes = L.straps_measure_workspace_bytes(B, N, F, M)
    assert ws_bytes == B * M * 8 * ((F + FPB - 1) // FPB + 2 * ((N + VPB - 1) // VPB)) > 0
    ws = z.guarded((ws_bytes // 4,), name='workspace')
    assert ws.data_ptr() % 8 == 0
    put = lambda a: None if a is None or a.size == 0 else z.at_end(torch.from_numpy(np.ascontiguousarray(a)))
    v, p, f, fp = put(verts), put(points), put(faces), put(parts)
    hipabi.check(L.straps_measure_mesh(hipabi.ptr(v), hipabi.ptr(p), hipabi.ptr(f), hipabi.ptr(fp), _structs(meas), hipabi.ptr(out), hipabi.ptr(ws), B, N,
                                       0 if points is None else points.shape[1], F, M, hipabi.stream_ptr()), 'straps_measure_mesh')
    torch.cuda.synchronize()
    z.check()
    return out.cpu().numpy()


def _assert_parity(got, verts, points, faces, parts, meas, what):
    want, S = MC.oracle(verts, points, faces, parts, meas)
    assert got.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaNs sit elsewhere than in the restatement' % what
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-10 * S
    ok = nan | (err <= bound)
    worst = np.where(nan, 0.0, err / np.where(bound > 0, bound, 1.0))
    print('%s: %d values, worst error / bound %.3f' % (what, got.size, float(worst.max())))
    assert ok.all(), '%s: (body, measurement) %s outside the bound: got %r, oracle %r, bound %r' % (
        what, np.argwhere(~ok)[:4].tolist(), got[~ok][:4].tolist(), want[~ok][:4].tolist(), bound[~ok][:4].tolist())
    return want


@pytest.mark.parametrize('nfaces', (1, 63, 64, 65, 255, 256, 257, FPB - 1, FPB, FPB + 1, 2 * FPB + 1))
def test_face_counts_at_wave_and_block_edges(dev, nfaces):
    """batch 3, 32 measurements with the five kinds interleaved, 7 points: anchors on vertices and on points, PATHs with 2, 3 and 4 anchors"""
    verts, points, faces, parts = MC.soup(3, 97, nfaces, n_points=7, seed=nfaces)
    meas = MC.mixed_measurements(32, 97, 7, seed=nfaces)
    assert sorted(set(q['kind'] for q in meas)) == [0, 1, 2, 3, 4] and set(sum(a >= 0 for a in q['anchor']) for q in meas if q['kind'] == PATH) == {2, 3, 4}
    got = _measure(dev, verts, points, faces, parts, meas)
    want = _assert_parity(got, verts, points, faces, parts, meas, 'nfaces %d' % nfaces)
    if nfaces >= 255:
        assert (want[:, [m for m, q in enumerate(meas) if q['kind'] == GIRTH and q['part_mask'] == 0]] > 0).any()


@pytest.mark.parametrize('nverts', (3, 64, VPB - 1, VPB, VPB + 1))
@pytest.mark.parametrize('planted', ('max_last', 'min_last'))
def test_vertex_counts_at_block_edges(dev, nverts, planted):
    """the extent's maximum planted in the last vertex and its minimum in the first, and the other way round; batch 1"""
    verts, points, faces, parts = MC.soup(1, nverts, 65, n_points=1, seed=nverts)
    hi, lo = (nverts - 1, 0) if planted == 'max_last' else (0, nverts - 1)
    verts[0, hi], verts[0, lo] = (2.0, 5.0, 3.0), (-4.0, -7.0, -1.0)
    meas = [measurement(EXTENT, direction=(0, 1, 0)), measurement(EXTENT, direction=(1, 0, 0)), measurement(EXTENT, direction=(0, 0, -2)),
            measurement(EXTENT, direction=(0.3, 0.5, 0.1)), measurement(AREA), measurement(GIRTH, (nverts,), (0, 1, 0)), measurement(PATH, (nverts - 1, nverts, 0))]
    got = _measure(dev, verts, points, faces, parts, meas)
    _assert_parity(got, verts, points, faces, parts, meas, 'nverts %d %s' % (nverts, planted))
    assert got[0, :3].tolist() == [12.0, 6.0, 8.0]


@pytest.mark.parametrize('batch', (1, 3))
@pytest.mark.parametrize('n_points', (0, 1, 64))
def test_single_measurements_and_point_counts(dev, batch, n_points):
    """n_meas == 1, one call per kind (an EXTENT or PATH alone launches no face block, a face kind alone no vertex block)"""
    verts, points, faces, parts = MC.soup(batch, 130, 300, n_points=n_points, seed=10 * batch + n_points)
    for q in MC.single_measurements(130, n_points):
        got = _measure(dev, verts, points, faces, parts, [q])
        want = _assert_parity(got, verts, points, faces, parts, [q], 'batch %d, %d points, kind %d alone' % (batch, n_points, q['kind']))
        assert (want != 0).any()
    if n_points:
        meas = MC.mixed_measurements(32, 130, n_points, seed=n_points)
        assert max(max(q['anchor']) for q in meas) == 130 + n_points - 1
        _assert_parity(_measure(dev, verts, points, faces, parts, meas), verts, points, faces, parts, meas, 'batch %d, %d points, 32 mixed' % (batch, n_points))
    # no faces at all: allowed when nothing reads them
    meas = [measurement(EXTENT, direction=(0, 1, 0)), measurement(PATH, (0, 129, 64, 1))]
    none = np.zeros((0, 3), np.int32)
    _assert_parity(_measure(dev, verts, points, none, None, meas), verts, points, none, None, meas, 'no faces')


def test_paths_with_two_three_and_four_anchors(dev):
    verts, points, faces, parts = MC.soup(3, 40, 9, n_points=5, seed=5)
    meas = [measurement(PATH, (0, 39)), measurement(PATH, (40, 44)), measurement(PATH, (3, 41, 17)), measurement(PATH, (44, 43, 42, 41)), measurement(PATH, (7, 7)),
            measurement(PATH, (1, 2, -1, 5))]
    got = _measure(dev, verts, points, faces, parts, meas)
    want = _assert_parity(got, verts, points, faces, parts, meas, 'paths')
    assert (got[:, 4] == 0).all() and (want[:, :4] > 0).all()
    v64 = verts.astype(np.float64)
    assert np.allclose(want[:, 5], np.linalg.norm(v64[:, 2] - v64[:, 1], axis=1), rtol=1e-15)      # the entry behind the first -1 is not read


def test_special_cases(dev):
    v, f, parts = MC.prism(6, 0.5, 1.0)
    verts = np.stack([v, v * 1.5, v + 0.25]).astype(np.float32)
    N = v.shape[0]
    points = np.tile(np.array([[[0.0, 9.0, 0.0], [0.0, 0.1, 0.0]]], np.float32), (3, 1, 1))
    odd = parts.copy()
    odd[:6] = (32, 33, 64, 255, 128, 40)
    # a part mask that selects nothing; a plane that misses; a plane that misses the selected part
    meas = [measurement(VOLUME, part_mask=1 << 9), measurement(AREA, part_mask=1 << 31), measurement(GIRTH, (N + 1,), (0, 1, 0), 1 << 9),
            measurement(GIRTH, (N,), (0, 1, 0)), measurement(GIRTH, (N + 1,), (0, 1, 0), 1 << 3), measurement(GIRTH, (N + 1,), (0, 1, 0)), measurement(AREA)]
    got = _measure(dev, verts, points, f, parts, meas)
    _assert_parity(got, verts, points, f, parts, meas, 'nothing selected / plane misses')
    assert (got[:, :5] == 0).all() and not np.signbit(got[:, :5]).any() and (got[:2, 5] > 0).all()
    # faces with an index out of range are skipped: appended, so that every other face keeps its thread, the results keep their bits
    bad = np.concatenate([f, [[0, 1, N], [-1, 2, 3], [4, 1 << 30, 5], [N, N, N]]]).astype(np.int32)
    bad_parts = np.concatenate([parts, [1, 1, 1, 1]]).astype(np.uint8)
    meas = [measurement(VOLUME), measurement(AREA), measurement(GIRTH, (N + 1,), (0.1, 1, 0)), measurement(AREA, part_mask=1 << 1)]
    with_bad, without = _measure(dev, verts, points, bad, bad_parts, meas), _measure(dev, verts, points, f, parts, meas)
    assert np.array_equal(with_bad.view(np.uint32), without.view(np.uint32))
    _assert_parity(with_bad, verts, points, bad, bad_parts, meas, 'out-of-range faces')
    # a label >= 32 is never selected by a non-zero mask (and is by mask 0)
    meas = [measurement(AREA, part_mask=0xffffffff), measurement(AREA), measurement(AREA, part_mask=1 << 0), measurement(VOLUME, part_mask=0xffffffff)]
    got = _measure(dev, verts, points, f, odd, meas)
    want = _assert_parity(got, verts, points, f, odd, meas, 'labels >= 32')
    assert (got[:, 0] < got[:, 1]).all() and (got[:, 2] == 0).all()
    assert np.allclose(want[0, 1] - want[0, 0], 6 * (0.5 * 0.5 * 1.0), rtol=1e-6)      # six side triangles of the hexagonal prism: base r = 0.5, height h = 1


@pytest.fixture(scope='module')
def body_set():
    b = MC.bodies()
    meas = MC.from_specs(list(measure.default_measurements().values()), b['verts'].shape[1])
    return b, meas


def test_full_size_bodies_with_the_default_measurements(dev, body_set):
    b, meas = body_set
    assert b['verts'].shape == (3, 6890, 3) and b['faces'].shape == (13776, 3) and len(meas) == 15
    got = _measure(dev, b['verts'], b['joints'], b['faces'], b['face_parts'], meas)
    want = _assert_parity(got, b['verts'], b['joints'], b['faces'], b['face_parts'], meas, 'synthetic bodies, defaults')
    assert (want[:, [0, 2]] > 0).all() and (want[:, 3:] > 0).all()


def test_isolation_and_reproducibility(dev, body_set):
    b, meas = body_set
    meas = meas + [measurement(PATH, (4000, 77)), measurement(GIRTH, (4000,), (0, 1, 0)), measurement(EXTENT, direction=(1, 0, 0))]
    args = (b['joints'], b['faces'], b['face_parts'], meas)
    clean = _measure(dev, b['verts'], *args)
    again = _measure(dev, b['verts'], *args)
    assert np.array_equal(clean.view(np.uint32), again.view(np.uint32)), 'two runs of the same call differ'
    # a body's row alone and inside the batch
    for k in range(3):
        alone = _measure(dev, b['verts'][k:k + 1], b['joints'][k:k + 1], *args[1:])
        assert np.array_equal(alone.view(np.uint32), clean[k:k + 1].view(np.uint32)), 'body %d differs between batch 1 and batch 3' % k
    # a NaN vertex in body 1
    dirty = b['verts'].copy()
    dirty[1, 4000] = np.nan
    got = _measure(dev, dirty, *args)
    assert np.array_equal(got[[0, 2]].view(np.uint32), clean[[0, 2]].view(np.uint32)), 'a NaN in body 1 changed another body'
    _assert_parity(got, dirty, *args, 'NaN vertex in body 1')
    names = list(measure.default_measurements())
    hit = [names.index('height'), names.index('volume'), names.index('surface_area'), 15, 17]      # the sums over all faces / vertices, and the path from the vertex
    assert np.isnan(got[1, hit]).all() and not np.isnan(got[[0, 2]]).any()
    assert got[1, 16] == 0                   # a plane through a NaN anchor has no positive side (d >= 0 is false for a NaN): it cuts nothing, as defined
    untouched = [names.index(n) for n in names if 'length' in n or 'breadth' in n]                    # paths between joints: the vertex is not read
    assert np.array_equal(got[1, untouched].view(np.uint32), clean[1, untouched].view(np.uint32))


# ---- through the modules -----------------------------------------------------------------------------------------------------------
def test_body_measurer_equals_the_raw_call(dev, body_set):
    b, meas = body_set
    raw = _measure(dev, b['verts'], b['joints'], b['faces'], b['face_parts'], meas)
    m = straps_amd.BodyMeasurer(b['faces'], b['face_parts']).to(dev)
    assert m.faces.is_cuda and m.face_parts.is_cuda
    v, j = torch.from_numpy(b['verts']).to(dev), torch.from_numpy(b['joints']).to(dev)
    res = m(v, j)
    assert list(res) == ['values'] + list(measure.default_measurements())
    assert res['values'].dtype == torch.float32 and tuple(res['values'].shape) == (3, 15)
    assert np.array_equal(res['values'].cpu().numpy().view(np.uint32), raw.view(np.uint32))
    for i, n in enumerate(m.names):
        assert tuple(res[n].shape) == (3,) and res[n].data_ptr() == res['values'][:, i].data_ptr() and torch.equal(res[n], res['values'][:, i])
    # more joints than are read (SMPL.forward_arrays gives 90), and a strided view
    wide = torch.zeros(3, 90, 3, device=dev)
    wide[:, :24] = j
    assert torch.equal(m(v, wide)['values'], res['values'])
    assert torch.equal(m(torch.cat([v, v], 2)[:, :, :3], j)['values'], res['values'])
    # own specs: vertex anchors only need no joints
    own = straps_amd.BodyMeasurer(b['faces'], None, {'vol': measure.volume(about=5), 'span': measure.extent((1, 0, 0)), 'ring': measure.girth(4000, (0, 1, 0)),
                                                    'hop': measure.path(1, 2, 3)}).to(dev)
    o = own(v)
    own_meas = [measurement(VOLUME, (5,)), measurement(EXTENT, direction=(1, 0, 0)), measurement(GIRTH, (4000,), (0, 1, 0)), measurement(PATH, (1, 2, 3))]
    assert np.array_equal(o['values'].cpu().numpy().view(np.uint32), _measure(dev, b['verts'], None, b['faces'], None, own_meas).view(np.uint32))
    with pytest.raises(RuntimeError, match='joints'):
        m(v)
    with pytest.raises(RuntimeError, match='joints'):
        m(v, j[:, :21])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        m(v.cpu(), j)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        m(v, j.cpu())
    with pytest.raises(RuntimeError, match='GPU tensor'):
        straps_amd.BodyMeasurer(b['faces'], b['face_parts'])(v, j)                  # buffers still on the host
    with pytest.raises(RuntimeError, match='vertex 4000'):
        own(v[:, :100].contiguous())
    with pytest.raises(RuntimeError, match='face_parts'):
        straps_amd.BodyMeasurer(b['faces'], None)


@pytest.fixture(scope='module')
def prediction(dev):
    """the seeded regressor and inputs of tests/test_gpu_predictor.py: three frames of the committed predict fixtures"""
    B = 3
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP).to(dev).eval()
    smpl = straps_amd.SMPL(MODEL, batch_size=B).to(dev)
    sil, joints = PC.inputs('a')
    pred = straps_amd.Predictor(reg, smpl)
    args = (torch.from_numpy(sil[:B]).to(dev), torch.from_numpy(joints[:B]).to(dev))
    return pred, smpl, args


def test_predictor_measure(dev, prediction):
    pred, smpl, args = prediction
    before = pred(*args)
    kept = {k: v.clone() for k, v in before.items()}
    measurer = straps_amd.BodyMeasurer.from_smpl(smpl).to(dev)
    assert measurer.faces.shape[0] == 13776 and measurer.names == tuple(measure.default_measurements())
    m = pred.measure(before, measurer)
    # `out` is untouched, and a Predictor call after the method ran gives the bits of the call before it
    assert set(before) == set(kept)
    bits = lambda t: t.contiguous().view(torch.uint8)
    for k in kept:
        assert torch.equal(bits(before[k]), bits(kept[k])), k
    after = pred(*args)
    assert set(after) == set(kept)
    for k in kept:
        assert after[k].dtype == kept[k].dtype and torch.equal(bits(after[k]), bits(kept[k])), k
    # equals BodyMeasurer on the reposed vertices with the T-pose joints
    B = before['shape'].shape[0]
    eye = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    tverts, tjoints = smpl.forward_arrays(before['shape'].contiguous(), eye)
    assert torch.equal(tverts, before['reposed_vertices'])
    direct = measurer(before['reposed_vertices'], tjoints)
    assert list(m) == list(direct) == ['values'] + list(measurer.names)
    for k in m:
        assert torch.equal(m[k], direct[k]), k
    vals = m['values'].cpu().numpy()
    meas = MC.from_specs(measurer.specs, 6890)
    rv, tj = before['reposed_vertices'].cpu().numpy(), tjoints[:, :24].cpu().numpy()
    _assert_parity(vals, rv, tj, MODEL['faces'], MODEL['face_parts'], meas, 'Predictor.measure')
    assert np.isfinite(vals).all() and (vals[:, 0] > 1.0).all()
    # on the result of refine as well
    fitted = pred.refine(before, straps_amd.KeypointFitter(smpl, iters=2))
    fm = pred.measure(fitted, measurer)
    _, fj = smpl.forward_arrays(fitted['shape'].contiguous(), eye)
    assert torch.equal(fm['values'], measurer(fitted['reposed_vertices'], fj)['values'])
