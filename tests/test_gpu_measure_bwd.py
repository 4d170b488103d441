"""GPU: straps_measure_mesh_bwd (csrc/measure_bwd.hip) against the float64 autograd restatement of tests/measure_grad_cases.py.

The bound is the forward's (tests/measure_cases.py), derived, not measured: |got - want| <= 2^-23 |want| + 1e-10 S per output element, S the sum
of |dout_m| x |contribution| over the terms added into it.  Every case asserts, on the CPU, the conditions under which a gradient is well
defined to the last bit (measure_grad_cases.assert_conditions); the seeds below were chosen so that they hold.  Every output and the workspace
sit between redzone margins; the operands end directly in front of poison.  Then isolation, reproducibility and graph replay (bit for bit),
and the argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import measure_cases as MC
import measure_grad_cases as GC
import straps_amd
from measure_cases import AREA, EXTENT, GIRTH, PATH, VOLUME, measurement
from redzone import Zone
from straps_amd import hipabi, measure
from straps_amd.nmr_renderer import vertex_face_table

pytestmark = pytest.mark.gpu
FPB, VPB = hipabi.MEASURE_FACES_PER_BLOCK, hipabi.MEASURE_VERTS_PER_BLOCK
EINVAL = 1
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


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


class Call:
    """the raw call on guarded outputs + workspace, operands ending in front of poison; dpoints has `extra` rows behind the n_points that are
    written, pre-filled (as every guarded body) with NaN"""

    def __init__(self, dev, verts, points, faces, parts, meas, dout, extra=0):
        self.B, self.N = verts.shape[0], verts.shape[1]
        self.F, self.M = faces.shape[0], len(meas)
        self.P = 0 if points is None else points.shape[1]
        self.rows = self.P + extra
        L = hipabi.lib()
        self.z = z = Zone(dev)
        self.dverts = z.guarded((self.B, self.N, 3), name='dverts')
        self.dpoints = z.guarded((self.B, self.rows, 3), name='dpoints') if self.rows else None
        ws_bytes = L.straps_measure_bwd_workspace_bytes(self.B, self.N, self.F, self.M)
        assert ws_bytes == self.B * self.M * 8 * (3 * ((self.F + FPB - 1) // FPB) + 4 * ((self.N + VPB - 1) // VPB)) > 0
        self.ws = z.guarded((ws_bytes // 4,), name='workspace')
        assert self.ws.data_ptr() % 8 == 0
        put = lambda a: None if a is None or a.size == 0 else z.at_end(torch.from_numpy(np.ascontiguousarray(a)))
        off, vf = vertex_face_table(faces, self.N)
        self.ops = [put(verts), put(points), put(faces), put(parts), put(off), put(vf)]
        self.dout = put(np.asarray(dout, np.float32))
        self.meas = _structs(meas)

    def run(self):
        v, p, f, fp, off, vf = self.ops
        hipabi.check(hipabi.lib().straps_measure_mesh_bwd(hipabi.ptr(v), hipabi.ptr(p), hipabi.ptr(f), hipabi.ptr(fp), hipabi.ptr(off), hipabi.ptr(vf), self.meas,
                                                          hipabi.ptr(self.dout), hipabi.ptr(self.dverts), hipabi.ptr(self.dpoints), hipabi.ptr(self.ws), self.B, self.N,
                                                          self.P, self.rows, self.F, self.M, hipabi.stream_ptr()), 'straps_measure_mesh_bwd')

    def result(self):
        torch.cuda.synchronize()
        self.z.check()
        dp = np.zeros((self.B, 0, 3), np.float32)
        if self.dpoints is not None:
            full = self.dpoints.cpu().numpy()
            assert np.isnan(full[:, self.P:]).all(), 'rows of dpoints behind n_points were written'
            dp = full[:, :self.P]
        return self.dverts.cpu().numpy(), dp


def _bwd(dev, verts, points, faces, parts, meas, dout, extra=0):
    c = Call(dev, verts, points, faces, parts, meas, dout, extra)
    c.run()
    return c.result()


def _assert_parity(got, verts, points, faces, parts, meas, dout, what, allow_extent_ties=False):
    GC.assert_conditions(verts, points, faces, parts, meas, allow_extent_ties)
    want_v, want_p, S_v, S_p = GC.oracle_grad(verts, points, faces, parts, meas, dout)
    worst = 0.0
    for name, g, want, S in (('dverts', got[0], want_v, S_v), ('dpoints', got[1], want_p, S_p)):
        assert g.dtype == np.float32 and g.shape == want.shape, (name, g.shape, want.shape)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g), nan), '%s: NaNs of %s sit elsewhere than in the restatement' % (what, name)
        err = np.abs(g.astype(np.float64) - want)
        bound = 2.0 ** -23 * np.abs(want) + 1e-10 * S
        ok = nan | (err <= bound)
        if g.size:
            worst = max(worst, float(np.where(nan | (bound == 0), 0.0, err / np.where(bound > 0, bound, 1.0)).max()))
        assert ok.all(), '%s: %s %s outside the bound: got %r, oracle %r, bound %r' % (
            what, name, np.argwhere(~ok)[:4].tolist(), g[~ok][:4].tolist(), want[~ok][:4].tolist(), bound[~ok][:4].tolist())
    print('%s: %d elements, worst error / bound %.3f' % (what, got[0].size + got[1].size, worst))
    return want_v, want_p


# the seed of every soup case: one at which assert_conditions and the S == 0 rule of measure_grad_cases hold (both are asserted again in every run;
# a case that fails them gets another seed here, it is never skipped)
FACE_SEEDS = {1: 1, FPB - 1: 511, FPB: 512, FPB + 1: 513, 2 * FPB + 1: 1025}


@pytest.mark.parametrize('nfaces', sorted(FACE_SEEDS))
def test_face_counts_at_block_edges(dev, nfaces):
    """batch 3, 32 measurements with the five kinds interleaved and part masks, 7 points: anchors on vertices and on points"""
    seed = FACE_SEEDS[nfaces]
    verts, points, faces, parts = MC.soup(3, 97, nfaces, n_points=7, seed=seed)
    meas = MC.mixed_measurements(32, 97, 7, seed=seed)
    dout = GC.random_dout(3, 32, seed)
    assert (dout == 0).any() and (dout < 0).any() and any(q['part_mask'] for q in meas)
    got = _bwd(dev, verts, points, faces, parts, meas, dout, extra=3)
    want_v, want_p = _assert_parity(got, verts, points, faces, parts, meas, dout, 'nfaces %d' % nfaces)
    assert (want_p != 0).any() and (want_v != 0).any()


@pytest.mark.parametrize('nverts', (1, VPB - 1, VPB, VPB + 1))
def test_vertex_counts_at_block_edges(dev, nverts):
    """batch 1; the extent's maximum planted in the last vertex and its minimum in the first"""
    if nverts == 1:
        verts, points = np.array([[[0.25, -0.5, 0.125]]], np.float32), np.array([[[0.5, 0.25, -0.25]]], np.float32)
        faces, parts = np.zeros((1, 3), np.int32), np.array([1], np.uint8)
        meas = [measurement(EXTENT, direction=(0.3, 0.5, 0.1)), measurement(PATH, (0, 1)), measurement(GIRTH, (1,), (0, 1, 0)), measurement(AREA)]
    else:
        verts, points, faces, parts = MC.soup(1, nverts, 65, n_points=1, seed=nverts)
        verts[0, nverts - 1], verts[0, 0] = (2.0, 5.0, 3.0), (-4.0, -7.0, -1.0)
        meas = [measurement(EXTENT, direction=(0, 1, 0)), measurement(EXTENT, direction=(1, 0, 0)), measurement(EXTENT, direction=(0, 0, -2)),
                measurement(EXTENT, direction=(0.3, 0.5, 0.1)), measurement(AREA), measurement(GIRTH, (nverts,), (0, 1, 0)), measurement(PATH, (nverts - 1, nverts, 0)),
                measurement(VOLUME, (nverts - 1,))]
    dout = GC.random_dout(1, len(meas), seed=nverts) + np.float32(0.5)
    got = _bwd(dev, verts, points, faces, parts, meas, dout)
    _assert_parity(got, verts, points, faces, parts, meas, dout, 'nverts %d' % nverts)


BATCH_SEEDS = {1: 0, 3: 0, 257: 0}


@pytest.mark.parametrize('batch', sorted(BATCH_SEEDS))
def test_batches(dev, batch):
    seed = BATCH_SEEDS[batch]
    verts, points, faces, parts = MC.soup(batch, 50, 130, n_points=2, seed=seed)
    meas = MC.mixed_measurements(10, 50, 2, seed=seed)
    dout = GC.random_dout(batch, 10, seed)
    got = _bwd(dev, verts, points, faces, parts, meas, dout)
    _assert_parity(got, verts, points, faces, parts, meas, dout, 'batch %d' % batch)


@pytest.mark.parametrize('n_points', (0, 1, 64))
def test_each_kind_alone_and_point_counts(dev, n_points):
    """n_meas == 1, one call per kind (no face block without a GIRTH or centred VOLUME, no vertex block without an EXTENT)"""
    verts, points, faces, parts = MC.soup(3, 130, 300, n_points=n_points, seed=30 + n_points)
    for q in MC.single_measurements(130, n_points) + [measurement(VOLUME, (130 + n_points - 1,), part_mask=0x36)]:
        dout = np.array([[1.5], [-0.75], [0.0]], np.float32)
        got = _bwd(dev, verts, points, faces, parts, [q], dout, extra=2 if n_points else 0)
        want_v, _ = _assert_parity(got, verts, points, faces, parts, [q], dout, '%d points, kind %d alone' % (n_points, q['kind']))
        assert (want_v[:2] != 0).any() and not got[0][2].any() and not np.signbit(got[0][2]).any()      # dout == 0: +0 everywhere
    # no faces at all: allowed when nothing reads them, and then without the vertex-to-face table
    meas = [measurement(EXTENT, direction=(0, 1, 0)), measurement(PATH, (0, 129, 64, 1))]
    none = np.zeros((0, 3), np.int32)
    dout = GC.random_dout(3, 2, 1) + np.float32(3)
    _assert_parity(_bwd(dev, verts, points, none, None, meas, dout), verts, points, none, None, meas, dout, 'no faces')


def _fan():
    """vertex 0 in the middle of a fan of 300 faces (ring 1..300, the last face closes it), vertex 301 with no incident face"""
    rng = np.random.RandomState(77)
    phi = 2 * np.pi * (np.arange(300) + rng.uniform(-0.3, 0.3, 300)) / 300
    ring = np.stack([0.4 * np.cos(phi), rng.uniform(-0.3, 0.3, 300), 0.4 * np.sin(phi)], 1)
    verts = np.concatenate([[[0.013, 0.021, -0.017]], ring, [[0.7, 0.9, 0.1]]]).astype(np.float32)[None]
    faces = np.array([(0, 1 + i, 1 + (i + 1) % 300) for i in range(300)], np.int32)
    parts = (np.arange(300) % 5).astype(np.uint8)
    return verts, faces, parts


def test_fan_isolated_vertex_shared_anchors_and_an_anchor_that_is_an_extreme(dev):
    verts, faces, parts = _fan()
    points = np.array([[[0.05, 0.02, 0.01], [0.3, -0.2, 0.1]]], np.float32)
    N = verts.shape[1]
    # vertex 0 anchors two GIRTHs, a VOLUME and a PATH; vertex 301 (no face) is the maximum of the y extent, anchors a VOLUME and ends a PATH
    meas = [measurement(GIRTH, (0,), (0.2, 1.0, 0.1)), measurement(GIRTH, (0,), (1, 0, 0), 0b10110), measurement(VOLUME, (0,)), measurement(PATH, (0, 301, N + 1)),
            measurement(EXTENT, direction=(0, 1, 0)), measurement(VOLUME, (301,)), measurement(AREA), measurement(GIRTH, (N,), (0, 1, 0)), measurement(VOLUME),
            measurement(PATH, (5, 5, 7)), measurement(EXTENT, direction=(1, 0, 0))]
    dout = GC.random_dout(1, len(meas), 9) + np.float32(0.25)
    got = _bwd(dev, verts, points, faces, parts, meas, dout, extra=88)
    want_v, _ = _assert_parity(got, verts, points, faces, parts, meas, dout, 'fan')
    assert np.argmax(verts[0, :, 1]) == 301 and (want_v[0, 301] != 0).all() and (want_v[0, 0] != 0).all()


def test_repeated_and_out_of_range_indices(dev):
    verts, points, faces, parts = MC.soup(3, 97, 300, n_points=4, seed=3)
    meas = MC.mixed_measurements(32, 97, 4, seed=3)
    dout = GC.random_dout(3, 32, 3)
    clean = _bwd(dev, verts, points, faces, parts, meas, dout)
    # appended, so that every other face keeps its place in the table's lists: out-of-range faces change no bit
    bad = np.concatenate([faces, [[0, 1, 97], [-1, 2, 3], [4, 1 << 30, 5], [97, 97, 97]]]).astype(np.int32)
    bad_parts = np.concatenate([parts, [1, 1, 1, 1]]).astype(np.uint8)
    with_bad = _bwd(dev, verts, points, bad, bad_parts, meas, dout)
    assert np.array_equal(bits(with_bad[0]), bits(clean[0])) and np.array_equal(bits(with_bad[1]), bits(clean[1]))
    # faces that name a vertex twice and three times
    rep = np.concatenate([faces, [[5, 5, 9], [9, 5, 9], [7, 7, 7], [11, 12, 11]]]).astype(np.int32)
    rep_parts = np.concatenate([parts, [1, 2, 3, 4]]).astype(np.uint8)
    assert (MC.soup(3, 97, 300, 4, 3)[2][:, 0] == MC.soup(3, 97, 300, 4, 3)[2][:, 1]).any(), 'the soup itself repeats indices'
    _assert_parity(_bwd(dev, verts, points, rep, rep_parts, meas, dout), verts, points, rep, rep_parts, meas, dout, 'repeated indices')


def test_extent_tie_goes_to_the_lowest_index(dev):
    verts, points, faces, parts = MC.soup(2, VPB + 40, 65, n_points=0, seed=12)
    for b in range(2):
        verts[b, [7, 300, VPB + 3], 1] = 3.0                  # three maxima, in two vertex blocks
        verts[b, [VPB + 30, 90], 1] = -3.0                    # two minima, the lower index in the first block
    meas = [measurement(EXTENT, direction=(0, 1, 0)), measurement(EXTENT, direction=(0, -2, 0))]
    dout = np.array([[1.0, 0.0], [0.5, -0.25]], np.float32)
    got = _bwd(dev, verts, points, faces, parts, meas, dout)
    _assert_parity(got, verts, points, faces, parts, meas, dout, 'extent ties', allow_extent_ties=True)
    assert got[0][0, 7].tolist() == [0, 1, 0] and got[0][0, 90].tolist() == [0, -1, 0] and np.count_nonzero(got[0][0]) == 2
    assert got[0][1, 7].tolist() == [0, 0, 0] and got[0][1, 90].tolist() == [0, 0, 0]      # 0.5 (0, 1, 0) - (-0.25) (0, -2, 0), and the reverse


@pytest.fixture(scope='module')
def body_set():
    b = MC.bodies(betas_seed=1)      # (seed 0 puts a vertex of body 2 at 1.7e-6 m from the upper-arm plane: assert_conditions)
    meas = MC.from_specs(list(measure.default_measurements().values()), b['verts'].shape[1])
    dout = GC.random_dout(3, len(meas), 5) + np.float32(0.125)
    return b, meas, dout


def test_full_size_bodies_with_the_default_measurements(dev, body_set):
    b, meas, dout = body_set
    got = _bwd(dev, b['verts'], b['joints'], b['faces'], b['face_parts'], meas, dout, extra=90 - 24)
    want_v, want_p = _assert_parity(got, b['verts'], b['joints'], b['faces'], b['face_parts'], meas, dout, 'synthetic bodies, defaults')
    assert (np.abs(want_p[:, [0, 3, 9, 4, 5, 18, 19, 16, 17]]).sum(2) > 0).all()


def test_isolation_reproducibility_and_graph_replay(dev, body_set):
    b, meas, dout = body_set
    meas = meas + [measurement(PATH, (4000, 77)), measurement(GIRTH, (4000,), (0, 1, 0)), measurement(EXTENT, direction=(1, 0, 0))]
    dout = np.concatenate([dout, [[0.5, -1.0, 2.0]] * 3], 1).astype(np.float32)
    args = (b['faces'], b['face_parts'], meas)
    clean = _bwd(dev, b['verts'], b['joints'], *args, dout)
    again = _bwd(dev, b['verts'], b['joints'], *args, dout)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(clean, again)), 'two runs of the same call differ'
    for k in range(3):
        alone = _bwd(dev, b['verts'][k:k + 1], b['joints'][k:k + 1], *args, dout[k:k + 1])
        assert all(np.array_equal(bits(x), bits(y[k:k + 1])) for x, y in zip(alone, clean)), 'body %d differs between batch 1 and batch 3' % k
    # a NaN vertex in body 1: its own rows may hold NaNs, the neighbours keep their bits
    dirty = b['verts'].copy()
    dirty[1, 4000] = np.nan
    got = _bwd(dev, dirty, b['joints'], *args, dout)
    assert all(np.array_equal(bits(x[[0, 2]]), bits(y[[0, 2]])) for x, y in zip(got, clean)), 'a NaN in body 1 changed another body'
    assert np.isnan(got[0][1]).any() and not np.isnan(got[0][[0, 2]]).any() and not np.isnan(got[1][[0, 2]]).any()
    # graph capture and replay against eager
    c = Call(dev, b['verts'], b['joints'], *args, dout)
    c.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.run()
    for _ in range(2):
        c.dverts.fill_(float('nan'))
        c.dpoints.fill_(float('nan'))
        c.ws.fill_(float('nan'))
        g.replay()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(c.result(), clean)), 'a replayed graph differs from the eager call'


def test_argument_errors_name_the_argument():
    """every failure is EINVAL before any HIP call (the pointers are never dereferenced) and names the argument"""
    L = hipabi.load()
    P = C.c_void_p(4096)
    meas = [measurement(GIRTH, (10,), (0, 1, 0)), measurement(EXTENT, direction=(0, 1, 0))]

    def call(meas=meas, verts=P, points=P, faces=P, parts=P, off=P, vf=P, dout=P, dverts=P, dpoints=P, ws=P, batch=2, nverts=10, n_points=3, rows=3, nfaces=20):
        rc = L.straps_measure_mesh_bwd(verts, points, faces, parts, off, vf, _structs(meas), dout, dverts, dpoints, ws, batch, nverts, n_points, rows, nfaces, len(meas), None)
        return rc, L.straps_last_error().decode()
    for kw, word in ((dict(dout=None), '`dout`'), (dict(dverts=None), '`dverts`'), (dict(verts=None), '`verts`'), (dict(ws=None), '`workspace`'),
                     (dict(ws=C.c_void_p(4100)), '`workspace`'), (dict(off=None), '`vf_offsets`'), (dict(vf=None), '`vf_faces`'), (dict(rows=2), '`dpoints_rows`'),
                     (dict(dpoints=None), '`dpoints`'), (dict(points=None), '`points`'), (dict(faces=None), '`faces`'), (dict(batch=0), '`batch`'),
                     (dict(nverts=0), '`nverts`'), (dict(nverts=(1 << 20) + 1), '`nverts`'), (dict(n_points=65, rows=65), '`n_points`'), (dict(nfaces=-1), '`nfaces`'),
                     (dict(nfaces=0), '`nfaces`'), (dict(meas=[measurement(GIRTH, (13,), (0, 1, 0))]), 'anchor[0]'), (dict(meas=[measurement(GIRTH, (), (0, 1, 0))]), 'anchor[0]'),
                     (dict(meas=[measurement(PATH, (1,))]), 'PATH'), (dict(meas=[measurement(7)]), 'kind'),
                     (dict(meas=[measurement(AREA, part_mask=2)], parts=None), '`face_parts`')):
        rc, err = call(**kw)
        assert rc == EINVAL and word in err and 'straps_measure_mesh_bwd' in err, (kw, rc, err)
    # dpoints may be NULL when no anchor that is read is a point, the table when nothing reads faces: the checks pass (and a launch would follow,
    # so only the sizes are asked here)
    assert L.straps_measure_bwd_workspace_bytes(2, 10, 20, 2) == 2 * 2 * 8 * (3 + 4)
    for bad in ((0, 10, 20, 2), (2, 0, 20, 2), (2, 10, -1, 2), (2, 10, 20, 0), (2, 10, 20, 33)):
        assert L.straps_measure_bwd_workspace_bytes(*bad) == 0
