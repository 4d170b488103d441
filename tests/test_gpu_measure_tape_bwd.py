"""GPU: straps_measure_tape_bwd (csrc/measure_tape_bwd.hip) against the float64 autograd restatement of tests/tape_grad_cases.py.

The bar is the module's own, derived and not measured: |got - want| <= 2^-23 |want| + 1e-10 S per element of dverts and dpoints, S the sum of
the magnitudes of the terms added into it (tape_grad_cases.scatter).  `values` and `counts` must be straps_measure_tape's bit for bit: that
is how a test sees that the backward took the forward's branch.  Every case asserts, on the CPU, the conditions under which the gradient is
defined to the last bit (tape_grad_cases.assert_conditions).  Every output and the workspace sit between redzone margins (the workspace
NaN-filled: what a kernel reads and none wrote shows); the operands end directly in front of poison.  Every test prints the worst used
fraction of the bar.  Measured on MI355X: see the figure in DESIGN.md section 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import measure_cases as MC
import measure_grad_cases as GC
import tape_cases as TC
import tape_grad_cases as TG
from redzone import Zone
from straps_amd import hipabi, measure
from straps_amd.nmr_renderer import vertex_face_table
from tape_cases import HULL, SECTION, tape

pytestmark = pytest.mark.gpu
FPB = hipabi.MEASURE_TAPE_FACES_PER_BLOCK
Y = (0.0, 1.0, 0.0)
CASES = TC.gpu_cases()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _structs(meas):
    arr = (hipabi.TapeStruct * len(meas))()
    for q, m in zip(arr, meas):
        q.kind = m['kind']
        q.anchor[:] = m['anchor']
        q.dir[:] = m['dir']
        q.part_mask = m['part_mask']
    return arr


def workspace_formula(B, M, cap):
    return B * M * 8 * (10 + 4 * cap + ((cap + 1) // 2 + 1) // 2)


class Call:
    """the raw call on guarded outputs + workspace, operands ending in front of poison.  dpoints has `rows` rows (default: n_points) and, as
    dverts, is pre-filled with `prefill` (NaN: an element that should have been written and was not shows)"""

    def __init__(self, dev, verts, points, faces, parts, meas, dout, capacity=0, accumulate=0, rows=None, prefill=float('nan'), with_values=True):
        self.B, self.N = verts.shape[0], verts.shape[1]
        self.F, self.M = faces.shape[0], len(meas)
        self.P = 0 if points is None else points.shape[1]
        self.rows = self.P if rows is None else rows
        self.capacity, self.accumulate = capacity, accumulate
        L = hipabi.lib()
        self.z = z = Zone(dev)
        self.dverts = z.guarded((self.B, self.N, 3), name='dverts')
        self.dpoints = z.guarded((self.B, self.rows, 3), name='dpoints') if self.rows else None
        self.values = z.guarded((self.B, self.M), name='values') if with_values else None
        self.counts = z.guarded((self.B, self.M), dtype=torch.int32, fill=-1, name='counts') if with_values else None
        ws_bytes = L.straps_measure_tape_bwd_workspace_bytes(self.B, self.N, self.F, self.M, capacity)
        assert ws_bytes == workspace_formula(self.B, self.M, capacity or 2 * self.F) > 0
        self.ws = z.guarded((ws_bytes // 8,), dtype=torch.float64, name='workspace')
        assert self.ws.data_ptr() % 8 == 0
        self.prefill(prefill)
        put = lambda a: None if a is None or a.size == 0 else z.at_end(torch.from_numpy(np.ascontiguousarray(a)))
        off, vf = vertex_face_table(faces, self.N)
        self.ops = [put(verts), put(points), put(faces), put(parts), put(off), put(vf)]
        self.dout = put(np.asarray(dout, np.float32))
        self.meas = _structs(meas)

    def prefill(self, value):
        for t in (self.dverts, self.dpoints):
            if t is not None:
                t.fill_(value)

    def run(self):
        v, p, f, fp, off, vf = self.ops
        hipabi.check(hipabi.lib().straps_measure_tape_bwd(hipabi.ptr(v), hipabi.ptr(p), hipabi.ptr(f), hipabi.ptr(fp), hipabi.ptr(off), hipabi.ptr(vf), self.meas,
                                                          hipabi.ptr(self.dout), hipabi.ptr(self.dverts), hipabi.ptr(self.dpoints), hipabi.ptr(self.values),
                                                          hipabi.ptr(self.counts), hipabi.ptr(self.ws), self.B, self.N, self.P, self.rows, self.F, self.M, self.capacity,
                                                          self.accumulate, hipabi.stream_ptr()), 'straps_measure_tape_bwd')

    def result(self):
        """-> (dverts, dpoints rows 0 .. n_points - 1, values, counts); the rows of dpoints behind n_points must be as they were pre-filled"""
        torch.cuda.synchronize()
        self.z.check()
        dp, rest = np.zeros((self.B, 0, 3), np.float32), None
        if self.dpoints is not None:
            full = self.dpoints.cpu().numpy()
            dp, rest = full[:, :self.P], full[:, self.P:]
        self.rest = rest
        return (self.dverts.cpu().numpy(), dp, None if self.values is None else self.values.cpu().numpy(), None if self.counts is None else self.counts.cpu().numpy())


def _bwd(dev, verts, points, faces, parts, meas, dout, **kw):
    c = Call(dev, verts, points, faces, parts, meas, dout, **kw)
    c.run()
    return c.result()


def _forward(dev, verts, points, faces, parts, meas, capacity=0):
    """straps_measure_tape on the same operands -> (out, counts)"""
    B, N, F, M = verts.shape[0], verts.shape[1], faces.shape[0], len(meas)
    L = hipabi.lib()
    z = Zone(dev)
    out, counts = z.guarded((B, M), name='out'), z.guarded((B, M), dtype=torch.int32, fill=-1, name='counts')
    ws = z.guarded((L.straps_measure_tape_workspace_bytes(B, F, M, capacity) // 8,), dtype=torch.float64, name='forward workspace')
    put = lambda a: None if a is None or a.size == 0 else z.at_end(torch.from_numpy(np.ascontiguousarray(a)))
    v, p, f, fp = put(verts), put(points), put(faces), put(parts)
    hipabi.check(L.straps_measure_tape(hipabi.ptr(v), hipabi.ptr(p), hipabi.ptr(f), hipabi.ptr(fp), _structs(meas), hipabi.ptr(out), hipabi.ptr(counts), hipabi.ptr(ws), B, N,
                                       0 if points is None else points.shape[1], F, M, capacity, hipabi.stream_ptr()), 'straps_measure_tape')
    torch.cuda.synchronize()
    z.check()
    return out.cpu().numpy(), counts.cpu().numpy()


WORST = [0.0]


def _compare(got_v, got_p, want_v, want_p, S_v, S_p, what):
    worst = 0.0
    for name, g, want, S in (('dverts', got_v, want_v, S_v), ('dpoints', got_p, want_p, S_p)):
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
    WORST[0] = max(WORST[0], worst)
    print('%s: %d elements, worst error / bound %.3f (worst so far %.3f)' % (what, got_v.size + got_p.size, worst, WORST[0]))


def _assert_parity(dev, got, verts, points, faces, parts, meas, dout, what, capacity=0, oracle=None):
    """the gradient against the oracle, values and counts against straps_measure_tape bit for bit -> the oracle"""
    TG.assert_conditions(verts, points, faces, parts, meas)
    orc = oracle if oracle is not None else TG.oracle_grad(verts, points, faces, parts, meas, dout)
    _, want_v, want_p, S_v, S_p = orc
    _compare(got[0], got[1], want_v, want_p, S_v, S_p, what)
    if got[2] is not None:
        out, counts = _forward(dev, verts, points, faces, parts, meas, capacity)
        assert np.array_equal(bits(got[2]), bits(out)), '%s: values are not the bits of straps_measure_tape' % what
        assert np.array_equal(got[3], counts), '%s: counts differ from straps_measure_tape' % what
    return orc


def _dout(batch, n_meas, seed):
    """measure_grad_cases.random_dout with a zero planted in every body and, asserted, negative entries"""
    d = GC.random_dout(batch, n_meas, seed)
    for b in range(batch):
        d[b, (b + 1) % n_meas] = 0.0
    assert (d < 0).any() and (d == 0).any()
    return d


# ---- oracle parity on the hand-made families --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_parity(dev, name):
    """prisms 3 / 4 / 7; the star; two prisms with part masks; the sheet (a collinear set: two corners); the box (equal u, equal v, collinear
    points); one face (toward=, a zero normal, a plane that misses, a plane through the lone corner)"""
    verts, points, f, p, meas = CASES[name]
    dout = _dout(3, len(meas), sorted(CASES).index(name))
    got = _bwd(dev, verts, points, f, p, meas, dout)
    _, want_v, want_p, _, _ = _assert_parity(dev, got, verts, points, f, p, meas, dout, name)
    assert (want_v != 0).any() and (want_p != 0).any()
    for b in range(3):      # a row with dout == 0 and rows of planes that miss add nothing: the same call without them gives the same bits
        keep = [m for m in range(len(meas)) if dout[b, m] != 0]
        alone = _bwd(dev, verts[b:b + 1], points[b:b + 1], f, p, [meas[m] for m in keep], dout[b:b + 1, keep], with_values=False)
        assert np.array_equal(bits(alone[0]), bits(got[0][b:b + 1])) and np.array_equal(bits(alone[1]), bits(got[1][b:b + 1])), b
    if name == 'sheet':      # a collinear set: twice the unit vector at the two ends, with dout = 1 the x components of the corners' rows sum to +-2
        one = _bwd(dev, verts[:1], points[:1], f, p, meas[:1], np.ones((1, 1), np.float32))
        assert abs(one[0][0, :, 0][one[0][0, :, 0] > 0].sum() - 2.0) < 1e-6 and abs(one[0][0, :, 0][one[0][0, :, 0] < 0].sum() + 2.0) < 1e-6
    if name == 'one face':      # a zero normal, a miss, the plane through the lone corner: nothing
        for m in (3, 4, 5, 6):
            z = _bwd(dev, verts, points, f, p, [meas[m]], np.ones((3, 1), np.float32))
            assert not z[0].any() and not z[1].any() and not np.signbit(z[0]).any()


@pytest.fixture(scope='module')
def body_set():
    b = MC.bodies(betas_seed=1)
    specs = list(measure.tape_measurements().values()) + list(measure.posed_measurements().values())
    arr, _ = measure.tape_structs(specs, 6890)
    meas = [{'kind': q.kind, 'anchor': list(q.anchor), 'dir': list(q.dir), 'part_mask': q.part_mask} for q in arr]
    dout = GC.random_dout(3, len(meas), 5) + np.float32(0.125)
    return b, meas, dout, TG.oracle_grad(b['verts'], b['joints'], b['faces'], b['face_parts'], meas, dout)


def test_full_size_bodies(dev, body_set):
    """MC.bodies(betas_seed=1), 6 890 vertices: tape_measurements() and posed_measurements() in one call -- joint anchors and per-body normals --
    with dpoints the first 24 rows of a zeroed [B][90][3]"""
    b, meas, dout, oracle = body_set
    c = Call(dev, b['verts'], b['joints'], b['faces'], b['face_parts'], meas, dout, rows=90)
    c.dpoints.zero_()
    c.run()
    got = c.result()
    assert not c.rest.any() and not np.signbit(c.rest).any(), 'rows of dpoints behind n_points were written'
    _, want_v, want_p, _, _ = _assert_parity(dev, got, b['verts'], b['joints'], b['faces'], b['face_parts'], meas, dout, 'synthetic bodies', oracle=oracle)
    per = [(want_v[k] != 0).any(1).sum() for k in range(3)]
    print('vertices with a gradient per body: %s of 6890' % per)
    assert (np.abs(want_p[:, [0, 3, 9, 4, 5, 18, 19, 1, 2, 7, 8, 16, 17, 20, 21]]).sum(2) > 0).all() and max(per) < 600


# ---- slot prefixes and face counts at their edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (1, 2, 63, 64, 65, FPB - 1, FPB, FPB + 1, 2 * FPB + 1))
def test_cut_face_counts_at_compaction_edges(dev, k):
    verts, points, f, p, meas = TC.compaction_case(k)
    dout = np.array([[1.5, -0.75], [-2.0, 0.5], [0.25, 1.0]], np.float32)
    got = _bwd(dev, verts, points, f, p, meas, dout)
    _assert_parity(dev, got, verts, points, f, p, meas, dout, '%d cut faces' % k)
    assert (got[3] == 2 * k).all() and f.shape[0] > k
    tight = _bwd(dev, verts, points, f, p, meas, dout, capacity=2 * k)      # exactly the capacity the count needs
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(tight[:3], got[:3]))


@pytest.mark.parametrize('nfaces', (1, FPB - 1, FPB, FPB + 1))
def test_face_counts_at_trip_edges(dev, nfaces):
    verts, points, f, p, meas = TC.compaction_case(nfaces)
    f, p = f[:nfaces], p[:nfaces]
    dout = np.array([[1.0, -0.5], [-1.25, 2.0], [0.75, 0.5]], np.float32)
    got = _bwd(dev, verts, points, f, p, meas, dout)
    _assert_parity(dev, got, verts, points, f, p, meas, dout, 'nfaces %d' % nfaces)
    assert f.shape[0] == nfaces and (got[3] > 0).all()


# ---- capacity ----------------------------------------------------------------------------------------------------------------------------
def test_capacity(dev):
    """capacity == count; count - 2: the NaN rule in that row alone (NaN x dout in the row of its anchor[0], nothing else of it); dout == 0 on
    such a row leaves everything finite"""
    verts, points, f, p, _ = CASES['two prisms']
    N = verts.shape[1]
    meas = [tape(HULL, N, Y, part_mask=1 << 1), tape(HULL, N + 2, Y), tape(SECTION, N, Y), tape(HULL, N, Y, part_mask=1 << 4), tape(HULL, N + 3, Y)]
    dout = np.array([[1.0, 0.5, -1.5, 2.0, 1.0], [-0.5, 1.5, 1.0, 0.25, 1.0], [2.0, -1.0, 0.5, 1.0, 1.0]], np.float32)
    full = _bwd(dev, verts, points, f, p, meas, dout)
    _assert_parity(dev, full, verts, points, f, p, meas, dout, 'capacity 0')
    assert full[3][0].tolist() == [28, 56, 56, 28, 0]
    exact = _bwd(dev, verts, points, f, p, meas, dout, capacity=56)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(exact[:3], full[:3])) and np.array_equal(exact[3], full[3])
    short = _bwd(dev, verts, points, f, p, meas, dout, capacity=54)
    out, counts = _forward(dev, verts, points, f, p, meas, 54)
    assert np.isnan(short[2][:, 1]).all() and np.array_equal(bits(short[2]), bits(out)) and np.array_equal(short[3], counts) and np.array_equal(counts, full[3])
    # the oracle: row 1 is absent, and NaN sits in the row of its anchor, point 2
    d1 = dout.copy()
    d1[:, 1] = 0
    _, want_v, want_p, S_v, S_p = TG.oracle_grad(verts, points, f, p, meas, d1)
    want_p[:, 2] = np.nan
    _compare(short[0], short[1], want_v, want_p, S_v, S_p, 'capacity 54')
    without = _bwd(dev, verts, points, f, p, meas, d1, capacity=54)
    assert np.array_equal(bits(without[0]), bits(short[0])) and np.isfinite(without[0]).all() and np.isfinite(without[1]).all()
    assert np.array_equal(bits(without[1][:, [0, 1, 3]]), bits(short[1][:, [0, 1, 3]])) and np.isnan(without[2][:, 1]).all()


# ---- accumulate --------------------------------------------------------------------------------------------------------------------------
def test_accumulate(dev):
    verts, points, f, p, meas = CASES['prism 7']
    dout = _dout(3, len(meas), 11)
    plain = _bwd(dev, verts, points, f, p, meas, dout)
    orc = _assert_parity(dev, plain, verts, points, f, p, meas, dout, 'accumulate 0')
    onto_zeros = _bwd(dev, verts, points, f, p, meas, dout, accumulate=1, prefill=0.0)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(onto_zeros[:3], plain[:3])), 'accumulate = 1 onto zeros differs from accumulate = 0'
    rng = np.random.RandomState(5)
    old_v, old_p = rng.uniform(-2, 2, plain[0].shape).astype(np.float32), rng.uniform(-2, 2, plain[1].shape).astype(np.float32)
    c = Call(dev, verts, points, f, p, meas, dout, accumulate=1)
    c.dverts.copy_(torch.from_numpy(old_v))
    c.dpoints.copy_(torch.from_numpy(old_p))
    c.run()
    got = c.result()
    _, want_v, want_p, S_v, S_p = orc
    _compare(got[0], got[1], old_v + want_v, old_p + want_p, S_v + np.abs(old_v), S_p + np.abs(old_p), 'accumulate 1 onto a prefilled buffer')


# ---- isolation and reproducibility: bit for bit -------------------------------------------------------------------------------------------
def test_isolation_reproducibility_and_graph_replay(dev, body_set):
    b, meas, dout, _ = body_set
    args = (b['faces'], b['face_parts'], meas)
    clean = _bwd(dev, b['verts'], b['joints'], *args, dout)
    again = _bwd(dev, b['verts'], b['joints'], *args, dout)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(clean[:3], again[:3])), 'two runs of the same call differ'
    for k in range(3):
        alone = _bwd(dev, b['verts'][k:k + 1], b['joints'][k:k + 1], *args, dout[k:k + 1])
        assert all(np.array_equal(bits(x), bits(y[k:k + 1])) for x, y in zip(alone[:3], clean[:3])), 'body %d differs between batch 1 and batch 3' % k
    order = [2, 0, 1, 0, 2]      # every body at another position, in a batch of 5
    moved = _bwd(dev, b['verts'][order], b['joints'][order], *args, dout[order])
    assert all(np.array_equal(bits(x), bits(y[order])) for x, y in zip(moved[:3], clean[:3])), 'a body differs at another position in a batch of 5'
    # a NaN vertex in body 1 (one of the torso's): its own rows may hold NaNs, the neighbours keep their bits
    dirty = b['verts'].copy()
    dirty[1, b['faces'][np.nonzero(b['face_parts'] == 6)[0][:40]].ravel()] = np.nan
    got = _bwd(dev, dirty, b['joints'], *args, dout)
    assert all(np.array_equal(bits(x[[0, 2]]), bits(y[[0, 2]])) for x, y in zip(got[:3], clean[:3])), 'a NaN in body 1 changed another body'
    assert np.isnan(got[2][1]).any() and not np.isnan(got[0][[0, 2]]).any() and not np.isnan(got[1][[0, 2]]).any()
    # graph capture and replay against eager
    c = Call(dev, b['verts'], b['joints'], *args, dout)
    c.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.run()
    for _ in range(2):
        for t in (c.dverts, c.dpoints, c.values, c.ws):
            t.fill_(float('nan'))
        c.counts.fill_(-1)
        g.replay()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(c.result()[:3], clean[:3])), 'a replayed graph differs from the eager call'


# ---- kinds and measurement counts ---------------------------------------------------------------------------------------------------------
def _mixed(n_meas, nverts, n_points, seed, kinds=(HULL, SECTION)):
    rng = np.random.RandomState(4000 + seed)
    out = []
    for m in range(n_meas):
        a = int(rng.randint(nverts + n_points)) if m % 3 else nverts + n_points - 1
        mask = int(rng.randint(1, 256)) if m % 4 == 1 else 0
        kind = kinds[m % len(kinds)]
        if m % 5 == 3:
            b = (a + 1 + int(rng.randint(nverts + n_points - 1))) % (nverts + n_points)
            out.append(tape(kind, a, toward=b, part_mask=mask))
        else:
            out.append(tape(kind, a, rng.uniform(-1, 1, 3) if m % 7 else (0.0, 0.0, 2.0), part_mask=mask))
    return out


SOUP_SEED = 21      # one at which tape_grad_cases.assert_conditions holds for the three sets below (asserted in every run)


@pytest.mark.parametrize('kinds', [(HULL, SECTION), (SECTION,), (HULL,)], ids=['mixed', 'section only', 'hull only'])
def test_32_measurements_and_one(dev, kinds):
    """a triangle soup (faces that repeat a vertex included), 32 measurements with vertex and point anchors, per-body normals and part masks;
    SECTION-only calls skip the march; then n_meas == 1"""
    verts, points, faces, parts = MC.soup(3, 97, FPB + 61, n_points=7, seed=SOUP_SEED)
    meas = _mixed(32, 97, 7, SOUP_SEED, kinds)
    dout = _dout(3, 32, SOUP_SEED)
    got = _bwd(dev, verts, points, faces, parts, meas, dout)
    _, want_v, want_p, _, _ = _assert_parity(dev, got, verts, points, faces, parts, meas, dout, '32 measurements, kinds %r' % (kinds,))
    assert (want_v != 0).any() and (want_p != 0).any() and any(q['anchor'][1] >= 0 for q in meas)
    one = _bwd(dev, verts, points, faces, parts, meas[:1], dout[:, 2:3])
    _assert_parity(dev, one, verts, points, faces, parts, meas[:1], dout[:, 2:3], 'one measurement of kind %d' % meas[0]['kind'])


def test_argument_errors_name_the_argument():
    """(the full list is in test_measure_tape_bwd_abi.py, which needs no GPU; here: a failing call launches nothing and leaves the error text)"""
    L = hipabi.load()
    P = C.c_void_p(4096)
    rc = L.straps_measure_tape_bwd(P, P, P, P, P, P, _structs([tape(HULL, 3, Y)]), None, P, P, None, None, P, 2, 10, 3, 3, 20, 1, 0, 0, None)
    assert rc == 1 and '`dout`' in L.straps_last_error().decode()
