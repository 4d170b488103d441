"""GPU: straps_measure_tape (csrc/measure_tape.hip) against the float64 restatement of tests/tape_cases.py.

The bar is the module's own, derived and not measured: |gpu - oracle| <= 2^-23 |oracle| + 1e-10 S.  Both sides read the same fp32 inputs and
compute every term in double.  For SECTION S is the sum of the terms (the two differ by summation order and fused multiply-adds).  For HULL
S = perimeter + 2 pi max_q |q - o|: the perimeter of a convex hull is 2 pi-Lipschitz in the largest displacement of a point
(tests/test_tape_cases_cpu.py asserts it), and the two computations displace the section points by a few double ulps of their distance
from the anchor.  `counts` is compared exactly: in the hand-made cases no vertex lies within 1e-9 of the mesh size of a plane unless exactly
on it (asserted on the CPU).  `out`, `counts` and the workspace (NaN-filled doubles: a point the hull kernel reads and the collect kernel
did not write makes the row NaN) sit between redzone margins; the operands end directly in front of poison.  Every test prints the worst
used fraction of the bar."""
import numpy as np
import pytest
import torch

import measure_cases as MC
import predict_cases as PC
import straps_amd
import tape_cases as TC
from redzone import Zone
from straps_amd import hipabi, measure
from tape_cases import HULL, SECTION, tape

pytestmark = pytest.mark.gpu
FPB = hipabi.MEASURE_TAPE_FACES_PER_BLOCK
MP = straps_amd.synthetic_mean_params(0)
MODEL = straps_amd.synthetic_smpl_model(0)
Y = (0.0, 1.0, 0.0)
CASES = TC.gpu_cases()


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


class Call:
    """the raw call on guarded out / counts / workspace, operands ending in front of poison; `run()` launches on the current stream"""

    def __init__(self, dev, verts, points, faces, parts, meas, capacity=0, with_counts=True):
        B, N = verts.shape[0], verts.shape[1]
        F, M = faces.shape[0], len(meas)
        L = hipabi.lib()
        self.z = z = Zone(dev)
        self.out = z.guarded((B, M), name='out')
        self.counts = z.guarded((B, M), dtype=torch.int32, fill=-1, name='counts') if with_counts else None
        ws_bytes = L.straps_measure_tape_workspace_bytes(B, F, M, capacity)
        assert ws_bytes == B * M * 8 * (2 + 2 * (capacity or 2 * F)) > 0
        self.ws = z.guarded((ws_bytes // 8,), dtype=torch.float64, name='workspace')
        assert self.ws.data_ptr() % 8 == 0
        put = lambda a: None if a is None or a.size == 0 else z.at_end(torch.from_numpy(np.ascontiguousarray(a)))
        v, p, f, fp = put(verts), put(points), put(faces), put(parts)
        arr = _structs(meas)
        self.run = lambda: hipabi.check(L.straps_measure_tape(hipabi.ptr(v), hipabi.ptr(p), hipabi.ptr(f), hipabi.ptr(fp), arr, hipabi.ptr(self.out), hipabi.ptr(self.counts),
                                                              hipabi.ptr(self.ws), B, N, 0 if points is None else points.shape[1], F, M, capacity,
                                                              hipabi.stream_ptr()), 'straps_measure_tape')

    def result(self):
        torch.cuda.synchronize()
        self.z.check()
        return self.out.cpu().numpy(), None if self.counts is None else self.counts.cpu().numpy()


def _tape(dev, verts, points, faces, parts, meas, capacity=0, with_counts=True):
    c = Call(dev, verts, points, faces, parts, meas, capacity, with_counts)
    c.run()
    return c.result()


WORST = [0.0]


def _assert_parity(got, counts, verts, points, faces, parts, meas, what, oracle=None):
    want, S, cnt = oracle if oracle is not None else TC.oracle(verts, points, faces, parts, meas)
    assert got.dtype == np.float32 and got.shape == want.shape
    if counts is not None:
        assert counts.dtype == np.int32 and np.array_equal(counts, cnt), '%s: counts %r, oracle %r' % (what, counts.tolist()[:2], cnt.tolist()[:2])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaNs sit elsewhere than in the restatement' % what
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-10 * S
    ok = nan | (err <= bound)
    worst = float(np.where(nan, 0.0, err / np.where(bound > 0, bound, 1.0)).max())
    WORST[0] = max(WORST[0], worst)
    print('%s: %d values, worst error / bound %.3f (worst so far %.3f)' % (what, got.size, worst, WORST[0]))
    assert ok.all(), '%s: (body, measurement) %s outside the bound: got %r, oracle %r, bound %r' % (
        what, np.argwhere(~ok)[:4].tolist(), got[~ok][:4].tolist(), want[~ok][:4].tolist(), bound[~ok][:4].tolist())
    return want, cnt


bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


# ---- oracle parity and degenerate sections --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_parity(dev, name):
    """prisms n = 3, 4 (axis-aligned corners), 7 with a point and a vertex as anchors, a tilted plane and a plane that misses; the star, HULL <
    SECTION; two prisms with and without part masks; the flat sheet (a collinear section); the box (equal u, equal v); one face"""
    verts, points, f, p, meas = CASES[name]
    got, counts = _tape(dev, verts, points, f, p, meas)
    want, cnt = _assert_parity(got, counts, verts, points, f, p, meas, name)
    hull = [m for m, q in enumerate(meas) if q['kind'] == HULL]
    if name.startswith('prism'):
        n = int(name.split()[1])
        assert cnt[:, :2].tolist() == [[4 * n, 4 * n]] * 3 and (cnt[:, 6:] == 0).all() and (got[:, 6:] == 0).all() and not np.signbit(got[:, 6:]).any()
        assert np.allclose(got[0, :2], 2 * n * 0.5 * np.sin(np.pi / n), rtol=1e-6) and (cnt[:, 2:6] > 0).all()
        assert np.allclose(got[:, 2], got[:, 3], rtol=1e-6) and np.allclose(got[:, 4], got[:, 5], rtol=1e-6)      # convex sections: hull == section
    if name == 'star':
        assert (got[:, 0] < 0.9 * got[:, 1]).all() and (got[:, 2] < 0.9 * got[:, 3]).all() and abs(got[0, 0] - 5.8779) < 1e-4 and abs(got[0, 1] - 7.1609) < 1e-4
    if name == 'two prisms':
        per = 14 * 0.3 * np.sin(np.pi / 7)
        assert np.allclose(got[0], [per + 2.0, 2 * per, per, per, per, 0.0], rtol=1e-6) and cnt[0].tolist() == [56, 56, 28, 28, 28, 0]
    if name == 'sheet':
        assert np.allclose(got[:, 0], 2 * got[:, 1], rtol=1e-6) and np.allclose(got[0, :2], [4.0, 2.0], rtol=1e-6) and cnt[0, 0] == 20      # there and back
    if name == 'box':
        assert np.allclose(got[0, :2], 4.0, rtol=1e-6) and cnt[0, 0] == 80
    if name == 'one face':
        assert np.allclose(got[:, 0], 2 * got[:, 1], rtol=1e-6) and (got[:, 1] > 0).all() and cnt.tolist() == [[2, 2, 2, 0, 0, 2, 2]] * 3      # one cut face: 2 x its segment
        assert (got[:, 3:] == 0).all()                                                                                                # A1 == A0: a zero normal; a miss
        assert (got[:, 5:] == 0).all() and not np.signbit(got[:, 5:]).any()      # two section points, both the corner the plane passes through: all of Q coincides, hull 0
    assert len(hull) >= 2


def test_skipped_faces_and_labels(dev):
    """a face with an index out of range is skipped (appended, so every other face keeps its slot: same bits); a label >= 32 is never selected by
    a mask, and is without one"""
    verts, points, f, p, _ = CASES['prism 7']
    N = verts.shape[1]
    meas = [tape(HULL, N, Y), tape(SECTION, N, Y), tape(HULL, N + 2, (0.3, 1.0, -0.2), part_mask=1 << 1)]
    bad = np.concatenate([f, [[0, 7, N], [-1, 2, 9], [4, 1 << 30, 12], [N, N, N], [0, 7, 1]]]).astype(np.int32)
    bad_parts = np.concatenate([p, [1, 1, 1, 1, 9]]).astype(np.uint8)
    with_bad, cb = _tape(dev, verts, points, bad, bad_parts, meas)
    without, cw = _tape(dev, verts, points, f, p, meas)
    _assert_parity(with_bad, cb, verts, points, bad, bad_parts, meas, 'out-of-range faces')
    assert np.array_equal(bits(with_bad[:, 2]), bits(without[:, 2])) and np.array_equal(cb[:, 2], cw[:, 2]) and (cb[:, :2] == cw[:, :2] + 2).all()      # (0, 7, 1) is cut, unmasked
    odd = p.copy()
    odd[:6] = (32, 33, 64, 255, 128, 40)
    meas = [tape(HULL, N, Y, part_mask=0xffffffff), tape(SECTION, N, Y, part_mask=0xffffffff), tape(HULL, N, Y), tape(SECTION, N, Y), tape(HULL, N, Y, part_mask=1 << 0)]
    got, counts = _tape(dev, verts, points, f, odd, meas)
    _assert_parity(got, counts, verts, points, f, odd, meas, 'labels >= 32')
    assert counts[0].tolist() == [28 - 12, 28 - 12, 28, 28, 0] and (got[:, 1] < got[:, 3]).all() and (got[:, 4] == 0).all()


@pytest.mark.parametrize('k', (63, 64, 65, FPB - 1, FPB, FPB + 1, 2 * FPB + 1))
def test_cut_face_counts_at_compaction_edges(dev, k):
    """k cut faces with uncut ones strewn between them: the wave's ballot prefix, the wave offsets and the running count across trips"""
    verts, points, f, p, meas = TC.compaction_case(k)
    got, counts = _tape(dev, verts, points, f, p, meas)
    _assert_parity(got, counts, verts, points, f, p, meas, '%d cut faces' % k)
    assert (counts == 2 * k).all() and f.shape[0] > k
    # exactly the capacity the count needs, and with_counts = NULL
    tight, _ = _tape(dev, verts, points, f, p, meas, capacity=2 * k, with_counts=False)
    assert np.array_equal(bits(tight), bits(got))


def test_capacity(dev):
    """capacity == count; count - 2: that HULL row is NaN, SECTION is right, counts are full, the neighbouring rows keep their bits; 0"""
    verts, points, f, p, _ = CASES['two prisms']
    N = verts.shape[1]
    meas = [tape(HULL, N, Y, part_mask=1 << 1), tape(HULL, N, Y), tape(SECTION, N, Y), tape(HULL, N, Y, part_mask=1 << 4), tape(HULL, N + 3, Y)]
    full, cf = _tape(dev, verts, points, f, p, meas, capacity=0)
    _assert_parity(full, cf, verts, points, f, p, meas, 'capacity 0')
    assert cf[0].tolist() == [28, 56, 56, 28, 0]
    exact, ce = _tape(dev, verts, points, f, p, meas, capacity=56)
    assert np.array_equal(bits(exact), bits(full)) and np.array_equal(ce, cf)
    for cap in (54, 55, 28, 29):
        short, cs = _tape(dev, verts, points, f, p, meas, capacity=cap)
        assert np.isnan(short[:, 1]).all() and np.array_equal(cs, cf), cap
        keep = [0, 2, 3, 4]
        assert np.array_equal(bits(short[:, keep]), bits(full[:, keep])), cap
    tiny, ct = _tape(dev, verts, points, f, p, meas, capacity=2)
    assert np.isnan(tiny[:, [0, 1, 3]]).all() and np.array_equal(bits(tiny[:, [2, 4]]), bits(full[:, [2, 4]])) and np.array_equal(ct, cf)


def test_per_body_normals(dev):
    """three rigidly rotated copies of one prism, the plane through joint 0 perpendicular to the bone toward joint 1: each row within the bar of its
    own oracle, and the three rows agree to 1e-6 relative (the rounding of the fp32 rotation)"""
    v, f, p = TC.prism(7, 0.5, 1.0)
    pts = np.array([[0.02, 0.1, 0.01], [0.02, 0.6, 0.01]])
    Rs = [np.eye(3), TC.rotation((1.0, 2.0, -0.5), 0.9), TC.rotation((-0.3, 0.1, 1.0), 2.4)]
    verts = np.stack([v @ R.T for R in Rs]).astype(np.float32)
    points = np.stack([pts @ R.T for R in Rs]).astype(np.float32)
    N = v.shape[0]
    meas = [tape(HULL, N, toward=N + 1), tape(SECTION, N, toward=N + 1), tape(HULL, N, toward=N + 1, part_mask=1 << 1), tape(HULL, N + 1, toward=N), tape(HULL, N, toward=7)]
    got, counts = _tape(dev, verts, points, f, p, meas)
    want, cnt = _assert_parity(got, counts, verts, points, f, p, meas, 'per-body normals')
    assert (cnt[:, :3] == 28).all() and (cnt[:, 3] == 0).all()           # the plane through joint 1 lies beyond the prism's top
    assert np.allclose(got[1:], got[:1], rtol=1e-6, atol=0) and np.allclose(got[:, 0], 14 * 0.5 * np.sin(np.pi / 7), rtol=1e-6)
    assert (cnt[:, 4] > 0).all() and (got[:, 4] > got[:, 0]).all()      # toward a vertex of the top ring: a tilted plane


def test_section_equals_the_girth_of_measure_mesh(dev):
    """SECTION with `dir` against GIRTH of straps_measure_mesh on the same inputs, within the bar (the summation orders differ)"""
    verts, points, faces, parts = MC.soup(3, 97, 2 * FPB + 45, n_points=7, seed=3)
    planes = [(97 + 2, (0.1, 1.0, -0.2), 0), (5, (1.0, 0.0, 0.0), 0), (97 + 6, (0.0, -2.0, 0.5), 0b10110), (96, (0.3, 0.3, 0.3), 1 << 31 | 1)]
    meas = [tape(SECTION, a, d, part_mask=m) for a, d, m in planes]
    got, counts = _tape(dev, verts, points, faces, parts, meas)
    want, _ = _assert_parity(got, counts, verts, points, faces, parts, meas, 'SECTION on a soup')
    L = hipabi.lib()
    old = (hipabi.MeasureStruct * len(planes))()
    for q, (a, d, m) in zip(old, planes):
        q.kind, q.part_mask = hipabi.MEASURE_GIRTH, m
        q.anchor[:] = [a, -1, -1, -1]
        q.dir[:] = d
    z = Zone(dev)
    out = z.guarded((3, len(planes)), name='girth')
    ws = z.guarded((L.straps_measure_workspace_bytes(3, 97, faces.shape[0], len(planes)) // 8,), dtype=torch.float64, name='girth workspace')
    t = [z.at_end(torch.from_numpy(a)) for a in (verts, points, faces, parts)]
    hipabi.check(L.straps_measure_mesh(*[hipabi.ptr(x) for x in t], old, hipabi.ptr(out), hipabi.ptr(ws), 3, 97, 7, faces.shape[0], len(planes), hipabi.stream_ptr()),
                 'straps_measure_mesh')
    torch.cuda.synchronize()
    z.check()
    girth = out.cpu().numpy()
    assert (want[:, :3] > 0).all() and (want[:, 3] > 0).any() and (np.abs(girth.astype(np.float64) - got) <= 2.0 ** -23 * want + 1e-10 * want).all()


# ---- kinds and batches ----------------------------------------------------------------------------------------------------------------
def _mixed(n_meas, nverts, n_points, seed):
    rng = np.random.RandomState(4000 + seed)
    out = []
    for m in range(n_meas):
        a = int(rng.randint(nverts + n_points)) if m % 3 else nverts + n_points - 1
        mask = int(rng.randint(1, 256)) if m % 4 == 1 else 0
        if m % 5 == 3:
            b = (a + 1 + int(rng.randint(nverts + n_points - 1))) % (nverts + n_points)
            out.append(tape(m % 2, a, toward=b, part_mask=mask))
        else:
            out.append(tape(m % 2, a, rng.uniform(-1, 1, 3) if m % 7 else (0.0, 0.0, 2.0), part_mask=mask))
    return out


@pytest.mark.parametrize('batch', (1, 3))
def test_32_measurements_of_mixed_kinds(dev, batch):
    verts, points, faces, parts = MC.soup(batch, 97, FPB + 61, n_points=7, seed=20 + batch)
    meas = _mixed(32, 97, 7, batch)
    assert sum(q['kind'] == HULL for q in meas) == 16 and any(q['anchor'][1] >= 0 for q in meas)
    got, counts = _tape(dev, verts, points, faces, parts, meas)
    want, cnt = _assert_parity(got, counts, verts, points, faces, parts, meas, 'batch %d, 32 mixed' % batch)
    assert (cnt > 0).sum() > 20 * batch and (want > 0).sum() > 20 * batch
    for q in (meas[0], meas[1]):      # n_meas == 1: a HULL alone, a SECTION alone (no hull launch)
        g1, c1 = _tape(dev, verts, points, faces, parts, [q])
        _assert_parity(g1, c1, verts, points, faces, parts, [q], 'batch %d, kind %d alone' % (batch, q['kind']))


def test_more_rows_than_65535(dev):
    """batch x n_meas = 65 568 workgroups on the 12-face prism: bodies are copies of three, so every row must carry the bits of its first copy"""
    verts3, points3, f, p, _ = CASES['prism 3']
    assert f.shape[0] == 12
    B, N = 2049, verts3.shape[1]
    verts, points = np.tile(verts3, (B // 3, 1, 1)), np.tile(points3, (B // 3, 1, 1))
    meas = [tape(m % 2, N + m % 3, Y if m % 4 < 2 else (0.3, 1.0, -0.2), part_mask=0 if m % 8 else 1 << 1) for m in range(32)]
    got, counts = _tape(dev, verts, points, f, p, meas)
    assert B * 32 > 65535 and got.shape == (B, 32)
    _assert_parity(got[:3], counts[:3], verts3, points3, f, p, meas, 'first three of 2049 bodies')
    assert np.array_equal(bits(got), np.tile(bits(got[:3]), (B // 3, 1))) and np.array_equal(counts, np.tile(counts[:3], (B // 3, 1)))


# ---- isolation and reproducibility: bit for bit ---------------------------------------------------------------------------------------
def test_isolation_and_reproducibility(dev):
    verts, points, faces, parts = MC.soup(3, 97, FPB + 61, n_points=7, seed=9)
    meas = _mixed(12, 97, 7, 9)
    clean, cc = _tape(dev, verts, points, faces, parts, meas)
    again, ca = _tape(dev, verts, points, faces, parts, meas)
    assert np.array_equal(bits(clean), bits(again)) and np.array_equal(cc, ca), 'two runs of the same call differ'
    for k in range(3):      # a body alone, and inside a batch at another index
        alone, c1 = _tape(dev, verts[k:k + 1], points[k:k + 1], faces, parts, meas)
        assert np.array_equal(bits(alone), bits(clean[k:k + 1])) and np.array_equal(c1, cc[k:k + 1]), 'body %d differs between batch 1 and batch 3' % k
    moved, cm = _tape(dev, verts[[2, 0, 1]], points[[2, 0, 1]], faces, parts, meas)
    assert np.array_equal(bits(moved), bits(clean[[2, 0, 1]])) and np.array_equal(cm, cc[[2, 0, 1]])
    # a NaN body beside finite ones: every vertex of body 1; then one vertex, then an infinite one
    for what, poison in (('all NaN', lambda v: v.fill(np.nan)), ('one NaN vertex', lambda v: v.__setitem__(40, np.nan)), ('one infinite coordinate', lambda v: v.__setitem__((40, 1), np.inf))):
        dirty = verts.copy()
        poison(dirty[1])
        got, cg = _tape(dev, dirty, points, faces, parts, meas)
        assert np.array_equal(bits(got[[0, 2]]), bits(clean[[0, 2]])) and np.array_equal(cg[[0, 2]], cc[[0, 2]]), '%s in body 1 changed another body' % what
        _assert_parity(got, cg, dirty, points, faces, parts, meas, what + ' in body 1')
        assert not np.isnan(got[[0, 2]]).any()
    # graph capture and replay against eager
    c = Call(dev, verts, points, faces, parts, meas)
    c.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.run()
    for _ in range(2):
        c.out.fill_(float('nan'))
        c.counts.fill_(-1)
        c.ws.fill_(float('nan'))
        g.replay()
        replayed, cr = c.result()
        assert np.array_equal(bits(replayed), bits(clean)) and np.array_equal(cr, cc), 'a replayed graph differs from the eager call'


# ---- full size, through the modules ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def body_set():
    return MC.bodies(batch=4)


def _tape_dicts(specs, nverts):
    arr, _ = measure.tape_structs(specs, nverts)
    return [{'kind': q.kind, 'anchor': list(q.anchor), 'dir': list(q.dir), 'part_mask': q.part_mask} for q in arr]


def test_full_size_bodies_through_body_measurer(dev, body_set):
    """four bodies of the synthetic 6 890-vertex model: tape_measurements() and posed_measurements() through BodyMeasurer, alone, mixed with the
    default set, with counts and with a capacity"""
    b = body_set
    assert b['verts'].shape == (4, 6890, 3) and b['faces'].shape == (13776, 3)
    v, j = torch.from_numpy(b['verts']).to(dev), torch.from_numpy(b['joints']).to(dev)
    specs = list(measure.tape_measurements().items()) + list(measure.posed_measurements().items())
    meas = _tape_dicts([s for _, s in specs], 6890)
    m = straps_amd.BodyMeasurer(b['faces'], b['face_parts'], specs).to(dev)
    res = m(v, j)
    assert list(res) == ['values'] + [n for n, _ in specs] and res['values'].dtype == torch.float32 and tuple(res['values'].shape) == (4, 15)
    counts = m.measure_counts(v, j)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (4, 15)
    oracle = TC.oracle(b['verts'], b['joints'], b['faces'], b['face_parts'], meas)
    want, cnt = _assert_parity(res['values'].cpu().numpy(), counts.cpu().numpy(), b['verts'], b['joints'], b['faces'], b['face_parts'], meas, 'synthetic bodies', oracle)
    assert (want > 0).all() and (cnt >= 6).all()
    raw, craw = _tape(dev, b['verts'], b['joints'][:, :22], b['faces'], b['face_parts'], meas)
    assert np.array_equal(bits(raw), bits(res['values'].cpu().numpy())) and np.array_equal(craw, counts.cpu().numpy())
    for i, (n, _) in enumerate(specs):
        assert res[n].data_ptr() == res['values'][:, i].data_ptr()
    # the same plane and faces as tape girth, as section and as GIRTH of straps_measure_mesh.  (No order between hull and section here: the
    # synthetic model's faces are a soup, its section is loose segments and not a loop, and the hull of loose segments can be the longer.)
    names = [n for n, _ in specs]
    both = straps_amd.BodyMeasurer(b['faces'], b['face_parts'], [('t', measure.tape_girth(('joint', 3), Y, parts=(6,))), ('s', measure.section_girth(('joint', 3), Y, parts=(6,))),
                                                                ('g', measure.girth(('joint', 3), Y, parts=(6,)))]).to(dev)(v, j)
    assert torch.equal(both['t'], res['waist_tape_girth']) and (both['s'] > 0).all()
    assert ((both['s'].double() - both['g'].double()).abs() <= 2.0 ** -23 * both['g'].double()).all()
    # mixed with the default set, interleaved: every column carries the bits of its own call, in the order of `names`
    d = list(measure.default_measurements().items())
    mixed = [x for pair in zip(d, specs) for x in pair]
    mm = straps_amd.BodyMeasurer(b['faces'], b['face_parts'], mixed).to(dev)
    assert mm.tape_columns == tuple(range(1, 30, 2)) and mm.mesh_columns == tuple(range(0, 30, 2))
    vals = mm(v, j)
    old = straps_amd.BodyMeasurer(b['faces'], b['face_parts']).to(dev)(v, j)
    assert list(vals) == ['values'] + [n for n, _ in mixed] and tuple(vals['values'].shape) == (4, 30)
    assert torch.equal(vals['values'][:, 0::2], old['values']) and torch.equal(vals['values'][:, 1::2], res['values'])
    assert torch.equal(mm.measure_counts(v, j), counts) and tuple(straps_amd.BodyMeasurer(b['faces'], b['face_parts']).to(dev).measure_counts(v, j).shape) == (4, 0)
    # tape_capacity: just enough gives the same bits; one pair short makes exactly the fullest column's bodies NaN
    top = int(counts.max())
    assert torch.equal(straps_amd.BodyMeasurer(b['faces'], b['face_parts'], specs, tape_capacity=top).to(dev)(v, j)['values'], res['values'])
    short = straps_amd.BodyMeasurer(b['faces'], b['face_parts'], specs, tape_capacity=top - 2).to(dev)
    sv = short(v, j)['values']
    over = counts > top - 2
    assert over.any() and torch.equal(torch.isnan(sv), over) and torch.equal(sv[~over], res['values'][~over]) and torch.equal(short.measure_counts(v, j), counts)
    with pytest.raises(RuntimeError, match='joints'):
        m(v)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        m.measure_counts(v.cpu(), j)
    print('largest count %d of %d; names %s' % (top, 2 * 13776, names[int(counts.max(0).values.argmax())]))


def test_mixed_specs_that_read_different_numbers_of_joints(dev, body_set):
    """the mesh call and the tape call of one BodyMeasurer share the joints tensor, whose row count is the stride to a body's points: specs of
    one call that read fewer joints than the other's must not move it.  Every column bit for bit as the unmixed measurers give it, batch 4"""
    b = body_set
    v, j = torch.from_numpy(b['verts']).to(dev), torch.from_numpy(b['joints']).to(dev)
    F, P = b['faces'], b['face_parts']
    d, t, p = (list(f().items()) for f in (measure.default_measurements, measure.tape_measurements, measure.posed_measurements))
    few_mesh = [('waist', measure.girth(('joint', 3), Y, parts=(6,))), ('span', measure.extent((1, 0, 0))), ('hop', measure.path(('joint', 1), ('joint', 4)))]
    few_tape = [('waist_tape', measure.tape_girth(('joint', 3), Y, parts=(6,))), ('knee', measure.section_girth(('joint', 4), toward=('joint', 1), parts=(4,)))]
    alone = lambda specs: straps_amd.BodyMeasurer(F, P, specs).to(dev)
    for mesh, tape_specs in ((d, t), (few_mesh, p), (d, few_tape), (few_mesh, t)):
        ma, ta = alone(mesh), alone(tape_specs)
        assert ma.needs_joints != ta.needs_joints
        both = alone(mesh + tape_specs)
        assert both.needs_joints == max(ma.needs_joints, ta.needs_joints)
        got = both(v, j)
        want_m, want_t = ma(v, j), ta(v, j)
        assert torch.equal(got['values'].view(torch.int32), torch.cat([want_m['values'], want_t['values']], 1).view(torch.int32))
        for n, _ in mesh:
            assert torch.equal(got[n].view(torch.int32), want_m[n].view(torch.int32)), n
        for n, _ in tape_specs:
            assert torch.equal(got[n].view(torch.int32), want_t[n].view(torch.int32)), n
        assert torch.equal(both.measure_counts(v, j), ta.measure_counts(v, j))
        assert not torch.isnan(got['values']).any() and (got['values'][1:] != got['values'][:1]).any()      # the bodies differ: a wrong stride would show


def test_predictor_measure_posed(dev):
    """Predictor.measure(posed=True) measures out['vertices'] with out['joints']; the default call is today's"""
    B = 2
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP).to(dev).eval()
    smpl = straps_amd.SMPL(MODEL, batch_size=B).to(dev)
    sil, joints = PC.inputs('a')
    pred = straps_amd.Predictor(reg, smpl)
    out = pred(torch.from_numpy(sil[:B]).to(dev), torch.from_numpy(joints[:B]).to(dev))
    kept = {k: v.clone() for k, v in out.items()}
    measurer = straps_amd.BodyMeasurer.from_smpl(smpl, measure.posed_measurements()).to(dev)
    m = pred.measure(out, measurer, posed=True)
    for k in kept:
        assert torch.equal(out[k].contiguous().view(torch.uint8), kept[k].contiguous().view(torch.uint8)), k
    direct = measurer(out['vertices'], out['joints'])
    assert list(m) == list(direct) == ['values'] + list(measure.posed_measurements())
    for k in m:
        assert torch.equal(m[k], direct[k]), k
    meas = _tape_dicts(measurer.specs, 6890)
    v, j = out['vertices'].cpu().numpy(), out['joints'][:, :22].cpu().numpy()
    want, _ = _assert_parity(m['values'].cpu().numpy(), measurer.measure_counts(out['vertices'], out['joints']).cpu().numpy(), v, j, MODEL['faces'], MODEL['face_parts'], meas,
                             'Predictor.measure(posed=True)')
    assert np.isfinite(want).all() and (want > 0).any()
    # the T-pose call: unchanged by the new keyword
    default = straps_amd.BodyMeasurer.from_smpl(smpl).to(dev)
    a, b = pred.measure(out, default), pred.measure(out, default, posed=False)
    assert all(torch.equal(a[k], b[k]) for k in a)
    eye = torch.eye(3, device=dev).expand(B, 24, 3, 3).contiguous()
    _, tj = smpl.forward_arrays(out['shape'].contiguous(), eye)
    assert torch.equal(a['values'], default(out['reposed_vertices'], tj)['values'])
