"""GPU: straps_scan_energy (csrc/scanfit.hip) against the float64 restatement of tests/scan_cases.py: energy2, dverts, dtrans, nearest_vertex,
nearest_point.

Every output and the workspace sit behind redzone guards, every input ends against a NaN margin.  The cases (scan_cases.SPECS) are the
smallest shapes at which each size-dependent path of the kernels exists -- one and several candidate tiles and query chunks on either side,
ragged and whole last chunks, more work items than workgroups per body in either search, more than 256 partial sums of points and of
vertices -- plus one case of the workload's size; tests/test_scan_cases_cpu.py asserts, from path_facts, that they reach those paths, and
the input conditions of each.

Chosen indices.  Where the input conditions hold (every case of up to 4096 points and vertices: best and second-best squared distance differ by
more than 1e-4 relative outside the planted exact ties) the indices must equal the float64 ones exactly; planted ties resolve to the lower
index.  In the larger cases a differing index is accepted only by excess: the float64 squared distance of the chosen partner may exceed the
minimum by at most 2^-20 relative, and at most 1 in 10 000 indices of a case may differ at all.  The bound: with u = 2^-24, each fp32
difference carries one rounding (1 + e, |e| <= u) and enters squared, and the chain fmaf(dz, dz, fmaf(dy, dy, dx * dx)) adds one rounding per
operation, so an fp32 squared distance is its float64 value times a factor within (1 + u)^2 (1 + u)^3, i.e. within 5u + O(u^2) of one.  If the
kernel prefers j to the float64 minimum k, then d32(j) <= d32(k), hence d(j) (1 - 5u) <= d(k) (1 + 5u) and d(j) / d(k) <= 1 + 10u + O(u^2)
< 1 + 16u = 1 + 2^-20.
Bounds (the silhouette energy's, the project's bars): energies 1e-5 relative to the float64 restatement evaluated at the GPU's indices; dverts
and dtrans 1e-4 of the largest magnitude in the tensor.
Measured on MI355X: see DESIGN.md, "Test-time fitting to a 3-D scan"."""
import pytest
import torch

import scan_cases as S
from redzone import Zone
from smpl_cases import cpu_threads
from straps_amd import hipabi
from straps_amd.fit import scan_energy_raw

pytestmark = pytest.mark.gpu
ALL = ('energy2', 'dverts', 'dtrans', 'nearest_vertex', 'nearest_point')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    torch.set_num_threads(cpu_threads())
    return torch.device('cuda:0')


def run(dev, case, outputs=ALL, bodies=None, ld_trans=3):
    """one raw call on guarded buffers -> dict of CPU tensors"""
    sel = slice(None) if bodies is None else bodies
    verts, trans, points = case['verts'][sel], case['trans'][sel], case['points'][sel]
    B, V, N = verts.shape[0], verts.shape[1], points.shape[1]
    z = Zone(dev)
    shapes = {'energy2': ((B, 2), torch.float32), 'dverts': ((B, V, 3), torch.float32), 'dtrans': ((B, 3), torch.float32),
              'nearest_vertex': ((B, N), torch.int32), 'nearest_point': ((B, V), torch.int32)}
    out = {k: z.guarded(shapes[k][0], dtype=shapes[k][1], fill=float('nan') if shapes[k][1] == torch.float32 else -77, name=k) for k in outputs}
    nbytes = hipabi.lib().straps_scan_energy_workspace_bytes(B, V, N)
    assert nbytes == B * (24 * V + 28 * N + 16 * -(-V // 256) + 4 * -(-N // 256) + 16) and nbytes % 4 == 0
    ws = z.guarded((nbytes // 4,), name='workspace')
    assert ws.data_ptr() % 16 == 0
    tp = torch.full((B, ld_trans), float('nan'))
    tp[:, :3] = trans
    opts = hipabi.ScanOptsStruct(case['sigma'], case['w_s2m'], case['w_m2s'])
    scan_energy_raw(z.at_end(verts), z.at_end(tp), ld_trans, z.at_end(points), opts, out.get('energy2'), out.get('dverts'), out.get('dtrans'),
                    out.get('nearest_vertex'), out.get('nearest_point'), ws)
    z.check()
    return {k: t.cpu() for k, t in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


_RUNS = {}


def whole(dev, name):
    """the full call of a case, once per process (the comparisons below share it)"""
    if name not in _RUNS:
        _RUNS[name] = run(dev, S.get_case(name))
    return _RUNS[name]


@pytest.mark.parametrize('name', sorted(S.SPECS))
def test_indices_energy_and_gradients_vs_float64(dev, name):
    case = S.get_case(name)
    got = whole(dev, name)
    B, V, N = case['verts'].shape[0], case['verts'].shape[1], case['points'].shape[1]
    valid = torch.isfinite(case['points']).all(dim=2)
    nv, npt = got['nearest_vertex'].long(), got['nearest_point'].long()
    # the range of every index, -1 at invalid points, -1 everywhere for a skipped search or a body without a valid point
    assert bool((nv[~valid] == -1).all()) and bool((nv < V).all()) and bool((npt < N).all()) and bool((nv >= -1).all()) and bool((npt >= -1).all())
    if case['w_s2m'] == 0:
        assert bool((nv == -1).all()) and not bool(got['energy2'][:, 0].any()), 'w_s2m = 0: E_s2m == 0 and nearest_vertex == -1'
    if case['w_m2s'] == 0:
        assert bool((npt == -1).all()) and not bool(got['energy2'][:, 1].any()), 'w_m2s = 0: E_m2s == 0 and nearest_point == -1'
    for b in range(B):
        if not bool(valid[b].any()):      # zeros and -1 in its rows alone
            assert bool((nv[b] == -1).all()) and bool((npt[b] == -1).all())
            assert not bool(got['energy2'][b].any()) and not bool(got['dverts'][b].any()) and not bool(got['dtrans'][b].any())
        else:
            assert bool((nv[b][valid[b]] >= 0).all()) == (case['w_s2m'] != 0) and bool((npt[b] >= 0).all()) == (case['w_m2s'] != 0)
    differ, total, worst = S.index_differences(case, nv, npt)
    if S.exact(name):
        assert differ == 0, '%d of %d indices differ from the float64 ones although the input conditions hold' % (differ, total)
    assert differ <= S.SHARE * total and worst <= S.EXCESS, (differ, total, worst)
    if case['dup'] is not None:
        (v_lo, v_hi), (p_lo, p_hi) = case['dup']['vertex'], case['dup']['point']
        assert bool((nv[0] == v_lo).any()) and not bool((nv[0] == v_hi).any()), 'of two vertices at one position the lower index is reported'
        assert bool((npt[0] == p_lo).any()) and not bool((npt[0] == p_hi).any()), 'of two points at one position the lower index is reported'
    e2, gv, gt, _, _ = S.energies_grad(case['verts'], case['trans'], case['points'], case['sigma'], case['w_s2m'], case['w_m2s'], near_v=nv, near_p=npt)
    ok = e2 > 0
    e_en = float(((got['energy2'].double() - e2).abs() / e2.abs().clamp_min(1e-300))[ok].max()) if bool(ok.any()) else 0.0
    assert bool((got['energy2'][~ok] == 0).all())
    e_gv = float((got['dverts'].double() - gv).abs().max() / gv.abs().max().clamp_min(1e-300))
    e_gt = float((got['dtrans'].double() - gt).abs().max() / gt.abs().max().clamp_min(1e-300))
    print('%s: %d of %d indices differ (worst excess %.2e), energy rel %.2e, dverts rel-to-max %.2e, dtrans rel-to-max %.2e'
          % (name, differ, total, worst, e_en, e_gv, e_gt))
    assert e_en < 1e-5 and e_gv < 1e-4 and e_gt < 1e-4, (name, e_en, e_gv, e_gt)


@pytest.mark.parametrize('name', sorted(S.SPECS))
def test_two_calls_and_a_row_stride_agree(dev, name):
    got = whole(dev, name)
    assert same(got, run(dev, S.get_case(name))) and same(got, run(dev, S.get_case(name), ld_trans=157))


@pytest.mark.parametrize('name', ['v63_p65_nan_body', 'v257_p1025', 'v65_p70_s2m_only', 'v65_p70_m2s_only', 'v6890_p16384'])
def test_a_body_alone_equals_the_body_in_its_batch(dev, name):
    case, got = S.get_case(name), whole(dev, name)
    for b in range(3):
        alone = run(dev, case, bodies=slice(b, b + 1))
        assert same(alone, {k: v[b:b + 1] for k, v in got.items()}), (name, b)


@pytest.mark.parametrize('name', ['v63_p65_nan_body', 'v257_p1025_ties', 'v1025_p257', 'v65_p70_s2m_only'])
def test_each_output_alone(dev, name):
    case, got = S.get_case(name), whole(dev, name)
    for k in ALL:
        one = run(dev, case, outputs=(k,))
        assert torch.equal(_bits(one[k]), _bits(got[k])), (name, k)


@pytest.mark.parametrize('name', ['v63_p65_nan_body', 'v257_p1025', 'v1025_p257'])
def test_a_graph_replay_agrees(dev, name):
    case, got = S.get_case(name), whole(dev, name)
    verts, trans, points = (case[k].to(dev) for k in ('verts', 'trans', 'points'))
    B, V, N = verts.shape[0], verts.shape[1], points.shape[1]
    z = Zone(dev)
    out = {'energy2': z.guarded((B, 2)), 'dverts': z.guarded((B, V, 3)), 'dtrans': z.guarded((B, 3)),
           'nearest_vertex': z.guarded((B, N), dtype=torch.int32, fill=-77), 'nearest_point': z.guarded((B, V), dtype=torch.int32, fill=-77)}
    ws = z.guarded((hipabi.lib().straps_scan_energy_workspace_bytes(B, V, N) // 4,), name='workspace')
    opts = hipabi.ScanOptsStruct(case['sigma'], case['w_s2m'], case['w_m2s'])
    call = lambda: scan_energy_raw(verts, trans, 3, points, opts, out['energy2'], out['dverts'], out['dtrans'], out['nearest_vertex'], out['nearest_point'], ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in out.values():
        t.fill_(-77)
    graph.replay()
    torch.cuda.synchronize()
    z.check()
    assert same({k: t.cpu() for k, t in out.items()}, got), name
