"""GPU: straps_silhouette_energy (csrc/silfit.hip) against the float64 restatement of tests/silfit_cases.py: energy2, dverts, dcam, nearest.

Every output and the workspace sit behind redzone guards, every input ends against a NaN margin; the distance field handed to the kernel is the
CPU's (two_pass_d2), so that this file tests the energy alone.  The cases (silfit_cases.ENERGY_SPECS) cover nverts 1, 63, 64, 65, 257, 6890,
7000 (more than the 6912 vertices one LDS tile of the search holds) and 65537 (ten tiles, and 257 partial sums for the finish to add in two
strided trips), wh 2, 16, 33, 96, 256, 320 and 1024 (the limit), lattice 1, 2, 3, 4, 8 and wh + 1 (a single point), tau 0 and 1.5, batches of 1
and 3, vertices beyond every side and corner, an empty mask inside a batch, foreground without a valid lattice point, and two vertices at one
position.  Three cases have more chunks of 256 lattice points than the 32 workgroups the search gives a body -- 36 (workgroups 0..3 walk two
chunks, the others one; once with one vertex tile and once with two, so that the barriers and tile reloads run inside the chunk loop), 45 and 64
(two whole trips each).  tests/test_silfit_cases_cpu.py asserts the input conditions that keep fp32 and float64 on the same branch, and
(test_energy_cases_reach_every_path) that the cases reach each of these paths.

`nearest`: for EVERY valid lattice point the reported vertex's float64 distance must be within 1e-5 relative of the true minimum; the float64
energies and gradients are then evaluated with the reported vertices.
Bounds: energies 1e-5 relative, gradients 1e-4 of the largest magnitude in the tensor (the keypoint fit's bars; an fp32 mean of n terms is
off by at most n * 2^-23 relative in the worst case, 8e-4 at 6890 vertices).
Measured on MI355X, worst over all cases: nearest excess 0 (the float64 vertex everywhere), energy 1.6e-6 (the mean over 65537 vertices, whose
worst case by that model is 7.8e-3; 8.1e-7 over the other cases), dverts 6.2e-6, dcam 8.6e-7 -- all below a third of their bounds.  The cases
beyond 8192 lattice points, 256 pixels or 65536 vertices alone: energy 1.6e-6, dverts 5.0e-6, dcam 3.9e-7 (DESIGN.md has the same figures)."""
import numpy as np
import pytest
import torch

import silfit_cases as SC
from redzone import Zone
from smpl_cases import cpu_threads
from straps_amd import hipabi
from straps_amd.fit import silhouette_energy_raw

pytestmark = pytest.mark.gpu
W_IN, W_OUT = 100.0, 70.0
ALL = ('energy2', 'dverts', 'dcam', 'nearest')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    torch.set_num_threads(cpu_threads())
    return torch.device('cuda:0')


def at_end_bytes(t, dev):
    n = t.numel()
    base = torch.full((256 + n + 65536,), 255, dtype=torch.uint8, device=dev)
    out = base[256:256 + n].view(t.shape)
    out.copy_(t)
    return out


def run(dev, case, outputs=ALL, bodies=None, ld_cam=3):
    """one raw call on guarded buffers -> dict of CPU tensors"""
    sel = slice(None) if bodies is None else bodies
    verts, cam = case['verts'][sel], case['cam'][sel]
    masks, d2 = torch.from_numpy(case['masks'][sel]), torch.from_numpy(case['d2'][sel])
    B, N, wh, lat = verts.shape[0], verts.shape[1], case['wh'], case['lattice']
    nl = -(-wh // min(lat, wh))
    z = Zone(dev)
    shapes = {'energy2': ((B, 2), torch.float32), 'dverts': ((B, N, 3), torch.float32), 'dcam': ((B, 3), torch.float32), 'nearest': ((B, nl, nl), torch.int32)}
    out = {k: z.guarded(shapes[k][0], dtype=shapes[k][1], fill=float('nan') if shapes[k][1] == torch.float32 else -77, name=k) for k in outputs}
    nbytes = hipabi.lib().straps_silhouette_energy_workspace_bytes(B, N, wh, lat)
    assert nbytes == B * (16 * (N + nl * nl + -(-N // 256)) + 128)
    ws = z.guarded((nbytes // 4,), name='workspace')
    camp = torch.full((B, ld_cam), float('nan'))
    camp[:, :3] = cam
    opts = hipabi.SilFitOptsStruct(wh, lat, case['tau'], W_IN, W_OUT)
    silhouette_energy_raw(z.at_end(verts), z.at_end(camp), ld_cam, at_end_bytes(masks, dev), z.at_end(d2), opts, out.get('energy2'), out.get('dverts'),
                          out.get('dcam'), out.get('nearest'), ws)
    z.check()
    return {k: t.cpu() for k, t in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def check_nearest(case, got):
    """-> worst relative excess of a reported vertex's float64 distance over the true minimum, over every valid lattice point"""
    wh, lat = case['wh'], case['lattice']
    g = SC.grid_coords(case['verts'].double(), case['cam'].double(), wh)
    worst = 0.0
    for b in range(g.shape[0]):
        a, valid = SC.lattice_points(case['masks'][b], lat)
        rep = got['nearest'][b].reshape(-1).long()
        if not case['masks'][b].any():
            assert bool((rep == -1).all())
            continue
        assert bool((rep[~valid] == -1).all()) and bool(((rep[valid] >= 0) & (rep[valid] < g.shape[1])).all()), b
        if not bool(valid.any()):
            continue
        first, d = SC.nearest_vertices(g[b], a[valid])
        r_rep, r_min = d.gather(1, rep[valid][:, None])[:, 0].sqrt(), d.min(dim=1).values.sqrt()
        assert bool((r_min > 0).all()) and bool((r_rep <= r_min * (1 + 1e-5)).all()), (b, 'a reported vertex is not a nearest one')
        worst = max(worst, float(((r_rep - r_min) / r_min).max()))
        if case['tie'] is not None and b == 0:
            i, j = case['tie']
            assert bool((rep == i).any()) and not bool((rep == j).any()), 'of two vertices at one position the lower index is reported'
    return worst


@pytest.mark.parametrize('name', sorted(SC.ENERGY_SPECS))
def test_energy_and_gradients_vs_float64(dev, name):
    case = SC.get_energy_case(name)
    got = run(dev, case)
    e_near = check_nearest(case, got)
    e2, gv, gc, _ = SC.energies_grad(case['verts'].double(), case['cam'].double(), case['masks'], case['d2'], case['lattice'], case['tau'], W_IN, W_OUT,
                                     nearest=got['nearest'])
    ok = e2 > 0
    e_en = float(((got['energy2'].double() - e2).abs() / e2.abs().clamp_min(1e-300))[ok].max()) if bool(ok.any()) else 0.0
    assert bool((got['energy2'][~ok] == 0).all())
    e_gv = float((got['dverts'].double() - gv).abs().max() / gv.abs().max().clamp_min(1e-300))
    e_gc = float((got['dcam'].double() - gc).abs().max() / gc.abs().max().clamp_min(1e-300))
    print('%s: nearest excess %.2e, energy rel %.2e, dverts rel-to-max %.2e, dcam rel-to-max %.2e' % (name, e_near, e_en, e_gv, e_gc))
    assert e_near < 1e-5 and e_en < 1e-5 and e_gv < 1e-4 and e_gc < 1e-4, (name, e_near, e_en, e_gv, e_gc)
    assert not bool(got['dverts'][:, :, 2].any()), 'the z column is written as 0'
    for b in range(case['verts'].shape[0]):
        if not case['masks'][b].any():      # an empty target: both energies 0, every gradient 0
            assert not bool(got['energy2'][b].any()) and not bool(got['dverts'][b].any()) and not bool(got['dcam'][b].any())
    # a second call, and a camera with a leading dimension, give the same bits
    assert same(got, run(dev, case)) and same(got, run(dev, case, ld_cam=157))


@pytest.mark.parametrize('name', ['v63_wh16_l3', 'v65_wh33_l4', 'v6890_wh256_l4', 'v65_wh320_l3'])
def test_a_body_alone_equals_the_body_in_its_batch(dev, name):
    case = SC.get_energy_case(name)
    whole = run(dev, case)
    for b in range(3):
        alone = run(dev, case, bodies=slice(b, b + 1))
        assert same(alone, {k: v[b:b + 1] for k, v in whole.items()}), (name, b)


@pytest.mark.parametrize('name', ['v65_wh33_l4', 'v7000_wh16_l1', 'v7000_wh96_l1'])
def test_each_output_alone(dev, name):
    case = SC.get_energy_case(name)
    whole = run(dev, case)
    for k in ALL:
        one = run(dev, case, outputs=(k,))
        assert torch.equal(_bits(one[k]), _bits(whole[k])), (name, k)
