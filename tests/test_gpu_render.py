"""GPU: straps_render_mesh (csrc/render.hip) against the restatements of tests/render_cases.py.  Which face a pixel shows, the mask and
the depth are compared with the float32 restatement bit for bit (the depth as bit patterns) on every case; the mask also with
straps_wp_silhouette on the same inputs; the colours with the float64 oracle: exact where nothing covers, within ONE byte level per
channel where something does.  That bound is derived, not measured: the float32 shading chain carries an error of some 1e-6 (the cases
compared meet the normal-length condition of tests/test_render_cases_cpu.py), a byte level is 1 / 255 = 3.9e-3 wide, so the float32
and float64 values lie on the same side of all rounding boundaries but at most one.  Every output and the workspace sit between redzone
margins, pre-filled with a pattern the kernels never write; inputs end directly in front of poison.  Then the module surface:
WeakPerspectiveMeshRenderer, Predictor.render on the committed predict fixtures, and the drop-in Renderer."""
import ctypes

import numpy as np
import pytest
import torch

import predict_cases as PC
import render_cases as RC
import straps_amd
from redzone import Zone
from straps_amd import hipabi
from straps_amd.weak_perspective_pyrender_renderer import Renderer

pytestmark = pytest.mark.gpu
MP = straps_amd.synthetic_mean_params(0)
MODEL = straps_amd.synthetic_smpl_model(0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _opts_struct(opts):
    o = hipabi.RenderOptsStruct()
    o.colour[:] = [float(c) for c in opts['colour']]
    o.ambient = float(opts['ambient'])
    o.background[:] = [float(c) for c in opts['background']]
    d = np.asarray(opts['light_dir'], np.float32).reshape(-1, 3)
    o.n_lights = d.shape[0]
    o.light_dir[:d.size] = [float(x) for x in d.reshape(-1)]
    o.light_intensity[:d.shape[0]] = [float(x) for x in np.asarray(opts['light_intensity'], np.float32)]
    return o


def _render(dev, c, opts=RC.DEFAULT_OPTS, background=None, aux=True):
    """the raw call on guarded outputs + workspace, operands ending in front of poison -> dict of numpy arrays ('rgb', and with aux 'mask',
    'depth', 'face_ids')"""
    verts, faces, cam, wh, rot = c['verts'], c['faces'], c['cam'], c['wh'], c['rotation']
    B, N = verts.shape[0], verts.shape[1]
    L = hipabi.lib()
    z = Zone(dev)
    rgb = z.guarded((B, wh, wh, 3), dtype=torch.uint8, fill=0xAB, name='rgb')
    mask = z.guarded((B, wh, wh), dtype=torch.uint8, fill=0xAB, name='mask') if aux else None
    depth = z.guarded((B, wh, wh), name='depth') if aux else None
    fid = z.guarded((B, wh, wh), dtype=torch.int32, fill=-77, name='face_ids') if aux else None
    ws_bytes = L.straps_render_mesh_workspace_bytes(B, N, wh)
    assert ws_bytes == B * (8 * wh * wh + 32 * N)
    ws = z.guarded((ws_bytes // 4,), name='workspace')
    assert ws.data_ptr() % 8 == 0
    offsets, table = RC.csr_table(faces, N)
    if table.size == 0:
        table = np.zeros(1, np.int32)                    # (no vertex has a face: never read, but the library wants a pointer)
    put = lambda a: None if a is None else z.at_end(torch.from_numpy(np.ascontiguousarray(a)))
    v, f, off, tab, cm, r, bg = put(verts), put(faces), put(offsets), put(table), put(cam), put(rot), put(background)
    o = _opts_struct(opts)
    hipabi.check(L.straps_render_mesh(hipabi.ptr(v), hipabi.ptr(f), hipabi.ptr(off), hipabi.ptr(tab), hipabi.ptr(cm), 3, hipabi.ptr(r),
                                      1 if rot is not None and rot.ndim == 3 else 0, ctypes.byref(o), hipabi.ptr(bg), hipabi.ptr(rgb), hipabi.ptr(mask), hipabi.ptr(depth),
                                      hipabi.ptr(fid), hipabi.ptr(ws), B, N, faces.shape[0], wh, hipabi.stream_ptr()), 'straps_render_mesh')
    torch.cuda.synchronize()
    z.check()
    out = {'rgb': rgb.cpu().numpy()}
    if aux:
        out.update(mask=mask.cpu().numpy(), depth=depth.cpu().numpy(), face_ids=fid.cpu().numpy())
    return out


def _silhouette(dev, c):
    verts, faces, cam, wh = c['verts'], c['faces'], c['cam'], c['wh']
    B, N = verts.shape[0], verts.shape[1]
    L = hipabi.lib()
    z = Zone(dev)
    mask = z.guarded((B, wh, wh), dtype=torch.uint8, fill=0xAB, name='mask')
    ws = z.guarded((L.straps_wp_silhouette_workspace_bytes(B, N) // 4,), name='workspace')
    v, f, cm = z.at_end(torch.from_numpy(verts)), z.at_end(torch.from_numpy(faces)), z.at_end(torch.from_numpy(cam))
    hipabi.check(L.straps_wp_silhouette(hipabi.ptr(v), hipabi.ptr(f), hipabi.ptr(cm), hipabi.ptr(mask), hipabi.ptr(ws), B, N, faces.shape[0], wh,
                                        hipabi.stream_ptr()), 'straps_wp_silhouette')
    torch.cuda.synchronize()
    z.check()
    return mask.cpu().numpy()


def _assert_geometry(got, ref, what):
    assert got['face_ids'].dtype == np.int32 and got['mask'].dtype == np.uint8 and got['depth'].dtype == np.float32
    assert np.array_equal(got['face_ids'], ref['face_ids']), '%s: %d face ids differ from the restatement' % (what, int((got['face_ids'] != ref['face_ids']).sum()))
    assert np.array_equal(got['mask'], ref['mask']), '%s: the mask differs' % what
    gd, rd = got['depth'].view(np.uint32), ref['depth'].view(np.uint32)
    assert np.array_equal(gd, rd), '%s: %d depths differ in their bits' % (what, int((gd != rd).sum()))


def _assert_colours(rgb, want, hit, shaded, what):
    """exact where nothing covers; within one level where something does (shaded cases only)"""
    assert rgb.dtype == np.uint8 and rgb.shape == want.shape
    assert np.array_equal(rgb[~hit], want[~hit]), '%s: a background pixel differs' % what
    if shaded and hit.any():
        diff = np.abs(rgb[hit].astype(np.int64) - want[hit].astype(np.int64))
        print('%s: %d covered pixels, %d channel values one level off, worst %d' % (what, int(hit.sum()), int((diff == 1).sum()), int(diff.max())))
        assert diff.max() <= 1, '%s: a colour is %d levels from the float64 oracle' % (what, int(diff.max()))


@pytest.mark.parametrize('name', RC.CASES)
def test_case_equals_the_restatements(dev, name):
    c = RC.case(name)
    ref, shaded = c['ref'], name in RC.SHADED_CASES
    hit = ref['mask'] == 1
    B, wh = c['verts'].shape[0], c['wh']
    # the defaults over the constant background colour, every output asked for
    got = _render(dev, c)
    _assert_geometry(got, ref, name)
    if c['expected_ids'] is not None:
        assert np.array_equal(got['face_ids'], c['expected_ids']), '%s: the hand count' % name
    if c['rotation'] is None:
        assert np.array_equal(got['mask'], _silhouette(dev, c)), '%s: mask and straps_wp_silhouette differ' % name
    want = RC.oracle(name)['rgb'] if shaded else np.broadcast_to(RC.quantise(np.asarray(RC.DEFAULT_OPTS['background'], np.float32)), (B, wh, wh, 3))
    _assert_colours(got['rgb'], want, hit, shaded, name + ' (defaults)')
    # other colours and three lights over a background picture, no optional output
    bg = RC.background_image(B, wh)
    got2 = _render(dev, c, RC.OTHER_OPTS, background=bg, aux=False)
    want2 = RC.oracle(name, 'other', True)['rgb'] if shaded else bg
    _assert_colours(got2['rgb'], want2, hit, shaded, name + ' (three lights, over a picture)')
    if name == 'cameras_wh20':
        assert 0 < hit[0].sum() < hit[1].sum() < hit[2].sum()
    if name.startswith('border_'):
        assert hit[0, :, 0].any() and hit[0, :, -1].any() and hit[0, 0].any() and hit[0, -1].any()
    if name == 'smpl_wh64':
        assert c['faces'].shape[0] == 13776 and 0 < hit.sum() < 64 * 64 and len(np.unique(got['face_ids'])) > 300


@pytest.mark.parametrize('name', ('sphere_wh20', 'rotation_per_body', 'pair_negative_a_in_front'))
def test_optional_outputs_do_not_change_the_picture(dev, name):
    c = RC.case(name)
    bg = RC.background_image(c['verts'].shape[0], c['wh'], seed=77)
    for opts, background in ((RC.DEFAULT_OPTS, None), (RC.OTHER_OPTS, bg)):
        with_aux, without = _render(dev, c, opts, background, aux=True), _render(dev, c, opts, background, aux=False)
        assert np.array_equal(with_aux['rgb'], without['rgb'])
        _assert_geometry(with_aux, c['ref'], name)


def test_no_normal_fallback(dev):
    """every vertex normal of this mesh is exactly zero: each covered pixel takes (0, 0, -1), turned away where the winning face's own
    normal has positive z -- there only the ambient term is left.  Both branches are exact in float32 and float64 alike."""
    c = RC.case('no_normal')
    got = _render(dev, c, RC.OTHER_OPTS)
    _assert_geometry(got, c['ref'], 'no_normal')
    hit, flip = c['ref']['mask'][0] == 1, c['ref']['flip'][0]
    assert hit.sum() == 45 and (hit & flip).any() and (hit & ~flip).any()
    want = RC.oracle('no_normal', 'other')
    assert want['fallback'][0][hit].all()
    assert np.abs(got['rgb'].astype(np.int64) - want['rgb'].astype(np.int64)).max() <= 1
    col, amb = np.asarray(RC.OTHER_OPTS['colour'], np.float32), np.float32(RC.OTHER_OPTS['ambient'])
    assert (got['rgb'][0][hit & flip] == RC.quantise32(col * amb)).all()
    lam = amb                                     # the kernel's sum, light by light, for n = (0, 0, -1)
    for d, i in zip(np.asarray(RC.OTHER_OPTS['light_dir'], np.float32), np.asarray(RC.OTHER_OPTS['light_intensity'], np.float32)):
        dot = -d[2]                               # (0 * dx + 0 * dy) + (-1) * dz
        lam = lam + i * max(dot, np.float32(0))
    assert (got['rgb'][0][hit & ~flip] == RC.quantise32(col * min(lam, np.float32(1)))).all()


@pytest.mark.parametrize('ambient', (0.3, 0.75, 1.0, 2.5))
def test_no_lights_leaves_the_ambient_term_exactly(dev, ambient):
    c = RC.case('grid256_wh20')
    opts = dict(RC.OTHER_OPTS, ambient=ambient, light_dir=np.zeros((0, 3), np.float32), light_intensity=np.zeros((0,), np.float32))
    got = _render(dev, c, opts)
    _assert_geometry(got, c['ref'], 'no lights')
    hit = c['ref']['mask'] == 1
    flat = RC.quantise32(np.asarray(opts['colour'], np.float32) * min(np.float32(ambient), np.float32(1)))
    assert hit.sum() > 100 and (got['rgb'][hit] == flat).all()
    assert (got['rgb'][~hit] == RC.quantise32(np.asarray(opts['background'], np.float32))).all()


# ---- through the modules -----------------------------------------------------------------------------------------------------------
def _module(dev, name, **kw):
    c = RC.case(name)
    rend = straps_amd.WeakPerspectiveMeshRenderer(c['faces'], img_wh=c['wh'], num_vertices=c['num_vertices'], **kw).to(dev)
    rot = None if c['rotation'] is None else torch.from_numpy(c['rotation']).to(dev)
    return c, rend, torch.from_numpy(c['verts']).to(dev), torch.from_numpy(c['cam']).to(dev), rot


@pytest.mark.parametrize('name', ('rotation_per_body', 'rotation_shared', 'out_of_range_face', 'unreferenced_vertex', 'hand_index_out_of_range_wh16'))
def test_module_equals_the_raw_call_and_itself(dev, name):
    c, rend, v, cam, rot = _module(dev, name)
    assert rend.faces.dtype == torch.int32 and rend.faces.is_cuda and set(dict(rend.named_buffers())) == {'faces', 'vf_offsets', 'vf_faces'}
    a, b = rend(v, cam, rotation=rot, return_aux=True), rend(v, cam, rotation=rot, return_aux=True)
    assert set(a) == {'rgb', 'mask', 'depth', 'face_ids'}
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k                       # two calls, equal bits
    raw = _render(dev, c)
    got = {k: t.cpu().numpy() for k, t in a.items()}
    _assert_geometry(got, c['ref'], name + ' (module)')
    assert np.array_equal(got['rgb'], raw['rgb'])
    plain = rend(v, cam, rotation=rot)
    assert plain.dtype == torch.uint8 and tuple(plain.shape) == (v.shape[0], c['wh'], c['wh'], 3) and torch.equal(plain, a['rgb'])
    with pytest.raises(RuntimeError):
        rend(v[:, :-1], cam)
    with pytest.raises(RuntimeError):
        rend(v, cam[:, :2])


def test_module_options_and_non_contiguous_background(dev):
    o = RC.OTHER_OPTS
    lights = tuple((tuple(3.0 * d), float(i)) for d, i in zip(np.asarray(o['light_dir'], np.float64), o['light_intensity']))      # not unit: normalised by the module
    c, rend, v, cam, rot = _module(dev, 'rotation_per_body', colour=o['colour'], ambient=o['ambient'], lights=lights, background=o['background'])
    B, wh = v.shape[0], c['wh']
    hit = c['ref']['mask'] == 1
    _assert_colours(rend(v, cam, rotation=rot).cpu().numpy(), RC.oracle('rotation_per_body', 'other')['rgb'], hit, True, 'module, constant background')
    bg = RC.background_image(B, wh)
    wide = torch.zeros(B, wh, 2 * wh, 3, dtype=torch.uint8, device=dev)
    wide[:, :, ::2] = torch.from_numpy(bg).to(dev)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    over = rend(v, cam, background=view, rotation=rot)
    assert torch.equal(over, rend(v, cam, background=view.contiguous(), rotation=rot))
    _assert_colours(over.cpu().numpy(), RC.oracle('rotation_per_body', 'other', True)['rgb'], hit, True, 'module, strided background picture')
    with pytest.raises(RuntimeError):
        rend(v, cam, background=view[:, :-1])
    with pytest.raises(RuntimeError):
        rend(v, cam, background=view.float())


@pytest.fixture(scope='module')
def prediction(dev):
    """the seeded regressor and inputs of tests/test_gpu_predictor.py: three frames of the committed predict fixtures"""
    B = 3
    torch.manual_seed(18)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=MP).to(dev).eval()
    smpl = straps_amd.SMPL(MODEL, batch_size=B).to(dev)
    sil, joints = PC.inputs('a')
    pred = straps_amd.Predictor(reg, smpl)
    out = pred(torch.from_numpy(sil[:B]).to(dev), torch.from_numpy(joints[:B]).to(dev))
    return pred, smpl, out


def test_predictor_render(dev, prediction):
    pred, smpl, out = prediction
    B, wh = 3, 256
    rend = straps_amd.WeakPerspectiveMeshRenderer(MODEL['faces'], img_wh=wh).to(dev)
    images = torch.from_numpy(RC.background_image(B, wh, seed=9)).to(dev)
    pics = pred.render(out, rend, images)
    assert set(pics) == {'rend', 'reposed'}
    for k in pics:
        assert pics[k].dtype == torch.uint8 and tuple(pics[k].shape) == (B, wh, wh, 3)
    direct = rend(out['vertices'], out['cam_wp'], background=images, return_aux=True)
    assert torch.equal(pics['rend'], direct['rgb'])
    covered = direct['mask'].bool()
    assert (covered.flatten(1).sum(1) > 0).all() and not covered.all()
    assert torch.equal(pics['rend'][~covered], images[~covered])
    assert np.array_equal(direct['mask'].cpu().numpy(), straps_amd.WeakPerspectiveSilhouetteRenderer(MODEL['faces'], img_wh=wh).to(dev)(
        out['vertices'], out['cam_wp']).cpu().numpy())
    cam = torch.tensor([[0.8, 0.0, -0.2]], device=dev).expand(B, 3).contiguous()
    rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]], device=dev)
    rep = rend(out['reposed_vertices'], cam, rotation=rx, return_aux=True)
    assert torch.equal(pics['reposed'], rep['rgb'])
    assert (rep['mask'].flatten(1).sum(1) > 0).all() and not pics['reposed'][~rep['mask'].bool()].any()      # over the black background colour
    # without pictures: over the background colour; a second call gives the same bits
    plain = pred.render(out, rend)
    assert torch.equal(plain['reposed'], pics['reposed']) and torch.equal(plain['rend'][covered], pics['rend'][covered]) and not plain['rend'][~covered].any()
    again = pred.render(out, rend, images)
    assert torch.equal(again['rend'], pics['rend']) and torch.equal(again['reposed'], pics['reposed'])
    with pytest.raises(ValueError):
        pred.render(out, straps_amd.WeakPerspectiveMeshRenderer(MODEL['faces'], img_wh=128).to(dev), images)
    # on the result of refine as well
    fitted = pred.refine(out, straps_amd.KeypointFitter(smpl, iters=2))
    fp = pred.render(fitted, rend, images)
    assert torch.equal(fp['rend'], rend(fitted['vertices'], fitted['cam_wp'], background=images))
    assert torch.equal(fp['reposed'], rend(fitted['reposed_vertices'], cam, rotation=rx))


def test_drop_in_renderer(dev, prediction, tmp_path):
    pred, smpl, out = prediction
    wh = 64
    verts, cam = out['vertices'][0].cpu().numpy(), out['cam_wp'][0].cpu().numpy()
    r = Renderer(resolution=(wh, wh), faces=MODEL['faces'])
    module = straps_amd.WeakPerspectiveMeshRenderer(MODEL['faces'], img_wh=wh).to(dev)
    v, cm = out['vertices'][:1].contiguous(), out['cam_wp'][:1].contiguous()
    img = RC.background_image(1, wh, seed=3)[0]
    want = module(v, cm, background=torch.from_numpy(img)[None].to(dev), return_aux=True)
    got = r.render(verts, cam, img=img)
    assert got.dtype == np.uint8 and got.shape == (wh, wh, 3) and np.array_equal(got, want['rgb'][0].cpu().numpy())
    mask = r.render(verts, cam, return_mask=True)
    assert mask.dtype == bool and mask.shape == (wh, wh) and mask.any() and np.array_equal(mask, want['mask'][0].cpu().numpy() != 0)
    assert np.array_equal(r.render(verts, np.array([cam[0], cam[0], cam[1], cam[2]], np.float32), img=img), got)      # (sx, sy, tx, ty), sx == sy
    with pytest.raises(ValueError, match='sx'):
        r.render(verts, np.array([cam[0], 2 * cam[0], cam[1], cam[2]], np.float32))
    # another colour, handed through in the caller's channel order
    blue = r.render(verts, cam, color=[0.2, 0.3, 0.9])
    assert np.array_equal(blue, module(v, cm, colour=(0.2, 0.3, 0.9))[0].cpu().numpy()) and not np.array_equal(blue, r.render(verts, cam))
    # predict_3D.py:171-174: the reposed mesh, turned by 180 degrees about x after the reference's own turn
    reposed = out['reposed_vertices'][0].cpu().numpy()
    rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]], device=dev)
    want = module(out['reposed_vertices'][:1].contiguous(), torch.tensor([[0.8, 0.0, -0.2]], device=dev), rotation=rx)[0].cpu().numpy()
    got = r.render(reposed, np.array([0.8, 0.0, -0.2]), angle=180, axis=[1, 0, 0])
    assert np.array_equal(got, want) and got.any()
    assert not np.array_equal(got, r.render(reposed, np.array([0.8, 0.0, -0.2])))
    # the mesh file: a plain OBJ of the turned mesh
    path = tmp_path / 'mesh.obj'
    r.render(verts, cam, mesh_filename=str(path))
    lines = path.read_text().split('\n')
    vs, fs = [l for l in lines if l.startswith('v ')], [l for l in lines if l.startswith('f ')]
    assert len(vs) == 6890 and len(fs) == 13776
    first = np.array(vs[0].split()[1:], np.float64)
    assert np.allclose(first, verts[0].astype(np.float64) * [1, -1, -1], atol=1e-7) and fs[0].split()[1:] == [str(int(i) + 1) for i in MODEL['faces'][0]]
    with pytest.raises(ValueError):
        r.render(verts, cam, mesh_filename=str(tmp_path / 'mesh.ply'))
    with pytest.raises(ValueError):
        Renderer(resolution=(64, 48), faces=MODEL['faces'])
