"""GPU: straps_silhouette_counts (csrc/metrics.hip) against a numpy count, exactly, at the sizes around its wave, workgroup and chunk
boundaries; straps_wp_silhouette (csrc/eval.hip) against the numpy float32 restatement of tests/eval_cases.py, bit for bit; and the two
together through the module surface (renderer -> counts -> IoU).  Every output and workspace sits between redzone margins, pre-filled with
a pattern the kernel never writes: a byte it should have written and did not shows, a write outside damages a margin."""
import numpy as np
import pytest
import torch

import eval_cases as EC
import straps_amd
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu

CHUNK = 16384          # pixels per workgroup of silhouette_counts_kernel (SIL_CHUNK, csrc/metrics.hip)
NPIX = (1, 63, 64, 65, 255, 256, 257, 65536, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 4 * CHUNK + 1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


# ---- counts ------------------------------------------------------------------------------------------------------------------------
def _counts(dev, pred, target):
    """the raw call; each operand's last byte is directly followed by 0xFF bytes (an over-read counts as foreground), the counts start
    from a sentinel"""
    B, npix = pred.shape
    z = Zone(dev)

    def at_end(a):
        base = torch.full((256 + a.size + 4096,), 0xFF, dtype=torch.uint8, device=dev)
        v = base[256:256 + a.size].view(a.shape)
        v.copy_(torch.from_numpy(a))
        return v
    p, t = at_end(pred), at_end(target)
    out = z.guarded((B, 4), dtype=torch.int32, fill=-77, name='counts4')
    hipabi.check(hipabi.lib().straps_silhouette_counts(hipabi.ptr(p), hipabi.ptr(t), hipabi.ptr(out), B, npix, hipabi.stream_ptr()),
                 'straps_silhouette_counts')
    torch.cuda.synchronize()
    z.check()
    return out.cpu().numpy()


def _mask_pairs(B, npix, seed):
    zero, one = np.zeros((B, npix), np.uint8), np.ones((B, npix), np.uint8)
    rnd = lambda s, **kw: EC.random_mask((B, npix), seed + s, **kw)
    return {'zero/zero': (zero, zero), 'one/one': (one, one), 'zero/one': (zero, one), 'one/random': (one, rnd(1)),
            'random/random': (rnd(2), rnd(4, density=0.55)), 'random bytes 2 and 255': (rnd(6, values=(2, 255, 1)), rnd(8, density=0.3, values=(255, 2)))}


@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('npix', NPIX)
def test_counts_equal_numpy(dev, B, npix):
    for what, (p, t) in _mask_pairs(B, npix, 1000 + npix % 977).items():
        got = _counts(dev, p, t)
        want = EC.counts_numpy(p, t)
        assert np.array_equal(got, want), (what, B, npix, got.tolist(), want.tolist())
        assert (got.sum(1) == npix).all()


def test_counts_on_unaligned_frames_and_views(dev):
    """frames that start on odd addresses (a view a few bytes into a buffer): the byte path gives the same counts.  Each operand's last
    byte is directly followed by 0xFF bytes (an over-read counts as foreground), the counts sit between redzone margins"""
    B, npix = 3, 2 * CHUNK + 37
    p, t = EC.random_mask((B, npix), 31), EC.random_mask((B, npix), 33, values=(7, 255))
    want = EC.counts_numpy(p, t)

    def view_at(a, off):
        base = torch.full((256 + off + a.size + 4096,), 0xFF, dtype=torch.uint8, device=dev)
        v = base[256 + off:256 + off + a.size].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == off % 16
        return v
    for off_p, off_t in ((1, 0), (0, 3), (5, 5), (16, 16)):
        z = Zone(dev)
        vp, vt = view_at(p, off_p), view_at(t, off_t)
        out = z.guarded((B, 4), dtype=torch.int32, fill=-5, name='counts4')
        hipabi.check(hipabi.lib().straps_silhouette_counts(hipabi.ptr(vp), hipabi.ptr(vt), hipabi.ptr(out), B, npix, hipabi.stream_ptr()),
                     'straps_silhouette_counts')
        torch.cuda.synchronize()
        z.check()
        assert np.array_equal(out.cpu().numpy(), want), (off_p, off_t)


def test_counts_module_function_on_non_contiguous_masks(dev):
    """a permuted float mask (a comparison keeps its input's strides) and sliced uint8 / bool masks: the module function counts the
    pixels of the tensor it was given, frame by frame, not of the memory behind it"""
    B, H, W = 5, 6, 3
    p, t = EC.random_mask((B, H, W), 61, values=(1, 2, 255)), EC.random_mask((B, H, W), 63, density=0.55)
    want = EC.counts_numpy(p, t)
    assert len({tuple(r) for r in want.tolist()}) > 1                                # frames differ: a mispaired frame shows
    tp, tt = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    hwb = lambda m: m.permute(1, 2, 0).contiguous().permute(2, 0, 1)                # [B,H,W] values over [H,W,B] memory
    fp, ft = hwb(tp.float()), hwb(tt.double())
    assert not fp.is_contiguous() and not (fp != 0).is_contiguous()
    for a, b in ((fp, ft), (fp, tt.float()), (tp.half(), ft), (hwb(tp), hwb(tt != 0))):
        assert np.array_equal(straps_amd.metrics.silhouette_counts(a, b).cpu().numpy(), want)
    wide_p, wide_t = torch.full((B, H + 2, 2 * W + 1), 9, dtype=torch.uint8, device=dev), torch.ones((2 * B, H, W + 4), dtype=torch.bool, device=dev)
    wide_p[:, 1:H + 1, 1:2 * W:2] = tp                                               # sliced in rows, strided in columns
    wide_t[::2, :, 2:W + 2] = tt != 0                                                # every second frame, sliced in columns
    sp, st = wide_p[:, 1:H + 1, 1:2 * W:2], wide_t[::2, :, 2:W + 2]
    assert not sp.is_contiguous() and not st.is_contiguous()
    assert np.array_equal(straps_amd.metrics.silhouette_counts(sp, st).cpu().numpy(), want)
    assert np.array_equal(straps_amd.metrics.silhouette_counts(sp.float(), st).cpu().numpy(), want)


def test_counts_module_function_accepts_float_bool_and_uint8(dev):
    p, t = EC.random_mask((3, 40, 56), 51, values=(1, 2, 255)), EC.random_mask((3, 40, 56), 53)
    want = EC.counts_numpy(p, t)
    tp, tt = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
    for conv in (lambda m: m, lambda m: m != 0, lambda m: m.float(), lambda m: m.double() * 0.25, lambda m: m.half()):
        got = straps_amd.metrics.silhouette_counts(conv(tp), conv(tt))
        assert got.dtype == torch.int32 and got.shape == (3, 4) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        straps_amd.metrics.silhouette_counts(tp.long(), tt.long())


# ---- masks -------------------------------------------------------------------------------------------------------------------------
def _render(dev, verts, faces, cam, wh):
    """the raw call on guarded mask + workspace -> uint8 [B,wh,wh] numpy"""
    B, N = verts.shape[0], verts.shape[1]
    L = hipabi.lib()
    z = Zone(dev)
    mask = z.guarded((B, wh, wh), dtype=torch.uint8, fill=0xAB, name='mask')
    ws_bytes = L.straps_wp_silhouette_workspace_bytes(B, N)
    assert ws_bytes == B * N * 8
    ws = z.guarded((ws_bytes // 4,), name='workspace')
    v, f, c = z.at_end(torch.from_numpy(np.ascontiguousarray(verts, np.float32))), torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev), \
        z.at_end(torch.from_numpy(np.ascontiguousarray(cam, np.float32)))
    hipabi.check(L.straps_wp_silhouette(hipabi.ptr(v), hipabi.ptr(f), hipabi.ptr(c), hipabi.ptr(mask), hipabi.ptr(ws), B, N, faces.shape[0], wh,
                                        hipabi.stream_ptr()), 'straps_wp_silhouette')
    torch.cuda.synchronize()
    z.check()
    return mask.cpu().numpy()


def _assert_mask(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert set(np.unique(got).tolist()) <= {0, 1}, '%s: a mask byte is neither 0 nor 1 (not written?)' % what
    assert np.array_equal(got, want), '%s: %d of %d pixels differ from the restatement' % (what, int((got != want).sum()), got.size)


@pytest.mark.parametrize('name', sorted(EC.hand_mesh_cases()))
def test_hand_counted_masks(dev, name):
    verts, faces, cam, want = EC.hand_mesh_cases(16)[name]
    got = _render(dev, verts, faces, cam, 16)
    _assert_mask(got, want, name)
    _assert_mask(got, EC.wp_silhouette(verts, faces, cam, 16), name + ' (restatement)')


@pytest.mark.parametrize('wh', (16, 20, 256))
def test_border_and_camera_meshes_equal_the_restatement(dev, wh):
    verts, faces = EC.border_mesh()
    got = _render(dev, verts, faces, EC.IDENTITY_CAM, wh)
    _assert_mask(got, EC.wp_silhouette(verts, faces, EC.IDENTITY_CAM, wh), 'border mesh, wh %d' % wh)
    assert got[0, :, 0].any() and got[0, :, -1].any() and got[0, 0].any() and got[0, -1].any()
    verts, faces, cams = EC.camera_batch_case()
    got = _render(dev, verts, faces, cams, wh)
    _assert_mask(got, EC.wp_silhouette(verts, faces, cams, wh), 'blob mesh under three cameras, wh %d' % wh)
    assert 0 < got[0].sum() < got[1].sum() < got[2].sum()
    hand = EC.hand_mesh_cases(16)
    for name in ('right_triangle', 'index_out_of_range', 'degenerate'):      # the hand-made meshes at this size too
        v, f, c, _ = hand[name]
        _assert_mask(_render(dev, v, f, c, wh), EC.wp_silhouette(v, f, c, wh), '%s, wh %d' % (name, wh))


def test_synthetic_smpl_mesh_equals_the_restatement(dev):
    model = straps_amd.synthetic_smpl_model(0)
    verts, faces = model['v_template'][None].astype(np.float32), model['faces']
    assert faces.shape == (13776, 3)
    cam = np.array([[0.9, 0.05, -0.1]], np.float32)
    got = _render(dev, verts, faces, cam, 64)
    _assert_mask(got, EC.wp_silhouette(verts, faces, cam, 64), 'synthetic SMPL mesh')
    assert 0 < got.sum() < 64 * 64


# ---- renderer -> counts -> IoU -----------------------------------------------------------------------------------------------------
def test_iou_of_rendered_silhouettes(dev):
    verts, faces, cams = EC.camera_batch_case()
    rend = straps_amd.WeakPerspectiveSilhouetteRenderer(faces, img_wh=64).to(dev)
    assert rend.faces.dtype == torch.int32 and rend.faces.is_cuda and 'faces' in dict(rend.named_buffers())
    v, c = torch.from_numpy(verts).to(dev), torch.from_numpy(cams).to(dev)
    a, b = rend(v, c), rend(v, c)
    assert a.dtype == torch.uint8 and a.shape == (3, 64, 64) and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), EC.wp_silhouette(verts, faces, cams, 64))
    n = straps_amd.metrics.silhouette_counts(a, b).cpu().numpy().astype(np.float64)
    assert (n[:, 0] > 0).all() and (n[:, 1] == 0).all() and (n[:, 3] == 0).all()
    assert (n[:, 0] / (n[:, 0] + n[:, 1] + n[:, 3]) == 1.0).all()
    shifted = cams.copy()
    shifted[:, 1] += 0.1
    s = rend(v, torch.from_numpy(shifted).to(dev))
    n = straps_amd.metrics.silhouette_counts(s, a).cpu().numpy()
    want = EC.counts_numpy(EC.wp_silhouette(verts, faces, shifted, 64), EC.wp_silhouette(verts, faces, cams, 64))
    assert np.array_equal(n, want)
    iou = n[:, 0] / (n[:, 0] + n[:, 1] + n[:, 3]).astype(np.float64)
    assert ((iou > 0) & (iou < 1)).all(), iou
    assert np.array_equal(iou, want[:, 0] / (want[:, 0] + want[:, 1] + want[:, 3]).astype(np.float64))
    with pytest.raises(RuntimeError):
        rend(v, c[:, :2])
