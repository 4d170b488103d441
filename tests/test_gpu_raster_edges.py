"""GPU: straps_rasterize_parts (csrc/raster.hip) off the 256-pixel frame, against the BRUTE FORCE of tests/datagen_cases.py -- every face
tested at every pixel centre, no bounding box, no cull -- bit for bit in parts and depth: frames of 1 to 100 pixels (powers of two and the
division branch of raster_face_kernel), faces whose edges pass exactly through samples, slivers, boxes narrower than, as wide as and much
wider than the 16 lanes that share a face, faces across and outside every frame edge, every way the depth test can reject a face, vertex
indices out of range.  The raw C entry runs on buffers of the test: parts, depth and the workspace of exactly the advertised size sit
between redzone margins, pre-filled with NaN; every operand ends directly in front of a poisoned margin."""
import numpy as np
import pytest
import torch

import datagen_cases as DC
import straps_oracle as O
from detgen import det_uniform
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _at_end(dev, a, fill):
    """an int32 / uint8 operand whose last element is directly followed by a margin of `fill` (a repeating pattern), and preceded by it"""
    a = np.array(a)
    pat = np.asarray(fill, a.dtype).ravel()
    front, back = 64 * pat.size, 4096 * pat.size
    base = torch.from_numpy(np.tile(pat, 64 + -(-a.size // pat.size) + 4096)[:front + a.size + back].copy()).to(dev)
    v = base[front:front + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


class Call:
    """one scene's operands on the device, placed once; run() makes a fresh set of guarded outputs"""

    def __init__(self, dev, scene, wh, cam_per_body=False, noise_u=None):
        verts, faces, parts, K, R, t = scene
        self.dev, self.wh, self.B, self.N, self.F = dev, wh, verts.shape[0], verts.shape[1], faces.shape[0]
        self.cam_per_body = int(cam_per_body)
        f32 = lambda a: torch.from_numpy(np.array(a, np.float32))                # (a copy: the cached scenes are read-only)
        z = Zone(dev)
        if cam_per_body:
            K, R = np.broadcast_to(K, (self.B, 3, 3)), np.broadcast_to(R, (self.B, 3, 3))
        assert K.shape == R.shape == ((self.B, 3, 3) if cam_per_body else (3, 3)) and t.shape == (self.B, 3)
        self.verts, self.K, self.R, self.t = z.at_end(f32(verts)), z.at_end(f32(K)), z.at_end(f32(R)), z.at_end(f32(t))
        # behind the faces: indices of three different faces' corners; behind the part table: part 255 -- a face or a part read past the end SHOWS
        self.faces = _at_end(dev, np.asarray(faces, np.int32), (0, 4, 8))
        self.face_parts = _at_end(dev, np.asarray(parts, np.uint8), (255,))
        self.noise_u = None if noise_u is None else z.at_end(f32(noise_u))
        self.ws_bytes = hipabi.lib().straps_rasterize_workspace_bytes(self.B, self.N, wh)
        assert self.ws_bytes == self.B * (wh * wh * 8 + self.N * 12)

    def run(self, want_parts=True, want_depth=True, workspace=None, near=DC.NEAR, far=DC.FAR, noise=(-0.01, 0.01)):
        """-> (parts, depth) numpy (None where not requested); margins checked, no NaN left in an output"""
        z = Zone(self.dev)
        B, wh = self.B, self.wh
        parts = z.guarded((B, wh, wh), name='parts') if want_parts else None
        depth = z.guarded((B, wh, wh), name='depth') if want_depth else None
        ws = z.guarded((self.ws_bytes // 4,), name='workspace') if workspace is None else workspace
        self.workspace, self.zone = ws, z
        hipabi.check(hipabi.lib().straps_rasterize_parts(
            hipabi.ptr(self.verts), hipabi.ptr(self.faces), hipabi.ptr(self.face_parts), hipabi.ptr(self.K), hipabi.ptr(self.R), hipabi.ptr(self.t),
            hipabi.ptr(parts), hipabi.ptr(depth), hipabi.ptr(ws), B, self.N, self.F, wh, self.cam_per_body, near, far, hipabi.ptr(self.noise_u),
            noise[0], noise[1], hipabi.stream_ptr()), 'straps_rasterize_parts')
        torch.cuda.synchronize()
        z.check()
        out = [None if o is None else o.cpu().numpy() for o in (parts, depth)]
        for o in out:
            assert o is None or not np.isnan(o).any(), 'an output pixel was not written'
        return out


def _assert_equal(got, want, what):
    for g, w, name in zip(got, want, ('parts', 'depth')):
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(g, w), '%s: %d of %d %s pixels differ from the brute force' % (what, int((g != w).sum()), g.size, name)


@pytest.mark.parametrize('wh', DC.RASTER_WH)
@pytest.mark.parametrize('family', DC.FAMILIES)
def test_bit_exact_against_the_brute_force(dev, family, wh):
    """every family, frame size and batch: parts and depth equal rasterize_brute exactly.  For `bad_indices` the reference is the scene with
    the faces that hold an index of -1 or nverts made degenerate: the kernel skips them, and the margins stay intact"""
    for B in DC.RASTER_B:
        got = Call(dev, DC.scene(family, wh, B), wh).run()
        _assert_equal(got, DC.brute_reference(family, wh, B), '%s, wh %d, B %d' % (family, wh, B))


@pytest.mark.parametrize('family,wh', [('on_centre', 33), ('strips', 100), ('depth', 48), ('tiny', 5), ('bad_indices', 64)])
def test_per_body_cameras_output_selection_and_determinism(dev, family, wh):
    """the same scene under per-body copies of the camera; parts only, depth only and both give the same values; a second call into the
    SAME workspace, not refilled, gives the same result"""
    B = 3
    want = DC.brute_reference(family, wh, B)
    shared, per_body = Call(dev, DC.scene(family, wh, B), wh), Call(dev, DC.scene(family, wh, B), wh, cam_per_body=True)
    for call in (shared, per_body):
        both = call.run()
        _assert_equal(both, want, '%s, wh %d' % (family, wh))
        ws, first_zone = call.workspace, call.zone
        again = call.run(workspace=ws)
        _assert_equal(again, want, '%s, wh %d, second call into the same workspace' % (family, wh))
        first_zone.check()
        only_parts, none = call.run(want_depth=False)
        assert none is None and np.array_equal(only_parts, want[0])
        none, only_depth = call.run(want_parts=False, workspace=ws)
        assert none is None and np.array_equal(only_depth, want[1])


def test_rotated_per_body_cameras_and_a_single_face(dev):
    """per-body K, R != I and t != 0 (body 2 crosses the near plane): the brute force on the same cameras; and B = F = 1"""
    scene = DC.rotated_camera_scene()
    want = DC.rasterize_brute(*scene, 48, return_depth=True)
    call = Call(dev, scene, 48, cam_per_body=True)
    _assert_equal(call.run(), want, 'rotated per-body cameras')
    assert ((want[0] > 0).mean(axis=(1, 2)) > 0.1).all()
    scene = DC.single_face_scene()
    want = DC.rasterize_brute(*scene, 5, return_depth=True)
    _assert_equal(Call(dev, scene, 5).run(), want, 'one body, one face')
    assert (want[0] > 0).all()


@pytest.mark.parametrize('wh', (33, 64))
def test_fused_vertex_noise(dev, wh):
    """the projection kernel's vertex noise: the result equals the brute force on O.random_verts2D_deviation of the same uniforms (0.01
    camera units are 0.3 to 0.6 px here: samples change hands)"""
    B = 3
    for family in ('on_centre', 'tiny'):
        verts, faces, parts, K, R, t = DC.scene(family, wh, B)
        u = det_uniform((B, verts.shape[1], 2), 77 + wh, 0.0, 1.0)
        u[0, 0], u[0, 1] = (0.0, DC.LAST_DRAW), (DC.LAST_DRAW, 0.0)
        noisy = O.random_verts2D_deviation(verts.copy(), u, (-0.01, 0.01)).numpy()
        want = DC.rasterize_brute(noisy, faces, parts, K, R, t, wh, return_depth=True)
        assert not np.array_equal(want[0], DC.brute_reference(family, wh, B)[0])                  # the noise reaches the part map
        got = Call(dev, (verts, faces, parts, K, R, t), wh, noise_u=u).run(noise=(-0.01, 0.01))
        _assert_equal(got, want, '%s with vertex noise, wh %d' % (family, wh))


def test_argument_errors_write_nothing(dev):
    """wh = 0, wh = 4097, far <= near, neither output requested: nonzero, the outputs and the workspace still hold their fill, margins intact"""
    wh, B = 33, 1
    call = Call(dev, DC.scene('tiny', wh, B), wh)
    L = hipabi.lib()
    assert L.straps_rasterize_workspace_bytes(B, call.N, 0) == 0

    def attempt(wh_arg, near, far, want_parts=True, want_depth=True):
        z = Zone(dev)
        parts, depth, ws = z.guarded((B, wh, wh), name='parts'), z.guarded((B, wh, wh), name='depth'), z.guarded((call.ws_bytes // 4,), name='workspace')
        rc = L.straps_rasterize_parts(hipabi.ptr(call.verts), hipabi.ptr(call.faces), hipabi.ptr(call.face_parts), hipabi.ptr(call.K), hipabi.ptr(call.R),
                                      hipabi.ptr(call.t), hipabi.ptr(parts if want_parts else None), hipabi.ptr(depth if want_depth else None),
                                      hipabi.ptr(ws), B, call.N, call.F, wh_arg, 0, near, far, None, 0.0, 0.0, hipabi.stream_ptr())
        torch.cuda.synchronize()
        z.check()
        for o in (parts, depth, ws):
            assert bool(torch.isnan(o).all()), 'a refused call wrote to a buffer'
        return rc, L.straps_last_error()
    for args, message in (((0, DC.NEAR, DC.FAR), b'bad sizes'), ((4097, DC.NEAR, DC.FAR), b'bad sizes'), ((wh, 1.0, 1.0), b'near < far'),
                          ((wh, 2.0, 1.0), b'near < far'), ((wh, DC.NEAR, DC.FAR, False, False), b'neither parts nor depth')):
        rc, err = attempt(*args)
        assert rc != 0 and message in err, (args, rc, err)
    _assert_equal(call.run(), DC.brute_reference('tiny', wh, B), 'the same operands, accepted')
