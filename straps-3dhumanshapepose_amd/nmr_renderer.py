"""Body-part segmentation renderer -- drop-in for reference renderers/nmr_renderer.py:9-100 (class NMRRenderer) in
its `rend_parts_seg=True` configuration, the one the training loop uses (train loop :155).

The reference wraps the third-party CUDA extension `neural_renderer`; here the z-buffer pass and the part look-up
are three HIP kernels behind `straps_rasterize_parts` (csrc/raster.hip).  Same constructor / call surface:

    renderer = NMRRenderer(batch_size, cam_K, cam_R, img_wh=256, rend_parts_seg=True)
    parts = renderer(vertices, cam_ts)            # [B, wh, wh] long, 0 background, 1..6 body parts

Mesh topology and part labels: the reference reads additional/{smpl_faces,vertex_texture,cube_parts}.npy
(config.py).  Those assets are not redistributable; pass `faces` / `face_parts` explicitly (e.g. from
`synthetic_smpl_model()`), or leave them None to load the reference's files from `config`.  The RGB mode
(rend_parts_seg=False, visualisation only) is out of scope and raises.

Beside it, under the weak-perspective camera the regressor predicts: `WeakPerspectiveSilhouetteRenderer` (byte masks for evaluation,
csrc/eval.hip) and `WeakPerspectiveMeshRenderer` (shaded pictures of a prediction, csrc/render.hip).
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import config, hipabi


def face_parts_from_texture(vertex_texture, cube_parts):
    """per-face part id from the reference's assets: vertex_texture [1,F,T,T,T,3] colours decoded through
    cube_parts[floor(100 r), floor(100 g), floor(100 b)] exactly like get_parts (renderers/nmr_renderer.py:93-100);
    a face whose texels disagree (part boundary) takes the majority part, lowest id on ties."""
    vertex_texture = np.asarray(vertex_texture, np.float32)
    tex = vertex_texture.reshape(-1, int(np.prod(vertex_texture.shape[-4:-1])), 3)           # [F][texels][3]
    idx = np.floor(100.0 * tex).astype(np.int64)
    labels = np.asarray(cube_parts)[idx[..., 0], idx[..., 1], idx[..., 2]].astype(np.int64)      # [F, texels]
    counts = np.stack([(labels == k).sum(1) for k in range(7)], axis=1)
    return counts.argmax(1).astype(np.uint8)


class NMRRenderer(nn.Module):
    def __init__(self, batch_size, cam_K, cam_R, img_wh=256, rend_parts_seg=False, faces=None, face_parts=None,
                 near=0.1, far=100.0):
        super().__init__()
        if not rend_parts_seg:
            raise RuntimeError('NMRRenderer: only rend_parts_seg=True (the training-loop configuration) is built; the RGB '
                               'visualisation mode of renderers/nmr_renderer.py is out of scope')
        if faces is None:
            for pth in (config.SMPL_FACES_PATH, config.VERTEX_TEXTURE_PATH, config.CUBE_PARTS_PATH):
                if not os.path.isfile(pth):
                    raise RuntimeError('NMRRenderer: %s not found; pass faces= and face_parts= (e.g. from synthetic_smpl_model())' % pth)
            faces = np.load(config.SMPL_FACES_PATH)
            face_parts = face_parts_from_texture(np.load(config.VERTEX_TEXTURE_PATH), np.load(config.CUBE_PARTS_PATH))
        faces = np.ascontiguousarray(np.asarray(faces).astype(np.int32))
        face_parts = np.ascontiguousarray(np.asarray(face_parts).astype(np.uint8))
        if faces.ndim != 2 or faces.shape[1] != 3 or face_parts.shape != (faces.shape[0],):
            raise RuntimeError('NMRRenderer: faces must be [F,3] and face_parts [F] (got %s, %s)' % (faces.shape, face_parts.shape))
        self.register_buffer('faces', torch.from_numpy(faces))
        self.register_buffer('face_parts', torch.from_numpy(face_parts))
        cam_K = torch.as_tensor(cam_K, dtype=torch.float32)
        cam_R = torch.as_tensor(cam_R, dtype=torch.float32)
        if (cam_K.ndim == 3) != (cam_R.ndim == 3):
            raise RuntimeError('NMRRenderer: cam_K and cam_R must both be [3,3] or both [B,3,3]')
        self.register_buffer('cam_K', cam_K.contiguous())
        self.register_buffer('cam_R', cam_R.contiguous())
        self.batch_size, self.img_wh, self.rend_parts_seg = batch_size, int(img_wh), True
        self.near, self.far = float(near), float(far)

    @hipabi.on_tensor_device
    def render_arrays(self, vertices, cam_ts, want_depth=False, vert_noise_u=None, noise_range=(-0.01, 0.01), out=None):
        """raw entry: vertices [B,N,3], cam_ts [B,3] (fp32 GPU) -> float part map [B,wh,wh] (+ depth).
        vert_noise_u: optional uniforms [B,N,2] in [0,1): the rendered copy of the mesh gets x,y += (h-l)*u + l
        (random_verts2D_deviation, proxy_rep_augmentation.py:5-22) inside the projection kernel."""
        hipabi.require_gpu_tensor(vertices, 'vertices', torch.float32)
        hipabi.require_gpu_tensor(cam_ts, 'cam_ts', torch.float32)
        hipabi.require_gpu_tensor(self.faces, 'NMRRenderer buffers (call .to(device))')
        B, N = vertices.shape[0], vertices.shape[1]
        if cam_ts.ndim == 3:
            cam_ts = cam_ts[:, 0]
        if tuple(vertices.shape) != (B, N, 3) or tuple(cam_ts.shape) != (B, 3):
            raise RuntimeError('NMRRenderer: expected vertices [B,N,3] and cam_ts [B,3] / [B,1,3], got %s and %s'
                               % (tuple(vertices.shape), tuple(cam_ts.shape)))
        per_body = self.cam_K.ndim == 3
        if per_body and self.cam_K.shape[0] != B:
            raise RuntimeError('NMRRenderer: %d cameras for a batch of %d' % (self.cam_K.shape[0], B))
        vertices, cam_ts = vertices.contiguous(), cam_ts.contiguous()
        L = hipabi.lib()
        wh = self.img_wh
        parts = torch.empty(B, wh, wh, device=vertices.device, dtype=torch.float32) if out is None else out
        if vert_noise_u is not None:
            hipabi.require_gpu_tensor(vert_noise_u, 'vert_noise_u', torch.float32)
            if vert_noise_u.numel() != B * N * 2 or not vert_noise_u.is_contiguous():
                raise RuntimeError('NMRRenderer: vert_noise_u must be contiguous [B,N,2] uniforms')
        depth = torch.empty(B, wh, wh, device=vertices.device, dtype=torch.float32) if want_depth else None
        ws = torch.empty(L.straps_rasterize_workspace_bytes(B, N, wh) // 4, device=vertices.device, dtype=torch.float32)
        hipabi.check(L.straps_rasterize_parts(hipabi.ptr(vertices), hipabi.ptr(self.faces), hipabi.ptr(self.face_parts), hipabi.ptr(self.cam_K),
                                              hipabi.ptr(self.cam_R), hipabi.ptr(cam_ts), hipabi.ptr(parts), hipabi.ptr(depth), hipabi.ptr(ws),
                                              B, N, self.faces.shape[0], wh, 1 if per_body else 0, self.near, self.far,
                                              hipabi.ptr(vert_noise_u), float(noise_range[0]), float(noise_range[1]),
                                              hipabi.stream_ptr()), 'straps_rasterize_parts')
        return (parts, depth) if want_depth else parts

    def forward(self, vertices, cam_ts):
        """vertices (B, N, 3), cam_ts (B, 1, 3) or (B, 3) -> (B, wh, wh) long part ids (renderers/nmr_renderer.py:76-91)."""
        return self.render_arrays(vertices, cam_ts).long()


class WeakPerspectiveSilhouetteRenderer(nn.Module):
    """Predicted silhouette for evaluation: the mesh under the weak-perspective camera [s, tx, ty] the regressor predicts, as a byte mask
    (csrc/eval.hip, straps_wp_silhouette).  mask[b, r, c] = 1 iff the pixel centre ((2c + 1 - wh) / wh, (2r + 1 - wh) / wh) lies inside
    the projection u = s (x + tx), v = s (y + ty) of some face; rows run with +v (no flip), the pixel grid of
    undo_keypoint_normalisation, so the mask lines up with Predictor's `vertices2D`.

        renderer = WeakPerspectiveSilhouetteRenderer(faces, img_wh=256).to(device)
        silhouettes = renderer(out['vertices'], out['cam_wp'])          # uint8 [B, wh, wh]

    faces=None loads config.SMPL_FACES_PATH, as NMRRenderer does."""

    def __init__(self, faces=None, img_wh=256):
        super().__init__()
        if faces is None:
            if not os.path.isfile(config.SMPL_FACES_PATH):
                raise RuntimeError('WeakPerspectiveSilhouetteRenderer: %s not found; pass faces= (e.g. from synthetic_smpl_model())' % config.SMPL_FACES_PATH)
            faces = np.load(config.SMPL_FACES_PATH)
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        faces = np.ascontiguousarray(np.asarray(faces).astype(np.int32))
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
            raise RuntimeError('WeakPerspectiveSilhouetteRenderer: faces must be [F,3] (got %s)' % (faces.shape,))
        if not 1 <= int(img_wh) <= 4096:
            raise RuntimeError('WeakPerspectiveSilhouetteRenderer: img_wh must be in 1..4096 (got %r)' % (img_wh,))
        self.register_buffer('faces', torch.from_numpy(faces))
        self.img_wh = int(img_wh)

    @hipabi.on_tensor_device
    def forward(self, vertices, cam_wp):
        """vertices [B,N,3], cam_wp [B,3] (fp32 GPU) -> uint8 [B,wh,wh], 1 = covered."""
        hipabi.require_gpu_tensor(vertices, 'vertices', torch.float32)
        hipabi.require_gpu_tensor(cam_wp, 'cam_wp', torch.float32)
        hipabi.require_gpu_tensor(self.faces, 'WeakPerspectiveSilhouetteRenderer buffers (call .to(device))', torch.int32)
        if vertices.dim() != 3 or vertices.shape[2] != 3 or tuple(cam_wp.shape) != (vertices.shape[0], 3):
            raise RuntimeError('WeakPerspectiveSilhouetteRenderer: expected vertices [B,N,3] and cam_wp [B,3], got %s and %s'
                               % (tuple(vertices.shape), tuple(cam_wp.shape)))
        B, N, wh = vertices.shape[0], vertices.shape[1], self.img_wh
        vertices, cam_wp = vertices.detach().contiguous(), cam_wp.detach().contiguous()
        L = hipabi.lib()
        out = torch.empty(B, wh, wh, device=vertices.device, dtype=torch.uint8)
        ws = torch.empty(L.straps_wp_silhouette_workspace_bytes(B, N) // 4, device=vertices.device, dtype=torch.float32)
        hipabi.check(L.straps_wp_silhouette(hipabi.ptr(vertices), hipabi.ptr(self.faces), hipabi.ptr(cam_wp), hipabi.ptr(out), hipabi.ptr(ws),
                                            B, N, self.faces.shape[0], wh, hipabi.stream_ptr()), 'straps_wp_silhouette')
        return out


def vertex_face_table(faces, num_vertices):
    """CSR vertex-to-face table of csrc/render.hip's normal kernel: -> (vf_offsets [num_vertices + 1] int32, vf_faces int32).  Vertex v's
    faces are vf_faces[vf_offsets[v]:vf_offsets[v + 1]], ascending; a face that names a vertex twice is listed once for it; a face with an
    index outside [0, num_vertices) is listed nowhere (the rasteriser skips it as well).  Host numpy, built once per mesh."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = ((faces >= 0) & (faces < num_vertices)).all(1)
    fid = np.repeat(np.nonzero(valid)[0], 3)
    pairs = np.unique(faces[valid].reshape(-1) * np.int64(faces.shape[0] + 1) + fid)           # sorted by (vertex, face), duplicates dropped
    vert, face = pairs // (faces.shape[0] + 1), pairs % (faces.shape[0] + 1)
    offsets = np.zeros(num_vertices + 1, np.int64)
    np.cumsum(np.bincount(vert, minlength=num_vertices), out=offsets[1:])
    return offsets.astype(np.int32), np.ascontiguousarray(face.astype(np.int32))


class WeakPerspectiveMeshRenderer(nn.Module):
    """Shaded picture of the mesh under the weak-perspective camera [s, tx, ty] the regressor predicts (csrc/render.hip, straps_render_mesh):
    the batched, on-device counterpart of renderers/weak_perspective_pyrender_renderer.py for predict_3D.py:169-178.

        renderer = WeakPerspectiveMeshRenderer(faces, img_wh=256).to(device)
        rend = renderer(out['vertices'], out['cam_wp'], background=images)         # uint8 [B, wh, wh, 3]

    Geometry is exact and deterministic: the pixel grid and coverage rule of WeakPerspectiveSilhouetteRenderer, the nearest face (smallest z;
    the reference's scene, turned by 180 degrees about x and seen down -z, is this frame seen along +z) per pixel, ties to the lower face id.
    Shading is Lambert with an ambient term, c = colour * min(1, ambient + sum_l intensity_l * max(0, n . d_l)), on interpolated vertex
    normals turned towards the viewer per face -- NOT pyrender's metallic-roughness material: the pictures look like the reference's, their
    pixel values are not the reference's.  `lights` are ((direction from the surface to the light, intensity), ...), at most four,
    normalised here; the defaults are the reference's two lights at (0, -1, 1) and (0, 1, 1) expressed in this frame.  Channel order is the
    caller's: `colour` and the background are passed through as they are.

    faces=None loads config.SMPL_FACES_PATH, as the sibling renderers do.  num_vertices (default: the largest valid index + 1) fixes the
    vertex-to-face table; forward refuses meshes of another size."""

    def __init__(self, faces=None, img_wh=256, colour=(0.8, 0.3, 0.3), ambient=0.3, lights=(((0, 1, -1), 1.0), ((0, -1, -1), 1.0)), background=(0, 0, 0),
                 num_vertices=None):
        super().__init__()
        if faces is None:
            if not os.path.isfile(config.SMPL_FACES_PATH):
                raise RuntimeError('WeakPerspectiveMeshRenderer: %s not found; pass faces= (e.g. from synthetic_smpl_model())' % config.SMPL_FACES_PATH)
            faces = np.load(config.SMPL_FACES_PATH)
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        faces = np.ascontiguousarray(np.asarray(faces).astype(np.int32))
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
            raise RuntimeError('WeakPerspectiveMeshRenderer: faces must be [F,3] (got %s)' % (faces.shape,))
        if not 1 <= int(img_wh) <= 4096:
            raise RuntimeError('WeakPerspectiveMeshRenderer: img_wh must be in 1..4096 (got %r)' % (img_wh,))
        if num_vertices is None:
            num_vertices = int(faces.max()) + 1
        if int(num_vertices) < 1:
            raise RuntimeError('WeakPerspectiveMeshRenderer: num_vertices must be positive (got %r)' % (num_vertices,))
        self.num_vertices, self.img_wh = int(num_vertices), int(img_wh)
        offsets, table = vertex_face_table(faces, self.num_vertices)
        if table.size == 0:
            table = np.zeros(1, np.int32)                     # (never read: every vertex's range is empty; the library wants a pointer)
        self.register_buffer('faces', torch.from_numpy(faces))
        self.register_buffer('vf_offsets', torch.from_numpy(offsets))
        self.register_buffer('vf_faces', torch.from_numpy(table))
        lights = tuple(lights)
        if len(lights) > 4:
            raise RuntimeError('WeakPerspectiveMeshRenderer: at most four lights (got %d)' % len(lights))
        self.colour, self.background, self.ambient = tuple(float(c) for c in colour), tuple(float(c) for c in background), float(ambient)
        if len(self.colour) != 3 or len(self.background) != 3 or not (np.isfinite(self.ambient) and self.ambient >= 0):
            raise RuntimeError('WeakPerspectiveMeshRenderer: colour and background are three numbers each, ambient is finite and not negative')
        self.lights = []
        for d, inten in lights:
            d = np.asarray(d, np.float64).reshape(3)
            length = float(np.linalg.norm(d))
            if not (np.isfinite(length) and length > 0):
                raise RuntimeError('WeakPerspectiveMeshRenderer: a light direction must be a finite non-zero vector (got %r)' % (d.tolist(),))
            self.lights.append((tuple((d / length).tolist()), float(inten)))

    def render_opts(self, colour=None):
        """-> hipabi.RenderOptsStruct of this renderer (colour: a per-call override)"""
        o = hipabi.RenderOptsStruct()
        o.colour[:] = [float(c) for c in (self.colour if colour is None else colour)]
        o.ambient = self.ambient
        o.background[:] = self.background
        o.n_lights = len(self.lights)
        for l, (d, inten) in enumerate(self.lights):
            o.light_dir[3 * l:3 * l + 3] = d
            o.light_intensity[l] = inten
        return o

    @hipabi.on_tensor_device
    def forward(self, vertices, cam_wp, background=None, rotation=None, return_aux=False, colour=None):
        """vertices [B,N,3], cam_wp [B,3] (fp32 GPU); background None or uint8 [B,wh,wh,3] (GPU; made contiguous if it is not); rotation None,
        [3,3] (one for all bodies) or [B,3,3] (fp32 GPU, row-major, applied to the vertices before the camera)
        -> uint8 [B,wh,wh,3], or with return_aux a dict {'rgb', 'mask' uint8 [B,wh,wh], 'depth' float32 [B,wh,wh] (+inf where empty),
        'face_ids' int32 [B,wh,wh] (-1 where empty)}.  Never synchronises; runs on the current stream; capturable."""
        name = 'WeakPerspectiveMeshRenderer'
        hipabi.require_gpu_tensor(vertices, 'vertices', torch.float32)
        hipabi.require_gpu_tensor(cam_wp, 'cam_wp', torch.float32)
        hipabi.require_gpu_tensor(self.faces, name + ' buffers (call .to(device))', torch.int32)
        if vertices.dim() != 3 or vertices.shape[2] != 3 or tuple(cam_wp.shape) != (vertices.shape[0], 3):
            raise RuntimeError('%s: expected vertices [B,N,3] and cam_wp [B,3], got %s and %s' % (name, tuple(vertices.shape), tuple(cam_wp.shape)))
        B, N, wh = vertices.shape[0], vertices.shape[1], self.img_wh
        if N != self.num_vertices:
            raise RuntimeError('%s: the vertex-to-face table was built for %d vertices, got %d (pass num_vertices=)' % (name, self.num_vertices, N))
        vertices, cam_wp = vertices.detach().contiguous(), cam_wp.detach().contiguous()
        if background is not None:
            hipabi.require_gpu_tensor(background, 'background', torch.uint8)
            if tuple(background.shape) != (B, wh, wh, 3):
                raise RuntimeError('%s: background must be uint8 [%d,%d,%d,3], got %s' % (name, B, wh, wh, tuple(background.shape)))
            background = background.contiguous()
        per_body = 0
        if rotation is not None:
            hipabi.require_gpu_tensor(rotation, 'rotation', torch.float32)
            if tuple(rotation.shape) not in ((3, 3), (B, 3, 3)):
                raise RuntimeError('%s: rotation must be [3,3] or [%d,3,3], got %s' % (name, B, tuple(rotation.shape)))
            per_body = 1 if rotation.dim() == 3 else 0
            rotation = rotation.detach().contiguous()
        L = hipabi.lib()
        dev = vertices.device
        rgb = torch.empty(B, wh, wh, 3, device=dev, dtype=torch.uint8)
        mask = torch.empty(B, wh, wh, device=dev, dtype=torch.uint8) if return_aux else None
        depth = torch.empty(B, wh, wh, device=dev, dtype=torch.float32) if return_aux else None
        face_ids = torch.empty(B, wh, wh, device=dev, dtype=torch.int32) if return_aux else None
        ws = torch.empty(L.straps_render_mesh_workspace_bytes(B, N, wh) // 8, device=dev, dtype=torch.float64)
        opts = self.render_opts(colour)
        hipabi.check(L.straps_render_mesh(hipabi.ptr(vertices), hipabi.ptr(self.faces), hipabi.ptr(self.vf_offsets), hipabi.ptr(self.vf_faces),
                                          hipabi.ptr(cam_wp), 3, hipabi.ptr(rotation), per_body, C.byref(opts), hipabi.ptr(background), hipabi.ptr(rgb),
                                          hipabi.ptr(mask), hipabi.ptr(depth), hipabi.ptr(face_ids), hipabi.ptr(ws), B, N, self.faces.shape[0], wh,
                                          hipabi.stream_ptr()), 'straps_render_mesh')
        return {'rgb': rgb, 'mask': mask, 'depth': depth, 'face_ids': face_ids} if return_aux else rgb
