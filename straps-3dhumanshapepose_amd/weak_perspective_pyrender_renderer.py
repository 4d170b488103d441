"""Drop-in for the reference's renderers/weak_perspective_pyrender_renderer.py (class Renderer): numpy in, numpy out, one body per call.

    renderer = Renderer(resolution=(256, 256))
    rend_img = renderer.render(verts=pred_vertices, cam=pred_cam_wp, img=image)
    reposed = renderer.render(verts=pred_reposed_vertices, cam=np.array([0.8, 0., -0.2]), angle=180, axis=[1, 0, 0])

The reference draws with pyrender, trimesh and OpenGL; here the picture comes from nmr_renderer.WeakPerspectiveMeshRenderer (csrc/render.hip) on
the GPU.  Same geometry: the reference turns the mesh by 180 degrees about x and looks down -z through its weak-perspective projection, which is
this package's frame seen along +z on the pixel grid of undo_keypoint_normalisation.  Its optional rotation comes AFTER that turn, so the rotation
handed down is Rx(180) R(angle, axis) Rx(180).  NOT the same shading: Lambert with an ambient term instead of pyrender's metallic-roughness
material, so the pixel values differ from the reference's.  Channel order is the caller's (the reference hands `color` to cv2 as BGR).
For batches use WeakPerspectiveMeshRenderer or Predictor.render directly: this class copies to and from the host on every call.
"""
import math

import numpy as np
import torch

from . import config  # noqa: F401  (faces=None reads config.SMPL_FACES_PATH through the module below)
from .nmr_renderer import WeakPerspectiveMeshRenderer

_RX180 = np.diag([1.0, -1.0, -1.0])


def rotation_matrix(angle_degrees, axis):
    """[3,3] float64 rotation by `angle_degrees` about `axis` (Rodrigues), what trimesh.transformations.rotation_matrix gives for a direction"""
    ax = np.asarray(axis, np.float64).reshape(3)
    n = float(np.linalg.norm(ax))
    if not n > 0:
        raise ValueError('Renderer.render: axis must be a non-zero vector (got %r)' % (axis,))
    ax = ax / n
    a = math.radians(float(angle_degrees))
    K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    return np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * K.dot(K)


def write_obj(path, verts, faces):
    """a plain Wavefront OBJ: `v x y z` lines, then `f i j k` (1-based)"""
    with open(path, 'w') as fh:
        for v in np.asarray(verts, np.float64):
            fh.write('v %.8f %.8f %.8f\n' % (v[0], v[1], v[2]))
        for f in np.asarray(faces, np.int64):
            fh.write('f %d %d %d\n' % (f[0] + 1, f[1] + 1, f[2] + 1))


class Renderer():
    def __init__(self, resolution=(256, 256), faces=None, device='cuda'):
        self.resolution = tuple(int(r) for r in resolution)
        if len(self.resolution) != 2 or self.resolution[0] != self.resolution[1]:
            raise ValueError('Renderer: only square pictures are built (got resolution %r)' % (resolution,))
        self.device = torch.device(device)
        self.module = WeakPerspectiveMeshRenderer(faces, img_wh=self.resolution[0]).to(self.device)
        self.faces = self.module.faces.cpu().numpy()

    def render(self, verts, cam, img=None, angle=None, axis=None, mesh_filename=None, color=[0.8, 0.3, 0.3], return_mask=False):
        """verts [N,3], cam [3] = (s, tx, ty) or [4] = (sx, sy, tx, ty) with sx == sy, img None or [wh,wh,3] (drawn over; values taken to uint8),
        angle (degrees) and axis: an optional rotation after the reference's own 180-degree turn; mesh_filename: a .obj path that receives the
        turned mesh as the reference exports it -> uint8 [wh,wh,3], or with return_mask the bool [wh,wh] coverage."""
        verts = np.ascontiguousarray(np.asarray(verts, np.float32))
        if verts.ndim != 2 or verts.shape[1] != 3:
            raise ValueError('Renderer.render: verts must be [N,3] (got %s)' % (verts.shape,))
        cam = np.asarray(cam, np.float32).reshape(-1)
        if cam.shape[0] == 4:
            if cam[0] != cam[1]:
                raise ValueError('Renderer.render: a camera (sx, sy, tx, ty) with sx != sy (%r, %r) is not built: the weak-perspective camera here has '
                                 'one scale' % (float(cam[0]), float(cam[1])))
            cam = cam[1:]
        elif cam.shape[0] != 3:
            raise ValueError('Renderer.render: cam must have 3 or 4 entries (got %d)' % cam.shape[0])
        if mesh_filename is not None:
            if not str(mesh_filename).lower().endswith('.obj'):
                raise ValueError('Renderer.render: only .obj meshes are written (got %r)' % (mesh_filename,))
            write_obj(mesh_filename, verts.astype(np.float64).dot(_RX180.T), self.faces)
        wh = self.resolution[0]
        rotation = None
        if angle and axis is not None and np.any(np.asarray(axis)):
            rotation = torch.from_numpy(_RX180.dot(rotation_matrix(angle, axis)).dot(_RX180).astype(np.float32)).to(self.device)
        background = None
        if img is not None and not return_mask:
            img = np.asarray(img)
            if img.shape != (wh, wh, 3):
                raise ValueError('Renderer.render: img must be [%d,%d,3] (got %s)' % (wh, wh, img.shape))
            background = torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8)))[None].to(self.device)
        with torch.no_grad():
            out = self.module(torch.from_numpy(verts)[None].to(self.device), torch.from_numpy(np.ascontiguousarray(cam))[None].to(self.device),
                              background=background, rotation=rotation, return_aux=return_mask, colour=color)
        if return_mask:
            return out['mask'][0].cpu().numpy().astype(bool)
        return out[0].cpu().numpy()
