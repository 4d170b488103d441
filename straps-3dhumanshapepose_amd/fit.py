"""Test-time fitting of the regressor's answer to the 2-D keypoints it was given (straps_fit_keypoints, csrc/fit.hip).

The reference's predict path (predict/predict_3D.py:116-149) stops at the regressor; what it returns does not reproject onto the
keypoints.  `KeypointFitter` runs a fixed number of Adam steps on (cam, 6-D pose, shape) against the reprojection error of the
keypoints, with quadratic priors that hold pose and shape near the regressor's answer, as ONE kernel launch: one wave per body, all
iterations inside the kernel.  Only the 24 kinematic joints and up to 16 tracked mesh vertices take part, so no mesh is built; the 45
regressed joints (rows 45..89 of the 90-joint output) need the mesh and are refused.

The defaults (100 iterations, lr 0.01, lambda 1e-3) are the values of a float64 experiment on the synthetic model of this package: nobody
has tuned them on real detections, and neither a real SMPL model nor detector output was available when they were chosen.

`SilhouetteFitter` adds the silhouette the regressor was given to that objective (straps_distance_field, straps_silhouette_energy,
straps_fit_adam: csrc/silfit.hip): the projected vertices are pulled inside the target mask through its distance field, the mask's
foreground pixels pull their nearest projected vertex towards them.  That term needs the whole mesh, so its loop is a sequence of entry
points per iteration (SMPL forward and backward included), not one launch.  Its default weights (100 on both silhouette terms, lattice 4,
tau 1.5 px) are those of a float64 prototype on the synthetic model as well: untuned on real detections.

`SubjectFitter` is that loop for several frames of one person: cam and pose per frame, ONE shape per subject (straps_fit_adam_subjects and
straps_subject_mean_rows, csrc/fit_subjects.hip, in the place of straps_fit_adam).

`ScanFitter` takes a 3-D scan of the person as its target instead of images: the same loop with straps_scan_energy (csrc/scanfit.hip), the
two-sided nearest-point distance between the posed vertices and the scan's points, in the place of the silhouette term, and a translation
in metres in the place of the camera.  Its defaults (weights 100 and 100, sigma 0, lr 0.01) are a float64 prototype's on the synthetic
model as well: untuned on real scans.
"""
import ctypes as C

import numpy as np
import torch

from . import cam_utils, config, hipabi
from .rigid_transform_utils import rot6d_to_rotmat

NE, KP, MAX_KP, MAX_VERTS = 157, 224, 32, 16


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def pack_fit_model(smpl_or_model_dict, keypoints=None):
    """-> dict of the tables of straps_fit_model_t: 'j_template' [24,3], 'j_shapedirs' [24,3,10], 'parents' [24] int32, 'vert_dirs'
    [n_verts,3,224], 'vert_w' [n_verts,24], 'kp_src' [n_kp] int32, 'vertex_ids' [n_verts] (mesh ids of the tracked vertices, in order of
    first appearance), 'n_verts', 'n_kp'.

    keypoints (default config.ALL_JOINTS_TO_COCO_MAP): rows of the 90-joint output -- 0..23 kinematic joints, 24..44 the picked vertices
    (`extra_vertex_ids`) -- or ('vertex', id) for any mesh vertex.  Rows 45..89 are regressed from the whole mesh: ValueError, as are more
    than 32 keypoints or more than 16 distinct vertices.
    For an SMPL module the rest-joint tables are the module's own buffers (the forward kernel's rest joints, on its device); for a model
    dict they are computed as pack_smpl_model computes them.  Everything else is numpy."""
    keypoints = list(config.ALL_JOINTS_TO_COCO_MAP if keypoints is None else keypoints)
    is_module = isinstance(smpl_or_model_dict, torch.nn.Module)
    if is_module:
        s = smpl_or_model_dict
        vt, sd, pd, W = _np(s.v_template), _np(s.shapedirs), _np(s.posedirs), _np(s.lbs_weights)
        pick = _np(s._k_pick_ids)
        jt, js, parents = s._k_j_template, s._k_j_shapedirs, s._k_parents
    else:
        m = smpl_or_model_dict
        vt, sd, pd, W = (np.asarray(m[k], np.float32) for k in ('v_template', 'shapedirs', 'posedirs', 'weights'))
        pick = np.asarray(m['extra_vertex_ids'], np.int64)
        Jr = np.asarray(m['J_regressor'], np.float64)
        jt = (Jr @ np.asarray(m['v_template'], np.float64)).astype(np.float32)                      # (as pack_smpl_model)
        js = np.einsum('jv,vcl->jcl', Jr, np.asarray(m['shapedirs'], np.float64)).astype(np.float32)
        parents = np.asarray(m['parents'], np.int32).copy()
    nv_mesh = vt.shape[0]
    if not 1 <= len(keypoints) <= MAX_KP:
        raise ValueError('pack_fit_model: between 1 and %d keypoints (got %d)' % (MAX_KP, len(keypoints)))
    vids, kp_src = [], []
    for k in keypoints:
        if isinstance(k, (tuple, list)):
            if len(k) != 2 or k[0] != 'vertex' or not 0 <= int(k[1]) < nv_mesh:
                raise ValueError("pack_fit_model: a keypoint is a row of the 90-joint output or ('vertex', id) with id in 0..%d (got %r)" % (nv_mesh - 1, k))
            v = int(k[1])
        else:
            k = int(k)
            if 0 <= k < 24:
                kp_src.append(k)
                continue
            if not 24 <= k < 24 + len(pick):
                raise ValueError('pack_fit_model: keypoint row %d is a joint regressed from the whole mesh (rows %d..89): it needs the mesh, '
                                 'only rows 0..%d can be fitted' % (k, 24 + len(pick), 23 + len(pick)))
            v = int(pick[k - 24])
        if v not in vids:
            vids.append(v)
        kp_src.append(24 + vids.index(v))
    if len(vids) > MAX_VERTS:
        raise ValueError('pack_fit_model: at most %d distinct mesh vertices (got %d)' % (MAX_VERTS, len(vids)))
    n = len(vids)
    D = np.zeros((n, 3, KP), np.float32)
    Wd = np.zeros((n, 24), np.float32)
    pdv = pd.reshape(207, nv_mesh, 3)
    for i, v in enumerate(vids):
        D[i, :, 0] = vt[v]
        D[i, :, 1:11] = sd[v]
        D[i, :, 11:218] = pdv[:, v, :].T
        Wd[i] = W[v]
    return {'j_template': jt, 'j_shapedirs': js, 'parents': parents, 'vert_dirs': D, 'vert_w': Wd, 'kp_src': np.asarray(kp_src, np.int32),
            'vertex_ids': np.asarray(vids, np.int64), 'n_verts': n, 'n_kp': len(kp_src)}


def fit_keypoints_raw(model_struct, opts, est, est0, targets, conf, exp_avg, exp_avg_sq, energy, grad, best_est, best_energy, kp2d):
    """one straps_fit_keypoints call on contiguous fp32 GPU tensors (None -> NULL); est [B,157] is updated in place"""
    hipabi.check(hipabi.lib().straps_fit_keypoints(C.byref(model_struct), C.byref(opts), hipabi.ptr(est), hipabi.ptr(est0), hipabi.ptr(targets), hipabi.ptr(conf),
                                                   hipabi.ptr(exp_avg), hipabi.ptr(exp_avg_sq), hipabi.ptr(energy), hipabi.ptr(grad), hipabi.ptr(best_est),
                                                   hipabi.ptr(best_energy), hipabi.ptr(kp2d), est.shape[0], hipabi.stream_ptr()), 'straps_fit_keypoints')


class KeypointFitter:
    """`KeypointFitter(smpl)(cam, pose6d, shape, joints2D)` -> dict of device tensors; see the module docstring for what is minimised and
    include/straps_hip.h for the exact objective.  smpl: the SMPL module (its device holds the tables).  lr: a float or a (cam, pose,
    shape) triple.  The defaults are untuned on real data (module docstring)."""

    def __init__(self, smpl, keypoints=None, iters=100, lr=0.01, robust_sigma=0.0, lambda_pose=1e-3, lambda_shape=1e-3,
                 img_wh=config.REGRESSOR_IMG_WH, betas=(0.9, 0.999), eps=1e-8):
        packed = pack_fit_model(smpl, keypoints)
        hipabi.require_gpu_tensor(smpl._k_j_template, 'SMPL model buffers (call .to(device))')
        dev = smpl._k_j_template.device
        self.device, self.n_kp, self.n_verts = dev, packed['n_kp'], packed['n_verts']
        self.vertex_ids = packed['vertex_ids']
        self._tables = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(dev))
                        for k, v in packed.items() if k in ('j_template', 'j_shapedirs', 'parents', 'vert_dirs', 'vert_w', 'kp_src')}
        s = hipabi.FitModelStruct()
        for k, t in self._tables.items():
            setattr(s, k, t.data_ptr() if t.numel() else None)
        s.n_verts, s.n_kp = self.n_verts, self.n_kp
        self._struct = s
        lrs = tuple(float(v) for v in lr) if isinstance(lr, (tuple, list)) else (float(lr),) * 3
        if len(lrs) != 3:
            raise ValueError('KeypointFitter: lr is a float or a (cam, pose, shape) triple')
        self.iters, self.lr, self.robust_sigma = int(iters), lrs, float(robust_sigma)
        self.lambda_pose, self.lambda_shape, self.img_wh = float(lambda_pose), float(lambda_shape), float(img_wh)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)

    def opts(self, iters=None, step0=0):
        return hipabi.FitOptsStruct(self.iters if iters is None else int(iters), int(step0), self.lr[0], self.lr[1], self.lr[2], self.betas[0], self.betas[1],
                                    self.eps, self.robust_sigma, self.lambda_pose, self.lambda_shape, self.img_wh)

    def _inputs(self, cam, pose6d, shape, joints2D, conf, prior):
        for t, nm, w in ((cam, 'cam', 3), (pose6d, 'pose6d', 144), (shape, 'shape', 10)):
            hipabi.require_gpu_tensor(t, nm, torch.float32)
            if t.dim() != 2 or t.shape[1] != w or t.shape[0] != cam.shape[0]:
                raise RuntimeError('KeypointFitter: %s must be [B,%d], got %s' % (nm, w, tuple(t.shape)))
        B = cam.shape[0]
        hipabi.require_gpu_tensor(joints2D, 'joints2D')
        if joints2D.dim() != 3 or joints2D.shape[0] != B or joints2D.shape[1] != self.n_kp or joints2D.shape[2] not in (2, 3):
            raise RuntimeError('KeypointFitter: joints2D must be [%d,%d,2] or [%d,%d,3], got %s' % (B, self.n_kp, B, self.n_kp, tuple(joints2D.shape)))
        est = torch.cat([cam.detach(), pose6d.detach(), shape.detach()], dim=1)
        j = joints2D.detach().float()
        if conf is None and j.shape[2] == 3:
            conf = j[:, :, 2]
        targets = j[:, :, :2].contiguous()
        if conf is not None:
            hipabi.require_gpu_tensor(conf, 'conf')
            if tuple(conf.shape) != (B, self.n_kp):
                raise RuntimeError('KeypointFitter: conf must be [%d,%d], got %s' % (B, self.n_kp, tuple(conf.shape)))
            conf = conf.detach().float().contiguous()
        est0 = None
        if prior is not None:
            for p in (prior if isinstance(prior, (tuple, list)) else (prior,)):
                hipabi.require_gpu_tensor(p, 'prior', torch.float32)
            est0 = (torch.cat([p.detach() for p in prior], dim=1) if isinstance(prior, (tuple, list)) else prior.detach()).contiguous()
            if tuple(est0.shape) != (B, NE):
                raise RuntimeError('KeypointFitter: prior must be [B,157] or a (cam, pose6d, shape) triple, got %s' % (tuple(est0.shape),))
        return est, est0, targets, conf

    @hipabi.on_tensor_device
    def evaluate(self, cam, pose6d, shape, joints2D, conf=None, prior=None):
        """-> (energy [B], grad [B,157], kp2d [B,K,2] normalised): the objective, its gradient and the projection at the given parameters"""
        est, est0, targets, conf = self._inputs(cam, pose6d, shape, joints2D, conf, prior)
        B = est.shape[0]
        energy = torch.empty(B, 1, device=est.device, dtype=torch.float32)
        grad = torch.empty(B, NE, device=est.device, dtype=torch.float32)
        kp2d = torch.empty(B, self.n_kp, 2, device=est.device, dtype=torch.float32)
        fit_keypoints_raw(self._struct, self.opts(0), est, est0, targets, conf, None, None, energy, grad, None, None, kp2d)
        return energy[:, 0], grad, kp2d

    @hipabi.on_tensor_device
    def __call__(self, cam, pose6d, shape, joints2D, conf=None, prior=None, state=None, trace=False):
        """cam [B,3], pose6d [B,144], shape [B,10], joints2D [B,K,2] or [B,K,3] in pixels of an img_wh square (a third column is the
        confidence when `conf` is None), conf [B,K] or None, prior: the centre of the pose / shape priors ([B,157] or a triple; None = the
        start), state: the 'state' of an earlier call (the Adam moments and step count go on from there).
        -> {'cam_wp' [B,3], 'pose' [B,144], 'shape' [B,10], 'pose_rotmats' [B,24,3,3], 'energy0' [B], 'energy' [B] (at the returned
        parameters), 'best': {'cam_wp', 'pose', 'shape', 'energy'} (the iterate of the smallest energy), 'joints2D' [B,K,2] (the fitted
        projection, pixels), 'state', 'trace' [B,iters+1] if asked}.  The inputs are not modified.  Never synchronises; after one warm-up
        call at the same shapes it can be captured in torch.cuda.graph."""
        est, est0, targets, conf = self._inputs(cam, pose6d, shape, joints2D, conf, prior)
        B, dev = est.shape[0], est.device
        if state is None:
            m, v, step0 = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev), 0
        else:
            for k in ('exp_avg', 'exp_avg_sq'):
                hipabi.require_gpu_tensor(state[k], "state['%s']" % k, torch.float32)
                if tuple(state[k].shape) != (B, NE):
                    raise RuntimeError("KeypointFitter: state['%s'] must be [%d,157], got %s" % (k, B, tuple(state[k].shape)))
            # (contiguous copies: the call updates them in place, the caller's state stays as it was)
            m, v = (state[k].detach().clone(memory_format=torch.contiguous_format) for k in ('exp_avg', 'exp_avg_sq'))
            step0 = int(state['step'])
        energy = torch.empty(B, self.iters + 1, device=dev, dtype=torch.float32)
        best = torch.empty(B, NE, device=dev, dtype=torch.float32)
        best_e = torch.empty(B, device=dev, dtype=torch.float32)
        kp2d = torch.empty(B, self.n_kp, 2, device=dev, dtype=torch.float32)
        fit_keypoints_raw(self._struct, self.opts(step0=step0), est, est0, targets, conf, m, v, energy, None, best, best_e, kp2d)
        pose = est[:, 3:147]
        out = {'cam_wp': est[:, :3], 'pose': pose, 'shape': est[:, 147:], 'pose_rotmats': rot6d_to_rotmat(pose).view(B, 24, 3, 3),
               'energy0': energy[:, 0], 'energy': energy[:, self.iters],
               'best': {'cam_wp': best[:, :3], 'pose': best[:, 3:147], 'shape': best[:, 147:], 'energy': best_e},
               'joints2D': cam_utils.undo_keypoint_normalisation(kp2d, self.img_wh),
               'state': {'exp_avg': m, 'exp_avg_sq': v, 'step': step0 + self.iters}}
        if trace:
            out['trace'] = energy
        return out


def distance_field(masks):
    """masks [B,wh,wh] (uint8, bool or float GPU tensor; compared with 0) -> int32 [B,wh,wh]: the exact squared Euclidean distance of every
    pixel to the nearest foreground pixel of its frame, 2 * wh * wh in a frame without foreground (straps_distance_field)."""
    hipabi.require_gpu_tensor(masks, 'masks')
    if masks.dim() != 3 or masks.shape[1] != masks.shape[2] or masks.shape[0] < 1:
        raise RuntimeError('distance_field: masks must be [B,wh,wh], got %s' % (tuple(masks.shape),))
    m = masks.detach()
    m = m.contiguous() if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)
    d2 = torch.empty(m.shape, device=m.device, dtype=torch.int32)
    hipabi.check(hipabi.lib().straps_distance_field(hipabi.ptr(m), hipabi.ptr(d2), m.shape[0], m.shape[1], hipabi.stream_ptr()), 'straps_distance_field')
    return d2


def silhouette_energy_raw(verts, cam, ld_cam, mask, d2, opts, energy2, dverts, dcam, nearest, workspace):
    """one straps_silhouette_energy call on contiguous GPU tensors (None -> NULL); cam: a tensor or a raw device address"""
    camp = C.c_void_p(cam) if isinstance(cam, int) else hipabi.ptr(cam)
    hipabi.check(hipabi.lib().straps_silhouette_energy(hipabi.ptr(verts), camp, ld_cam, hipabi.ptr(mask), hipabi.ptr(d2), C.byref(opts), hipabi.ptr(energy2),
                                                       hipabi.ptr(dverts), hipabi.ptr(dcam), hipabi.ptr(nearest), hipabi.ptr(workspace), verts.shape[0],
                                                       verts.shape[1], hipabi.stream_ptr()), 'straps_silhouette_energy')


def fit_adam_raw(opts, est, g_kp, dcam, dx6, dbetas, e_kp, energy2, w_in, w_out, exp_avg, exp_avg_sq, energy, col, grad, best_est, best_energy,
                 step, first, update):
    """one straps_fit_adam call on contiguous fp32 GPU tensors (None -> NULL); energy [B,ld] receives column `col`"""
    hipabi.check(hipabi.lib().straps_fit_adam(C.byref(opts), hipabi.ptr(est), hipabi.ptr(g_kp), hipabi.ptr(dcam), hipabi.ptr(dx6), hipabi.ptr(dbetas), hipabi.ptr(e_kp),
                                              hipabi.ptr(energy2), w_in, w_out, hipabi.ptr(exp_avg), hipabi.ptr(exp_avg_sq), hipabi.ptr(energy),
                                              0 if energy is None else energy.shape[1], col, hipabi.ptr(grad), hipabi.ptr(best_est), hipabi.ptr(best_energy),
                                              int(step), int(bool(first)), int(bool(update)), est.shape[0], hipabi.stream_ptr()), 'straps_fit_adam')


class SilhouetteFitter(KeypointFitter):
    """`SilhouetteFitter(smpl)(cam, pose6d, shape, silhouettes, joints2D)`: KeypointFitter's objective plus w_in E_in + w_out E_out of
    straps_silhouette_energy (include/straps_hip.h) against the target masks, minimised by the same Adam.  lattice: spacing in pixels of the
    target's foreground samples; tau: the distance in pixels below which a sample counts as covered.  joints2D=None fits the silhouette
    and the priors alone.  The defaults are a float64 prototype's on the synthetic model, untuned on real detections (module docstring)."""

    def __init__(self, smpl, keypoints=None, iters=100, lr=0.01, lattice=4, tau=1.5, w_in=100., w_out=100., robust_sigma=0.0, lambda_pose=1e-3,
                 lambda_shape=1e-3, img_wh=config.REGRESSOR_IMG_WH, betas=(0.9, 0.999), eps=1e-8):
        KeypointFitter.__init__(self, smpl, keypoints, iters, lr, robust_sigma, lambda_pose, lambda_shape, img_wh, betas, eps)
        self.smpl = smpl
        self.wh = int(img_wh)
        if self.wh != img_wh or not 2 <= self.wh <= 1024:
            raise ValueError('SilhouetteFitter: img_wh must be an integer in 2..1024 (got %r)' % (img_wh,))
        if int(lattice) < 1 or not float(tau) >= 0:
            raise ValueError('SilhouetteFitter: lattice must be at least 1 and tau must not be negative')
        self.lattice, self.tau, self.w_in, self.w_out = int(lattice), float(tau), float(w_in), float(w_out)

    def sil_opts(self):
        return hipabi.SilFitOptsStruct(self.wh, self.lattice, self.tau, self.w_in, self.w_out)

    def _sil_inputs(self, cam, pose6d, shape, silhouettes, joints2D, conf, prior):
        hipabi.require_gpu_tensor(cam, 'cam', torch.float32)
        B = cam.shape[0]
        hipabi.require_gpu_tensor(silhouettes, 'silhouettes')
        if tuple(silhouettes.shape) != (B, self.wh, self.wh):
            raise RuntimeError('SilhouetteFitter: silhouettes must be [%d,%d,%d], got %s' % (B, self.wh, self.wh, tuple(silhouettes.shape)))
        if joints2D is None:      # no keypoints: all confidences zero, the keypoint kernel supplies the priors alone
            if conf is not None:
                raise RuntimeError('SilhouetteFitter: conf without joints2D')
            joints2D = torch.zeros(B, self.n_kp, 2, device=cam.device, dtype=torch.float32)
            conf = torch.zeros(B, self.n_kp, device=cam.device, dtype=torch.float32)
        est, est0, targets, conf = self._inputs(cam, pose6d, shape, joints2D, conf, prior)
        if est0 is None:
            est0 = est.clone()      # (the start: est itself moves)
        s = silhouettes.detach()
        mask = s.contiguous() if s.dtype == torch.uint8 else (s != 0).to(torch.uint8)
        return est, est0, targets, conf, mask

    def _buffers(self, B, dev, mask):
        L = hipabi.lib()
        f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        return {'d2': distance_field(mask), 'R': f(B, 24, 3, 3), 'betas': f(B, 10), 'verts': f(B, self.smpl.v_template.shape[0], 3),
                'dverts': f(B, self.smpl.v_template.shape[0], 3), 'dcam': f(B, 3), 'energy2': f(B, 2), 'drot': f(B, 24, 3, 3), 'dbetas': f(B, 10),
                'dx6': f(B, 144), 'e_kp': f(B, 1), 'g_kp': f(B, NE), 'est_kp': f(B, NE), 'kp2d': f(B, self.n_kp, 2),
                'ws': torch.empty(L.straps_silhouette_energy_workspace_bytes(B, self.smpl.v_template.shape[0], self.wh, self.lattice) // 8, device=dev, dtype=torch.float64),
                'ws_bwd': f(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)}

    def _terms(self, est, est0, targets, conf, mask, buf):
        """the six evaluating entry points of one iteration at `est` (steps 1 to 6 of the loop); the results are left in `buf`"""
        L, st, B = hipabi.lib(), hipabi.stream_ptr(), est.shape[0]
        x6 = C.c_void_p(est.data_ptr() + 12)
        hipabi.check(L.straps_rot6d_fwd(x6, NE, 24, hipabi.ptr(buf['R']), B, st), 'straps_rot6d_fwd')
        buf['betas'].copy_(est[:, 147:])
        self.smpl.forward_arrays(buf['betas'], buf['R'], want_joints=False, out_verts=buf['verts'])
        silhouette_energy_raw(buf['verts'], est, NE, mask, buf['d2'], self.sil_opts(), buf['energy2'], buf['dverts'], buf['dcam'], None, buf['ws'])
        hipabi.check(L.straps_smpl_bwd(C.byref(self.smpl._model_struct()), hipabi.ptr(buf['betas']), hipabi.ptr(buf['R']), hipabi.ptr(buf['dverts']), None,
                                       hipabi.ptr(buf['dbetas']), hipabi.ptr(buf['drot']), hipabi.ptr(buf['ws_bwd']), B, 0, st), 'straps_smpl_bwd')
        hipabi.check(L.straps_rot6d_bwd(x6, NE, 24, hipabi.ptr(buf['drot']), hipabi.ptr(buf['dx6']), 144, B, st), 'straps_rot6d_bwd')
        buf['est_kp'].copy_(est)      # (iters = 0 leaves it as it is; a copy keeps the loop's estimate out of the keypoint kernel's hands)
        fit_keypoints_raw(self._struct, self.opts(0), buf['est_kp'], est0, targets, conf, None, None, buf['e_kp'], buf['g_kp'], None, None, buf['kp2d'])

    @hipabi.on_tensor_device
    def evaluate(self, cam, pose6d, shape, silhouettes, joints2D=None, conf=None, prior=None):
        """-> (energy [B], grad [B,157], terms [B,3] = (E_kp including the priors, E_in, E_out; the silhouette terms unweighted)) at the given
        parameters"""
        est, est0, targets, conf, mask = self._sil_inputs(cam, pose6d, shape, silhouettes, joints2D, conf, prior)
        B, dev = est.shape[0], est.device
        buf = self._buffers(B, dev, mask)
        self._terms(est, est0, targets, conf, mask, buf)
        energy = torch.empty(B, 1, device=dev, dtype=torch.float32)
        grad = torch.empty(B, NE, device=dev, dtype=torch.float32)
        fit_adam_raw(self.opts(), est, buf['g_kp'], buf['dcam'], buf['dx6'], buf['dbetas'], buf['e_kp'], buf['energy2'], self.w_in, self.w_out, None, None,
                     energy, 0, grad, None, None, 0, True, False)
        return energy[:, 0], grad, torch.cat([buf['e_kp'], buf['energy2']], dim=1)

    @hipabi.on_tensor_device
    def __call__(self, cam, pose6d, shape, silhouettes, joints2D=None, conf=None, prior=None, state=None, trace=False):
        """KeypointFitter.__call__ with the target masks `silhouettes` [B,img_wh,img_wh] (uint8, bool or float: compared with 0) as fourth
        argument and joints2D optional.  -> the keys of KeypointFitter.__call__ plus 'energy_terms'
        [B,3] = (E_kp including the priors, E_in, E_out) at the returned parameters.  iters + 1 evaluations, iters updates; every iteration
        is rot6d forward, SMPL forward, straps_silhouette_energy, SMPL backward, rot6d backward, straps_fit_keypoints with iters = 0,
        straps_fit_adam, on buffers allocated before the loop.  The inputs are not modified.  Never synchronises; after one warm-up call at
        the same shapes it can be captured in torch.cuda.graph."""
        est, est0, targets, conf, mask = self._sil_inputs(cam, pose6d, shape, silhouettes, joints2D, conf, prior)
        B, dev = est.shape[0], est.device
        if state is None:
            m, v, step0 = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev), 0
        else:
            for k in ('exp_avg', 'exp_avg_sq'):
                hipabi.require_gpu_tensor(state[k], "state['%s']" % k, torch.float32)
                if tuple(state[k].shape) != (B, NE):
                    raise RuntimeError("SilhouetteFitter: state['%s'] must be [%d,157], got %s" % (k, B, tuple(state[k].shape)))
            m, v = (state[k].detach().clone(memory_format=torch.contiguous_format) for k in ('exp_avg', 'exp_avg_sq'))
            step0 = int(state['step'])
        buf = self._buffers(B, dev, mask)
        energy = torch.empty(B, self.iters + 1, device=dev, dtype=torch.float32)
        best = torch.empty(B, NE, device=dev, dtype=torch.float32)
        best_e = torch.empty(B, device=dev, dtype=torch.float32)
        opts = self.opts()
        for i in range(self.iters + 1):
            self._terms(est, est0, targets, conf, mask, buf)
            fit_adam_raw(opts, est, buf['g_kp'], buf['dcam'], buf['dx6'], buf['dbetas'], buf['e_kp'], buf['energy2'], self.w_in, self.w_out, m, v,
                         energy, i, None, best, best_e, step0 + i, i == 0, i < self.iters)
        pose = est[:, 3:147]
        out = {'cam_wp': est[:, :3], 'pose': pose, 'shape': est[:, 147:], 'pose_rotmats': buf['R'],
               'energy0': energy[:, 0], 'energy': energy[:, self.iters],
               'best': {'cam_wp': best[:, :3], 'pose': best[:, 3:147], 'shape': best[:, 147:], 'energy': best_e},
               'energy_terms': torch.cat([buf['e_kp'], buf['energy2']], dim=1),
               'joints2D': cam_utils.undo_keypoint_normalisation(buf['kp2d'], self.img_wh),
               'state': {'exp_avg': m, 'exp_avg_sq': v, 'step': step0 + self.iters}}
        if trace:
            out['trace'] = energy
        return out


def scan_energy_raw(verts, trans, ld_trans, points, opts, energy2, dverts, dtrans, nearest_vertex, nearest_point, workspace):
    """one straps_scan_energy call on contiguous GPU tensors (None -> NULL); trans: a tensor or a raw device address"""
    tp = C.c_void_p(trans) if isinstance(trans, int) else hipabi.ptr(trans)
    hipabi.check(hipabi.lib().straps_scan_energy(hipabi.ptr(verts), tp, ld_trans, hipabi.ptr(points), C.byref(opts), hipabi.ptr(energy2), hipabi.ptr(dverts),
                                                 hipabi.ptr(dtrans), hipabi.ptr(nearest_vertex), hipabi.ptr(nearest_point), hipabi.ptr(workspace), verts.shape[0],
                                                 verts.shape[1], points.shape[1], hipabi.stream_ptr()), 'straps_scan_energy')


class ScanFitter(KeypointFitter):
    """`ScanFitter(smpl)(transl, pose6d, shape, points)`: registers the body to a 3-D scan.  Minimises w_s2m E_s2m + w_m2s E_m2s of
    straps_scan_energy (include/straps_hip.h: every point pulls its nearest vertex, every vertex is pulled to its nearest point) plus
    KeypointFitter's pose and shape priors, by the same Adam.  In this mode the first three columns of a body's row hold the translation t
    in metres, where the image fitters keep (s, tx, ty); lr[0] is its learning rate.  points [B,P,3]: a point with a NaN or an infinite
    coordinate does not count, which is how scans of different sizes share a batch.  w_m2s = 0 is the mode for partial scans (vertices the
    scan does not cover are pulled nowhere) and costs half the time.  sigma > 0 (metres) bounds the pull of far partners.
    The defaults (weights 100 and 100, sigma 0, lr 0.01, lambda 1e-3) are a float64 prototype's on the synthetic model of this package:
    untuned on real scans, and no real SMPL model was available when they were chosen."""

    def __init__(self, smpl, iters=100, lr=0.01, sigma=0.0, w_s2m=100., w_m2s=100., lambda_pose=1e-3, lambda_shape=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 keypoints=None):
        KeypointFitter.__init__(self, smpl, keypoints, iters, lr, 0.0, lambda_pose, lambda_shape, config.REGRESSOR_IMG_WH, betas, eps)
        self.smpl = smpl
        ok = lambda x: np.isfinite(x) and x >= 0
        if not (ok(float(sigma)) and ok(float(w_s2m)) and ok(float(w_m2s))):
            raise ValueError('ScanFitter: sigma, w_s2m and w_m2s must be finite and not negative')
        self.sigma, self.w_s2m, self.w_m2s = float(sigma), float(w_s2m), float(w_m2s)

    def scan_opts(self):
        return hipabi.ScanOptsStruct(self.sigma, self.w_s2m, self.w_m2s)

    def _start_translation(self, pose6d, shape, pts):
        """the centroid of the valid points minus the centroid of the start mesh (plain torch; once per call)"""
        B = pose6d.shape[0]
        R = rot6d_to_rotmat(pose6d.detach().contiguous()).view(B, 24, 3, 3).contiguous()
        verts = self.smpl.forward_arrays(shape.detach().contiguous(), R, want_joints=False)
        verts = verts[0] if isinstance(verts, (tuple, list)) else verts
        valid = torch.isfinite(pts).all(dim=2, keepdim=True)
        n = valid.sum(dim=1).clamp(min=1).to(torch.float32)
        centroid = torch.where(valid, pts, torch.zeros_like(pts)).sum(dim=1) / n
        return (centroid - verts.mean(dim=1)) * (valid.any(dim=1)).to(torch.float32)

    def _scan_inputs(self, transl, pose6d, shape, points, prior):
        hipabi.require_gpu_tensor(pose6d, 'pose6d', torch.float32)
        B = pose6d.shape[0]
        hipabi.require_gpu_tensor(points, 'points', torch.float32)
        if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3 or not 1 <= points.shape[1] <= (1 << 20):
            raise RuntimeError('ScanFitter: points must be [%d,P,3] with 1 <= P <= 2^20, got %s' % (B, tuple(points.shape)))
        pts = points.detach().contiguous()
        hipabi.require_gpu_tensor(shape, 'shape', torch.float32)
        if tuple(pose6d.shape) != (B, 144) or tuple(shape.shape) != (B, 10):
            raise RuntimeError('ScanFitter: pose6d must be [B,144] and shape [B,10], got %s and %s' % (tuple(pose6d.shape), tuple(shape.shape)))
        if transl is None:
            transl = self._start_translation(pose6d, shape, pts)
        hipabi.require_gpu_tensor(transl, 'transl', torch.float32)
        if tuple(transl.shape) != (B, 3):
            raise RuntimeError('ScanFitter: transl must be [%d,3], got %s' % (B, tuple(transl.shape)))
        est = torch.cat([transl.detach(), pose6d.detach(), shape.detach()], dim=1)
        if prior is None:
            est0 = est.clone()      # (the start: est itself moves)
        else:
            for p in (prior if isinstance(prior, (tuple, list)) else (prior,)):
                hipabi.require_gpu_tensor(p, 'prior', torch.float32)
            est0 = (torch.cat([p.detach() for p in prior], dim=1) if isinstance(prior, (tuple, list)) else prior.detach()).contiguous()
            if tuple(est0.shape) != (B, NE):
                raise RuntimeError('ScanFitter: prior must be [B,157] or a (transl, pose6d, shape) triple, got %s' % (tuple(est0.shape),))
        return est, est0, pts

    def _scan_buffers(self, B, dev, P):
        L = hipabi.lib()
        V = self.smpl.v_template.shape[0]
        f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        unit = torch.zeros(B, 3, device=dev, dtype=torch.float32)
        unit[:, 0] = 1.0
        return {'R': f(B, 24, 3, 3), 'betas': f(B, 10), 'verts': f(B, V, 3), 'dverts': f(B, V, 3), 'dtrans': f(B, 3), 'energy2': f(B, 2), 'drot': f(B, 24, 3, 3),
                'dbetas': f(B, 10), 'dx6': f(B, 144), 'e_kp': f(B, 1), 'g_kp': f(B, NE), 'est_kp': f(B, NE), 'cam_unit': unit,
                'targets': torch.zeros(B, self.n_kp, 2, device=dev, dtype=torch.float32), 'conf': torch.zeros(B, self.n_kp, device=dev, dtype=torch.float32),
                'nearest_vertex': torch.empty(B, P, device=dev, dtype=torch.int32), 'nearest_point': torch.empty(B, V, device=dev, dtype=torch.int32),
                'ws': torch.empty(L.straps_scan_energy_workspace_bytes(B, V, P) // 16 + 1, 2, device=dev, dtype=torch.float64),
                'ws_bwd': f(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)}

    def _scan_terms(self, est, est0, pts, buf):
        """the six evaluating entry points of one iteration at `est` (steps 1 to 6 of the loop); the results are left in `buf`"""
        L, st, B = hipabi.lib(), hipabi.stream_ptr(), est.shape[0]
        x6 = C.c_void_p(est.data_ptr() + 12)
        hipabi.check(L.straps_rot6d_fwd(x6, NE, 24, hipabi.ptr(buf['R']), B, st), 'straps_rot6d_fwd')
        buf['betas'].copy_(est[:, 147:])
        self.smpl.forward_arrays(buf['betas'], buf['R'], want_joints=False, out_verts=buf['verts'])
        scan_energy_raw(buf['verts'], est, NE, pts, self.scan_opts(), buf['energy2'], buf['dverts'], buf['dtrans'], buf['nearest_vertex'], buf['nearest_point'],
                        buf['ws'])
        hipabi.check(L.straps_smpl_bwd(C.byref(self.smpl._model_struct()), hipabi.ptr(buf['betas']), hipabi.ptr(buf['R']), hipabi.ptr(buf['dverts']), None,
                                       hipabi.ptr(buf['dbetas']), hipabi.ptr(buf['drot']), hipabi.ptr(buf['ws_bwd']), B, 0, st), 'straps_smpl_bwd')
        hipabi.check(L.straps_rot6d_bwd(x6, NE, 24, hipabi.ptr(buf['drot']), hipabi.ptr(buf['dx6']), 144, B, st), 'straps_rot6d_bwd')
        # the priors: all confidences zero, and a camera of (1, 0, 0) in the translation's place, so that nothing rests on how an unevaluated
        # residual treats the camera
        buf['est_kp'].copy_(est)
        buf['est_kp'][:, :3].copy_(buf['cam_unit'])
        fit_keypoints_raw(self._struct, self.opts(0), buf['est_kp'], est0, buf['targets'], buf['conf'], None, None, buf['e_kp'], buf['g_kp'], None, None, None)

    @hipabi.on_tensor_device
    def evaluate(self, transl, pose6d, shape, points, prior=None):
        """-> (energy [B], grad [B,157], terms [B,3] = (the priors, E_s2m, E_m2s; the scan terms unweighted)) at the given parameters"""
        est, est0, pts = self._scan_inputs(transl, pose6d, shape, points, prior)
        B, dev = est.shape[0], est.device
        buf = self._scan_buffers(B, dev, pts.shape[1])
        self._scan_terms(est, est0, pts, buf)
        energy = torch.empty(B, 1, device=dev, dtype=torch.float32)
        grad = torch.empty(B, NE, device=dev, dtype=torch.float32)
        fit_adam_raw(self.opts(), est, buf['g_kp'], buf['dtrans'], buf['dx6'], buf['dbetas'], buf['e_kp'], buf['energy2'], self.w_s2m, self.w_m2s, None, None,
                     energy, 0, grad, None, None, 0, True, False)
        return energy[:, 0], grad, torch.cat([buf['e_kp'], buf['energy2']], dim=1)

    @hipabi.on_tensor_device
    def __call__(self, transl, pose6d, shape, points, prior=None, state=None, trace=False):
        """transl [B,3] (metres; None: the centroid of the valid points minus the centroid of the start mesh), pose6d [B,144], shape [B,10],
        points [B,P,3], prior: the centre of the pose / shape priors ([B,157] or a (transl, pose6d, shape) triple; None = the start), state:
        the 'state' of an earlier call.
        -> {'transl' [B,3], 'pose' [B,144], 'shape' [B,10], 'pose_rotmats' [B,24,3,3], 'verts' [B,V,3] (the final posed vertices, translation
        added), 'energy0' [B], 'energy' [B] (at the returned parameters), 'energy_terms' [B,3] = (the priors, E_s2m, E_m2s), 'nearest_vertex'
        [B,P] int32 (-1 at invalid points), 'nearest_point' [B,V] int32, 'best': {'transl', 'pose', 'shape', 'energy'} (the iterate of the
        smallest energy), 'state', 'trace' [B,iters+1] if asked}.  iters + 1 evaluations, iters updates; every iteration is rot6d forward, SMPL
        forward, straps_scan_energy, SMPL backward, rot6d backward, straps_fit_keypoints with iters = 0 (the priors), straps_fit_adam, on
        buffers allocated before the loop.  The inputs are not modified.  Never synchronises; after one warm-up call at the same shapes it can
        be captured in torch.cuda.graph."""
        est, est0, pts = self._scan_inputs(transl, pose6d, shape, points, prior)
        B, dev = est.shape[0], est.device
        if state is None:
            m, v, step0 = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev), 0
        else:
            for k in ('exp_avg', 'exp_avg_sq'):
                hipabi.require_gpu_tensor(state[k], "state['%s']" % k, torch.float32)
                if tuple(state[k].shape) != (B, NE):
                    raise RuntimeError("ScanFitter: state['%s'] must be [%d,157], got %s" % (k, B, tuple(state[k].shape)))
            m, v = (state[k].detach().clone(memory_format=torch.contiguous_format) for k in ('exp_avg', 'exp_avg_sq'))
            step0 = int(state['step'])
        buf = self._scan_buffers(B, dev, pts.shape[1])
        energy = torch.empty(B, self.iters + 1, device=dev, dtype=torch.float32)
        best = torch.empty(B, NE, device=dev, dtype=torch.float32)
        best_e = torch.empty(B, device=dev, dtype=torch.float32)
        opts = self.opts()
        for i in range(self.iters + 1):
            self._scan_terms(est, est0, pts, buf)
            fit_adam_raw(opts, est, buf['g_kp'], buf['dtrans'], buf['dx6'], buf['dbetas'], buf['e_kp'], buf['energy2'], self.w_s2m, self.w_m2s, m, v,
                         energy, i, None, best, best_e, step0 + i, i == 0, i < self.iters)
        out = {'transl': est[:, :3], 'pose': est[:, 3:147], 'shape': est[:, 147:], 'pose_rotmats': buf['R'], 'verts': buf['verts'] + est[:, None, :3],
               'energy0': energy[:, 0], 'energy': energy[:, self.iters],
               'best': {'transl': best[:, :3], 'pose': best[:, 3:147], 'shape': best[:, 147:], 'energy': best_e},
               'energy_terms': torch.cat([buf['e_kp'], buf['energy2']], dim=1),
               'nearest_vertex': buf['nearest_vertex'], 'nearest_point': buf['nearest_point'],
               'state': {'exp_avg': m, 'exp_avg_sq': v, 'step': step0 + self.iters}}
        if trace:
            out['trace'] = energy
        return out


def fit_adam_subjects_raw(opts, est, offsets, frame_mask, g_kp, dcam, dx6, dbetas, e_kp, energy2, w_in, w_out, exp_avg, exp_avg_sq, shape_avg, shape_avg_sq,
                          energy, col, subject_energy, grad, best_est, best_energy, step, first, update, n_subjects):
    """one straps_fit_adam_subjects call on contiguous GPU tensors (None -> NULL): offsets int32 [G+1], frame_mask uint8 [B]; energy [B,ld] and
    subject_energy [G,ld'] receive column `col`"""
    hipabi.check(hipabi.lib().straps_fit_adam_subjects(
        C.byref(opts), hipabi.ptr(est), hipabi.ptr(offsets), hipabi.ptr(frame_mask), hipabi.ptr(g_kp), hipabi.ptr(dcam), hipabi.ptr(dx6), hipabi.ptr(dbetas),
        hipabi.ptr(e_kp), hipabi.ptr(energy2), w_in, w_out, hipabi.ptr(exp_avg), hipabi.ptr(exp_avg_sq), hipabi.ptr(shape_avg), hipabi.ptr(shape_avg_sq),
        hipabi.ptr(energy), 0 if energy is None else energy.shape[1], col, hipabi.ptr(subject_energy), 0 if subject_energy is None else subject_energy.shape[1],
        hipabi.ptr(grad), hipabi.ptr(best_est), hipabi.ptr(best_energy), int(step), int(bool(first)), int(bool(update)), est.shape[0], int(n_subjects),
        hipabi.stream_ptr()), 'straps_fit_adam_subjects')


def subject_mean_rows_raw(rows, ld, cols, offsets, frame_mask, out, batch, n_subjects):
    """one straps_subject_mean_rows call; rows: a tensor or a raw device address (a column block of a wider matrix), ld its row stride in floats"""
    rp = C.c_void_p(rows) if isinstance(rows, int) else hipabi.ptr(rows)
    hipabi.check(hipabi.lib().straps_subject_mean_rows(rp, ld, cols, hipabi.ptr(offsets), hipabi.ptr(frame_mask), hipabi.ptr(out), batch, n_subjects,
                                                       hipabi.stream_ptr()), 'straps_subject_mean_rows')


class SubjectFitter(SilhouetteFitter):
    """`SubjectFitter(smpl)(cam, pose6d, shape, frames_per_subject, silhouettes, joints2D)`: SilhouetteFitter's objective with ONE shape per
    subject.  The frames of a subject are consecutive rows; cam and pose stay per frame, the ten shape coefficients are shared: their gradient
    is the sum over the subject's frames, their Adam step is one per subject (straps_fit_adam_subjects, csrc/fit_subjects.hip).  Without
    silhouettes the keypoints and the priors alone are fitted (two launches per iteration).  What this buys is ONE shape that explains all the
    frames as well as per-frame shapes do; on the synthetic model neither recovers the true coefficients.  Untuned on real data."""

    def __init__(self, *a, **k):
        SilhouetteFitter.__init__(self, *a, **k)
        self._subjects = {}

    def subjects(self, frames_per_subject, B, dev):
        """host validation of the frame counts -> (G, offsets int32 [G+1], subject of every frame int64 [B], first row of every subject int64 [G]),
        device tensors uploaded once per value and device"""
        try:
            fps = tuple(int(n) for n in frames_per_subject)
            ok = len(fps) >= 1 and all(n >= 1 for n in fps) and all(n == m for n, m in zip(fps, frames_per_subject))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('SubjectFitter: frames_per_subject is a sequence of positive integers (got %r)' % (frames_per_subject,))
        if sum(fps) != B:
            raise ValueError('SubjectFitter: frames_per_subject sums to %d, the batch has %d frames' % (sum(fps), B))
        key = (fps, str(dev))
        if key not in self._subjects:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('SubjectFitter: the first call with a new frames_per_subject uploads its offsets: warm up before capturing')
            off = np.concatenate([[0], np.cumsum(fps)]).astype(np.int32)
            self._subjects[key] = (torch.from_numpy(off).to(dev), torch.from_numpy(np.repeat(np.arange(len(fps)), fps).astype(np.int64)).to(dev),
                                   torch.from_numpy(off[:-1].astype(np.int64)).to(dev))
        return (len(fps),) + self._subjects[key]

    def _subject_inputs(self, cam, pose6d, shape, frames_per_subject, silhouettes, joints2D, conf, prior, frame_mask):
        """-> est (shape tied to the subjects' means), est0, targets, conf, mask (None without silhouettes), frame mask, G, offsets, first rows"""
        if silhouettes is None and joints2D is None:
            raise ValueError('SubjectFitter: give silhouettes, joints2D or both')
        hipabi.require_gpu_tensor(cam, 'cam', torch.float32)
        B, dev = cam.shape[0], cam.device
        G, offsets, subject_of, first_rows = self.subjects(frames_per_subject, B, dev)
        if silhouettes is not None:
            est, est0, targets, conf, mask = self._sil_inputs(cam, pose6d, shape, silhouettes, joints2D, conf, prior)
        else:
            est, est0, targets, conf = self._inputs(cam, pose6d, shape, joints2D, conf, prior)
            mask = None
            if est0 is None:
                est0 = est.clone()      # (the prior centre stays per frame: the parameters as given, before the shapes are tied)
        fm = None
        if frame_mask is not None:
            hipabi.require_gpu_tensor(frame_mask, 'frame_mask')
            if tuple(frame_mask.shape) != (B,):
                raise RuntimeError('SubjectFitter: frame_mask must be [%d], got %s' % (B, tuple(frame_mask.shape)))
            fm = frame_mask.detach()
            fm = fm.contiguous() if fm.dtype == torch.uint8 else (fm != 0).to(torch.uint8)
        # the start: every subject's mean shape over its counting frames, in all its rows
        mean = torch.empty(G, 10, device=dev, dtype=torch.float32)
        subject_mean_rows_raw(est.data_ptr() + 147 * 4, NE, 10, offsets, fm, mean, B, G)
        est[:, 147:] = mean.index_select(0, subject_of)
        return est, est0, targets, conf, mask, fm, G, offsets, first_rows

    def _subject_buffers(self, B, dev, mask):
        if mask is not None:
            return self._buffers(B, dev, mask)
        f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        return {'e_kp': f(B, 1), 'g_kp': f(B, NE), 'kp2d': f(B, self.n_kp, 2), 'dcam': None, 'dx6': None, 'dbetas': None, 'energy2': None}

    def _subject_terms(self, est, est0, targets, conf, mask, buf):
        if mask is not None:
            self._terms(est, est0, targets, conf, mask, buf)
        else:      # (iters = 0 leaves est as it is, bit for bit)
            fit_keypoints_raw(self._struct, self.opts(0), est, est0, targets, conf, None, None, buf['e_kp'], buf['g_kp'], None, None, buf['kp2d'])

    @hipabi.on_tensor_device
    def evaluate(self, cam, pose6d, shape, frames_per_subject, silhouettes=None, joints2D=None, conf=None, prior=None, frame_mask=None):
        """-> (subject energy [G], grad [B,157] with the subject's summed shape gradient in columns 147..156 of all its rows, energy per frame [B])
        at the given cam and pose and the subjects' mean shapes"""
        est, est0, targets, conf, mask, fm, G, offsets, _ = self._subject_inputs(cam, pose6d, shape, frames_per_subject, silhouettes, joints2D, conf, prior,
                                                                                frame_mask)
        B, dev = est.shape[0], est.device
        buf = self._subject_buffers(B, dev, mask)
        self._subject_terms(est, est0, targets, conf, mask, buf)
        energy = torch.empty(B, 1, device=dev, dtype=torch.float32)
        sub = torch.empty(G, 1, device=dev, dtype=torch.float32)
        grad = torch.empty(B, NE, device=dev, dtype=torch.float32)
        fit_adam_subjects_raw(self.opts(), est, offsets, fm, buf['g_kp'], buf['dcam'], buf['dx6'], buf['dbetas'], buf['e_kp'], buf['energy2'], self.w_in,
                              self.w_out, None, None, None, None, energy, 0, sub, grad, None, None, 0, True, False, G)
        return sub[:, 0], grad, energy[:, 0]

    @hipabi.on_tensor_device
    def __call__(self, cam, pose6d, shape, frames_per_subject, silhouettes=None, joints2D=None, conf=None, prior=None, frame_mask=None, state=None,
                 trace=False):
        """cam [B,3], pose6d [B,144], shape [B,10]; frames_per_subject: positive ints summing to B (a host sequence: subject s owns the next
        frames_per_subject[s] rows); silhouettes [B,img_wh,img_wh] and / or joints2D as for SilhouetteFitter (at least one); prior: the centre
        of the priors, per frame (None = the parameters as given, so the tied shape is pulled towards every frame's own start); frame_mask [B]
        (bool / uint8) or None: a frame whose entry is 0 neither pulls its subject's shape nor counts in its energy, and receives the shape;
        state: the 'state' of an earlier call.  Every subject starts from the mean of its counting frames' shapes (straps_subject_mean_rows).
        -> SilhouetteFitter's keys ('energy_terms' only with silhouettes; 'energy0' / 'energy' per frame [B]) plus 'subject_shape' [G,10],
        'subject_energy0' / 'subject_energy' [G]; 'best' is chosen per subject by the subject's energy ('energy' [G]); 'state' also holds
        'shape_avg' / 'shape_avg_sq' [G,10]; 'trace' [G,iters+1] (subject energies) if asked.  iters + 1 evaluations, iters updates, every
        iteration SilhouetteFitter's six evaluating entry points (without silhouettes: straps_fit_keypoints with iters = 0) and
        straps_fit_adam_subjects, on buffers allocated before the loop.  The inputs are not modified.  Never synchronises; after one warm-up
        call with the same frames_per_subject and shapes it can be captured in torch.cuda.graph."""
        est, est0, targets, conf, mask, fm, G, offsets, first_rows = self._subject_inputs(cam, pose6d, shape, frames_per_subject, silhouettes, joints2D, conf,
                                                                                         prior, frame_mask)
        B, dev = est.shape[0], est.device
        if state is None:
            m, v, step0 = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev), 0
            sm, sv = torch.zeros(G, 10, device=dev), torch.zeros(G, 10, device=dev)
        else:
            for k, want in (('exp_avg', (B, NE)), ('exp_avg_sq', (B, NE)), ('shape_avg', (G, 10)), ('shape_avg_sq', (G, 10))):
                if k not in state:
                    raise RuntimeError("SubjectFitter: state has no '%s' (the state of a per-frame fitter cannot be carried over)" % k)
                hipabi.require_gpu_tensor(state[k], "state['%s']" % k, torch.float32)
                if tuple(state[k].shape) != want:
                    raise RuntimeError("SubjectFitter: state['%s'] must be %s, got %s" % (k, list(want), tuple(state[k].shape)))
            m, v, sm, sv = (state[k].detach().clone(memory_format=torch.contiguous_format) for k in ('exp_avg', 'exp_avg_sq', 'shape_avg', 'shape_avg_sq'))
            step0 = int(state['step'])
        buf = self._subject_buffers(B, dev, mask)
        energy = torch.empty(B, self.iters + 1, device=dev, dtype=torch.float32)
        sub = torch.empty(G, self.iters + 1, device=dev, dtype=torch.float32)
        best = torch.empty(B, NE, device=dev, dtype=torch.float32)
        best_e = torch.empty(G, device=dev, dtype=torch.float32)
        opts = self.opts()
        for i in range(self.iters + 1):
            self._subject_terms(est, est0, targets, conf, mask, buf)
            fit_adam_subjects_raw(opts, est, offsets, fm, buf['g_kp'], buf['dcam'], buf['dx6'], buf['dbetas'], buf['e_kp'], buf['energy2'], self.w_in, self.w_out,
                                  m, v, sm, sv, energy, i, sub, None, best, best_e, step0 + i, i == 0, i < self.iters, G)
        pose = est[:, 3:147]
        out = {'cam_wp': est[:, :3], 'pose': pose, 'shape': est[:, 147:],
               'pose_rotmats': buf['R'] if mask is not None else rot6d_to_rotmat(pose).view(B, 24, 3, 3),
               'energy0': energy[:, 0], 'energy': energy[:, self.iters],
               'subject_shape': est[:, 147:].index_select(0, first_rows), 'subject_energy0': sub[:, 0], 'subject_energy': sub[:, self.iters],
               'best': {'cam_wp': best[:, :3], 'pose': best[:, 3:147], 'shape': best[:, 147:], 'energy': best_e},
               'joints2D': cam_utils.undo_keypoint_normalisation(buf['kp2d'], self.img_wh),
               'state': {'exp_avg': m, 'exp_avg_sq': v, 'shape_avg': sm, 'shape_avg_sq': sv, 'step': step0 + self.iters}}
        if mask is not None:
            out['energy_terms'] = torch.cat([buf['e_kp'], buf['energy2']], dim=1)
        if trace:
            out['trace'] = sub
        return out


SHAPE0 = 147      # first shape column of a [B,157] estimate row


class MeasurementFitter:
    """`MeasurementFitter(smpl, measurer)(shape, targets)`: the ten shape coefficients fitted to KNOWN body measurements -- a height, a chest
    or waist girth -- of the T-pose body, by Adam on

        E = sum_m w_m (value_m / target_m - 1)^2 + lambda_shape |beta - beta0|^2        (straps_measure_residual, include/straps_hip.h)

    measurer: a measure.BodyMeasurer on the SMPL module's device; with tape specs (tape_girth / section_girth: what a tape reads) only one
    made with tape_gradients=True (ValueError otherwise: without it a measurer does not differentiate tape girths).  targets
    [B,M] in the order of measurer.names, NaN (or 0) = unknown; or a dict name -> float or [B] tensor, absent names unknown (a dict is
    turned into a tensor by host code: pass a tensor to a call that is to be captured).  weights [B,M] or None (all ones); a weight that
    is not > 0 makes the column unknown.  The residuals are relative, so a height in metres and a volume in cubic metres pull alike.
    One iteration is SMPL forward with identity rotations, straps_measure_mesh, straps_measure_residual, straps_measure_mesh_bwd, straps_smpl_bwd
    and straps_fit_adam on a [B,157] row whose cam and pose columns have zero gradient and come back as they went in.  With tape specs an
    iteration also runs straps_measure_tape (before the residual) and straps_measure_tape_bwd with accumulate = 1 (onto
    straps_measure_mesh_bwd's output); a call without specs of one sort is not made.
    The defaults (lr 0.05, 100 iterations, lambda 1e-3, relative residuals) are those of a float64 prototype on the synthetic model of this
    package: untuned on a real SMPL model.  On the synthetic model, whose faces are a triangle soup, the fit lowers the energy but cannot be
    expected to recover the coefficients."""

    def __init__(self, smpl, measurer, iters=100, lr=0.05, lambda_shape=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if measurer.tape_columns and not getattr(measurer, 'tape_gradients', False):
            raise ValueError('MeasurementFitter: the measurer has the tape specs %r: tape girths (straps_measure_tape) have no gradient without '
                             'BodyMeasurer(..., tape_gradients=True)' % (list(measurer.tape_names),))
        hipabi.require_gpu_tensor(smpl._k_j_template, 'SMPL model buffers (call .to(device))')
        hipabi.require_gpu_tensor(measurer.faces, 'BodyMeasurer buffers (call .to(device))', torch.int32)
        if measurer.num_vertices != smpl.v_template.shape[0]:
            raise ValueError('MeasurementFitter: the measurer was built for %d vertices, the SMPL model has %d (BodyMeasurer.from_smpl)'
                             % (measurer.num_vertices, smpl.v_template.shape[0]))
        if measurer.needs_joints > 90:
            raise ValueError('MeasurementFitter: the measurer reads joint %d, the SMPL module gives 90' % (measurer.needs_joints - 1))
        self.smpl, self.measurer, self.device = smpl, measurer, smpl._k_j_template.device
        self.iters, self.lr, self.lambda_shape = int(iters), float(lr), float(lambda_shape)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if self.iters < 0 or not self.lambda_shape >= 0:
            raise ValueError('MeasurementFitter: iters and lambda_shape must not be negative')
        # with tape specs: the columns of `values` that each library call fills, as device indices (uploaded here, so that a call can be captured)
        self._columns = None
        if measurer.tape_columns:
            self._columns = tuple(torch.tensor(c, dtype=torch.int64).to(self.device) for c in (list(measurer.mesh_columns), list(measurer.tape_columns)))

    def opts(self):
        return hipabi.FitOptsStruct(self.iters, 0, self.lr, self.lr, self.lr, self.betas[0], self.betas[1], self.eps, 0.0, 0.0, self.lambda_shape, 0.0)

    def targets_tensor(self, targets, B, dev):
        """targets [B,M] or a dict by measurement name -> float32 [B,M], NaN where unknown"""
        M = len(self.measurer.names)
        if isinstance(targets, dict):
            unknown = [n for n in targets if n not in self.measurer.names]
            if unknown:
                raise ValueError('MeasurementFitter: the measurer has no measurement %r (it has %r)' % (unknown, list(self.measurer.names)))
            t = torch.full((B, M), float('nan'), device=dev, dtype=torch.float32)
            for n, v in targets.items():
                t[:, self.measurer.names.index(n)] = v.detach().to(dev, torch.float32) if isinstance(v, torch.Tensor) else float(v)
            return t
        hipabi.require_gpu_tensor(targets, 'targets', torch.float32)
        if tuple(targets.shape) != (B, M):
            raise RuntimeError('MeasurementFitter: targets must be [%d,%d], got %s' % (B, M, tuple(targets.shape)))
        return targets.detach().contiguous()

    def _inputs(self, shape, targets, weights, prior):
        hipabi.require_gpu_tensor(shape, 'shape', torch.float32)
        if shape.dim() != 2 or shape.shape[1] != 10 or shape.shape[0] < 1:
            raise RuntimeError('MeasurementFitter: shape must be [B,10], got %s' % (tuple(shape.shape),))
        B, dev = shape.shape[0], shape.device
        est = torch.zeros(B, NE, device=dev, dtype=torch.float32)
        est[:, SHAPE0:] = shape.detach()
        est0 = est.clone()
        if prior is not None:
            hipabi.require_gpu_tensor(prior, 'prior', torch.float32)
            if tuple(prior.shape) != (B, 10):
                raise RuntimeError('MeasurementFitter: prior must be [%d,10], got %s' % (B, tuple(prior.shape)))
            est0[:, SHAPE0:] = prior.detach()
        targets = self.targets_tensor(targets, B, dev)
        if weights is not None:
            hipabi.require_gpu_tensor(weights, 'weights', torch.float32)
            if tuple(weights.shape) != tuple(targets.shape):
                raise RuntimeError('MeasurementFitter: weights must be %s, got %s' % (list(targets.shape), tuple(weights.shape)))
            weights = weights.detach().contiguous()
        return est, est0, targets, weights

    def _buffers(self, B, dev):
        L, ms = hipabi.lib(), self.measurer
        V, F, M, P = self.smpl.v_template.shape[0], ms.faces.shape[0], len(ms.names), ms.needs_joints
        Mm, T = len(ms.mesh_columns), len(ms.tape_columns)
        f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        buf = {'R': torch.eye(3, device=dev, dtype=torch.float32).expand(B, 24, 3, 3).contiguous(), 'betas': f(B, 10), 'verts': f(B, V, 3), 'joints': f(B, 90, 3),
               'points': f(B, P, 3) if P else None, 'values': f(B, M), 'dvalues': f(B, M), 'e': f(B), 'g': f(B, NE), 'dverts': f(B, V, 3),
               'djoints': torch.zeros(B, 90, 3, device=dev, dtype=torch.float32) if P else None, 'dbetas': f(B, 10), 'drot': f(B, 24, 3, 3),
               'ws': torch.empty(L.straps_measure_workspace_bytes(B, V, F, Mm) // 8, device=dev, dtype=torch.float64),
               'ws_grad': torch.empty(L.straps_measure_bwd_workspace_bytes(B, V, F, Mm) // 8, device=dev, dtype=torch.float64),
               'ws_bwd': f(L.straps_smpl_bwd_workspace_bytes(B, 0) // 4)}
        if T:      # the two calls' own columns, gathered into / scattered from `values` / `dvalues` in the order of measurer.names
            buf.update({'mesh_values': f(B, Mm), 'mesh_dvalues': f(B, Mm), 'tape_values': f(B, T), 'tape_dvalues': f(B, T),
                        'ws_tape': torch.empty(ms.tape_workspace_bytes(B) // 8, device=dev, dtype=torch.float64),
                        'ws_tape_grad': torch.empty(ms.tape_grad_workspace_bytes(B, V) // 8, device=dev, dtype=torch.float64)})
        return buf

    def _terms(self, est, est0, targets, weights, buf):
        """the five evaluating entry points of one iteration at `est` (steps 1 to 5 of the loop; seven with tape specs); the results are left in `buf`"""
        L, st, B, ms = hipabi.lib(), hipabi.stream_ptr(), est.shape[0], self.measurer
        buf['betas'].copy_(est[:, SHAPE0:])
        self.smpl.forward_arrays(buf['betas'], buf['R'], out_verts=buf['verts'], out_joints=buf['joints'])
        if buf['points'] is not None:
            buf['points'].copy_(buf['joints'][:, :ms.needs_joints])
        tape = bool(ms.tape_columns)
        if not tape:
            ms.measure_raw(buf['verts'], buf['points'], buf['values'], buf['ws'])
        else:
            mesh_idx, tape_idx = self._columns
            if ms.mesh_columns:
                ms.measure_raw(buf['verts'], buf['points'], buf['mesh_values'], buf['ws'])
                buf['values'].index_copy_(1, mesh_idx, buf['mesh_values'])
            ms.measure_tape_raw(buf['verts'], buf['points'], buf['tape_values'], buf['ws_tape'])
            buf['values'].index_copy_(1, tape_idx, buf['tape_values'])
        hipabi.check(L.straps_measure_residual(hipabi.ptr(buf['values']), hipabi.ptr(targets), hipabi.ptr(weights), hipabi.ptr(est), hipabi.ptr(est0),
                                               self.lambda_shape, hipabi.ptr(buf['e']), hipabi.ptr(buf['dvalues']), hipabi.ptr(buf['g']), B, targets.shape[1], st),
                     'straps_measure_residual')
        if not tape:
            ms.measure_grad_raw(buf['verts'], buf['points'], buf['dvalues'], buf['dverts'], buf['djoints'], buf['ws_grad'])
        else:
            if ms.mesh_columns:
                torch.index_select(buf['dvalues'], 1, mesh_idx, out=buf['mesh_dvalues'])
                ms.measure_grad_raw(buf['verts'], buf['points'], buf['mesh_dvalues'], buf['dverts'], buf['djoints'], buf['ws_grad'])
            torch.index_select(buf['dvalues'], 1, tape_idx, out=buf['tape_dvalues'])
            ms.measure_tape_grad_raw(buf['verts'], buf['points'], buf['tape_dvalues'], buf['dverts'], buf['djoints'], buf['ws_tape_grad'],
                                     accumulate=bool(ms.mesh_columns))
        hipabi.check(L.straps_smpl_bwd(C.byref(self.smpl._model_struct()), hipabi.ptr(buf['betas']), hipabi.ptr(buf['R']), hipabi.ptr(buf['dverts']),
                                       hipabi.ptr(buf['djoints']), hipabi.ptr(buf['dbetas']), hipabi.ptr(buf['drot']), hipabi.ptr(buf['ws_bwd']), B, 0, st),
                     'straps_smpl_bwd')

    @hipabi.on_tensor_device
    def evaluate(self, shape, targets, weights=None, prior=None):
        """-> (energy [B], grad [B,10], values [B,M]) at the given shape"""
        est, est0, targets, weights = self._inputs(shape, targets, weights, prior)
        B, dev = est.shape[0], est.device
        buf = self._buffers(B, dev)
        self._terms(est, est0, targets, weights, buf)
        energy = torch.empty(B, 1, device=dev, dtype=torch.float32)
        grad = torch.empty(B, NE, device=dev, dtype=torch.float32)
        fit_adam_raw(self.opts(), est, buf['g'], None, None, buf['dbetas'], buf['e'], None, 0.0, 0.0, None, None, energy, 0, grad, None, None, 0, True, False)
        return energy[:, 0], grad[:, SHAPE0:], buf['values']

    @hipabi.on_tensor_device
    def __call__(self, shape, targets, weights=None, prior=None, state=None, trace=False):
        """shape [B,10] (the start), targets / weights as the class docstring says, prior [B,10]: the centre of the shape prior (None = the
        start), state: the 'state' of an earlier call (the Adam moments and step count go on from there).
        -> {'shape' [B,10], 'values' [B,M] (the measurements at the returned shape), 'energy0' [B], 'energy' [B] (at the returned shape),
        'best': {'shape', 'energy'} (the iterate of the smallest energy), 'state', 'trace' [B,iters+1] if asked}.  iters + 1 evaluations,
        iters updates, on buffers allocated before the loop.  The inputs are not modified.  Never synchronises; after one warm-up call at the
        same shapes it can be captured in torch.cuda.graph."""
        est, est0, targets, weights = self._inputs(shape, targets, weights, prior)
        B, dev = est.shape[0], est.device
        if state is None:
            m, v, step0 = torch.zeros(B, NE, device=dev), torch.zeros(B, NE, device=dev), 0
        else:
            for k in ('exp_avg', 'exp_avg_sq'):
                hipabi.require_gpu_tensor(state[k], "state['%s']" % k, torch.float32)
                if tuple(state[k].shape) != (B, NE):
                    raise RuntimeError("MeasurementFitter: state['%s'] must be [%d,157], got %s" % (k, B, tuple(state[k].shape)))
            m, v = (state[k].detach().clone(memory_format=torch.contiguous_format) for k in ('exp_avg', 'exp_avg_sq'))
            step0 = int(state['step'])
        buf = self._buffers(B, dev)
        energy = torch.empty(B, self.iters + 1, device=dev, dtype=torch.float32)
        best = torch.empty(B, NE, device=dev, dtype=torch.float32)
        best_e = torch.empty(B, device=dev, dtype=torch.float32)
        opts = self.opts()
        for i in range(self.iters + 1):
            self._terms(est, est0, targets, weights, buf)
            fit_adam_raw(opts, est, buf['g'], None, None, buf['dbetas'], buf['e'], None, 0.0, 0.0, m, v, energy, i, None, best, best_e, step0 + i, i == 0,
                         i < self.iters)
        out = {'shape': est[:, SHAPE0:], 'values': buf['values'], 'energy0': energy[:, 0], 'energy': energy[:, self.iters],
               'best': {'shape': best[:, SHAPE0:], 'energy': best_e}, 'state': {'exp_avg': m, 'exp_avg_sq': v, 'step': step0 + self.iters}}
        if trace:
            out['trace'] = energy
        return out
