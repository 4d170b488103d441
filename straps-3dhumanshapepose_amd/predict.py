"""The predict path for a batch, on the device (reference predict/predict_3D.py:116-149, run_predict.py).

The reference turns each image's detector outputs -- a silhouette and 17 keypoints -- into the regressor's 18-channel input on the
host, in numpy and cv2: `crop_and_resize_silhouette_joints` (utils/image_utils.py:108-163), `create_proxy_representation`
(predict_3D.py:67-76) and the numpy `convert_2Djoints_to_gaussian_heatmaps` (utils/label_conversions.py:58-87).  Here that is one
library call for the whole batch (straps_predict_proxy_input, csrc/predict.hip) on tensors that are already on the GPU, and
`Predictor` chains it with the one-call regressor, the SMPL forward and the orthographic projection.

These are the PREDICT-side semantics, not the training-side ones of image_utils.batch_crop_and_resize / label_conversions: the window
is not clamped to the frame (what sticks out reads as zero, and the joints are shifted by the unclamped corner), and the heat maps are
the numpy ones (float64 joints truncated to int16, a float64 Gaussian).  The detectors, pad_to_square and the resize of the RGB image are
not part of this package; of the visualisation, the two rendered pictures of predict_3D.py:169-178 are (`Predictor.render`).
`Predictor.measure` turns the predicted T-pose body into height, volume, girths and limb lengths, and with posed=True measures the body as
posed, for tape girths whose planes follow the limbs (measure.py).
"""
import numpy as np
import torch

from . import cam_utils, config, hipabi
from .fit import SilhouetteFitter, SubjectFitter
from .infer import InferenceRegressor

_PATCHES = {}


def heatmap_patch(std=4):
    """-> [4 std, 4 std] float32 numpy array: the truncated Gaussian of utils/label_conversions.py:68-71, computed as there (float64
    linspace, sqrt, exp) and cast as numpy casts it on assignment into the float32 heat map -- hence bit-identical heat maps."""
    std = int(std)
    if std <= 0:
        raise ValueError('heatmap_patch: std must be positive (got %r)' % (std,))
    # 4 std samples of [-2 std, 2 std] per axis; the distance goes through sqrt and is squared again, as there: x^2 + y^2 directly
    # would differ in the last bit
    t = np.linspace(-2 * std, 2 * std, 4 * std)
    dist = np.sqrt(t[None, :] * t[None, :] + t[:, None] * t[:, None])
    return np.exp(-(dist ** 2 / (2.0 * std ** 2))).astype(np.float32)


def _device_patch(device, std):
    """the patch on `device`, cached per (device, std).  The first use copies from the host: make it outside a graph capture."""
    key = (str(device), int(std))
    if key not in _PATCHES:
        _PATCHES[key] = torch.from_numpy(heatmap_patch(std)).to(device)
    return _PATCHES[key]


@hipabi.on_tensor_device
def create_proxy_representation_batch(silhouettes, joints2D, out_wh=config.REGRESSOR_IMG_WH, bbox_scale_factor=1.2, std=4):
    """silhouettes [B,H,W] (GPU; uint8, bool, or a float tensor of integer labels 0..255; 0 = background), joints2D [B,J,2] or [B,J,3]
    (GPU float; a confidence column is ignored) -> (proxy_rep [B,1+J,out_wh,out_wh] float32, joints2D_cropped [B,J,2] float32,
    boxes [B,6] int32 = {wr0, wc0, wr1, wc1, valid, 0}).

    Per sample exactly what the reference's crop_and_resize_silhouette_joints + create_proxy_representation compute.  Where the
    reference raises (an empty silhouette; a window that truncates to zero height or width, e.g. a one-pixel silhouette) the sample's
    `valid` is 0 and its proxy and joints are all zeros.  Never synchronises; runs on the current stream; capturable."""
    hipabi.require_gpu_tensor(silhouettes, 'silhouettes')
    hipabi.require_gpu_tensor(joints2D, 'joints2D')
    if silhouettes.dim() != 3:
        raise RuntimeError('create_proxy_representation_batch: silhouettes must be [B,H,W], got %s' % (tuple(silhouettes.shape),))
    B, H, W = silhouettes.shape
    if joints2D.dim() != 3 or joints2D.shape[0] != B or joints2D.shape[2] not in (2, 3):
        raise RuntimeError('create_proxy_representation_batch: joints2D must be [%d,J,2] or [%d,J,3], got %s' % (B, B, tuple(joints2D.shape)))
    if silhouettes.dtype not in (torch.uint8, torch.bool) and not silhouettes.dtype.is_floating_point:
        raise RuntimeError('create_proxy_representation_batch: silhouettes must be uint8, bool or float (got %s)' % silhouettes.dtype)
    dev = silhouettes.device
    sil = silhouettes.to(torch.uint8).contiguous()
    j = joints2D.float().contiguous()
    nj = j.shape[1]
    patch = _device_patch(dev, std)
    out = torch.empty(B, 1 + nj, out_wh, out_wh, device=dev, dtype=torch.float32)
    jout = torch.empty(B, nj, 2, device=dev, dtype=torch.float32)
    boxes = torch.empty(B, 6, device=dev, dtype=torch.int32)
    hipabi.check(hipabi.lib().straps_predict_proxy_input(hipabi.ptr(sil), hipabi.ptr(j), j.shape[2], hipabi.ptr(patch), int(std),
                                                         float(bbox_scale_factor), hipabi.ptr(out), hipabi.ptr(jout), hipabi.ptr(boxes),
                                                         B, H, W, nj, int(out_wh), hipabi.stream_ptr()), 'straps_predict_proxy_input')
    return out, jout, boxes


class Predictor:
    """predict_3D.py:116-149 for a batch: `Predictor(regressor, smpl)(silhouettes, joints2D)` -> dict of device tensors.

    regressor: a SingleInputRegressor (wrapped in an InferenceRegressor with `precision`) or an InferenceRegressor; smpl: the SMPL
    module on the same GPU.  Only existing entry points are composed -- create_proxy_representation_batch, InferenceRegressor(...,
    rotmats=True), SMPL.forward_arrays, cam_utils -- so every result equals that composition written by hand, bit for bit.  No call
    synchronises; after one warm-up call at the same shapes the call can be captured in `torch.cuda.graph`.  After the regressor's
    weights change, `refresh()`."""

    def __init__(self, regressor, smpl, precision=None, out_wh=config.REGRESSOR_IMG_WH, bbox_scale_factor=1.2, std=4):
        self.infer = regressor if isinstance(regressor, InferenceRegressor) else InferenceRegressor(regressor, precision)
        self.smpl = smpl
        self.out_wh, self.bbox_scale_factor, self.std = int(out_wh), float(bbox_scale_factor), int(std)
        self._identity = None
        self._render_consts = {}

    def refresh(self):
        self.infer.refresh()
        return self

    def _identity_rotmats(self, B, device):
        if self._identity is None or self._identity.shape[0] < B or self._identity.device != device:
            eye = torch.eye(3, device=device, dtype=torch.float32).expand(B, 24, 3, 3).contiguous()
            if torch.cuda.is_current_stream_capturing():
                return eye                      # (memory of the capture's pool: not kept)
            self._identity = eye
        return self._identity[:B]

    @hipabi.on_tensor_device
    def __call__(self, silhouettes, joints2D, vis_wh=None):
        """-> {'proxy_rep' [B,1+J,out,out], 'cam_wp' [B,3], 'pose' [B,144] (6-D), 'pose_rotmats' [B,24,3,3], 'shape' [B,10], 'vertices' [B,6890,3],
        'joints' [B,90,3], 'vertices2D' [B,6890,2] in pixels of a vis_wh (default out_wh) square, 'reposed_vertices' [B,6890,3] (identity
        rotations, the predicted shape), 'joints2D_cropped' [B,J,2], 'boxes' [B,6], 'valid' [B] bool}.  An invalid sample (see
        create_proxy_representation_batch) gets the regressor's answer to an all-zero input; `valid` says which."""
        with torch.no_grad():
            proxy, jc, boxes = create_proxy_representation_batch(silhouettes, joints2D, self.out_wh, self.bbox_scale_factor, self.std)
            cam, pose, shape, rot = self.infer(proxy, rotmats=True)
            return self._tail(proxy, cam, pose, shape, rot, jc, boxes, vis_wh)

    def _tail(self, proxy, cam, pose, shape, rot, jc, boxes, vis_wh):
        """parameters -> the result dict (under no_grad): SMPL forward, projection to pixels, reposed vertices"""
        B = proxy.shape[0]
        rot = rot.view(B, 24, 3, 3)
        shape = shape.contiguous()
        verts, joints = self.smpl.forward_arrays(shape, rot)
        v2d = cam_utils.undo_keypoint_normalisation(cam_utils.orthographic_project_torch(verts, cam), vis_wh or self.out_wh)
        reposed, _ = self.smpl.forward_arrays(shape, self._identity_rotmats(B, proxy.device), want_joints=False)
        return {'proxy_rep': proxy, 'cam_wp': cam, 'pose': pose, 'pose_rotmats': rot, 'shape': shape, 'vertices': verts, 'joints': joints,
                'vertices2D': v2d, 'reposed_vertices': reposed, 'joints2D_cropped': jc, 'boxes': boxes, 'valid': boxes[:, 4] != 0}

    @hipabi.on_tensor_device
    def refine(self, out, fitter, conf=None, subjects=None):
        """test-time fitting after the regressor: the parameters of `out` (a result of __call__) are fitted to out['joints2D_cropped'] by
        `fitter` (a fit.KeypointFitter, or a fit.SilhouetteFitter -- then also to the silhouette the regressor was given, out['proxy_rep'][:, 0] != 0,
        with 'energy_terms' [B,3] among the results -- on this SMPL module, with as many keypoints as joints2D had; its img_wh must be this predictor's
        out_wh: ValueError otherwise), with the regressor's answer as the centre of the priors.  conf [B,J] or None (all ones).  An invalid sample keeps its
        parameters bit for bit: its confidences are zeroed.
        subjects: for a fit.SubjectFitter (ValueError without it, and with it for any other fitter) the frames_per_subject list -- positive ints
        summing to B, subject s is the next subjects[s] frames: one shape per subject.  An invalid sample is passed as frame_mask = 0: it neither pulls
        its subject's shape nor counts in its energy, keeps its cam and pose bit for bit and receives its subject's shape.  The result then also has
        'subject_shape' [G,10], 'subject_energy0' / 'subject_energy' [G] and 'subjects' (the list).
        -> a dict with the keys of __call__, rebuilt from the fitted parameters by the same tail, plus the fitter's 'energy0' and 'energy'
        [B].  Never synchronises; capturable after a warm-up call."""
        with torch.no_grad():
            jc, valid = out['joints2D_cropped'], out['valid']
            B = jc.shape[0]
            if float(fitter.img_wh) != float(self.out_wh) or fitter.n_kp != jc.shape[1]:
                raise ValueError('Predictor.refine: the fitter normalises targets by img_wh = %g and has %d keypoints; this predictor crops to %d pixels '
                                 'and has %d joints' % (fitter.img_wh, fitter.n_kp, self.out_wh, jc.shape[1]))
            conf = torch.ones(B, jc.shape[1], device=jc.device, dtype=torch.float32) if conf is None else conf.float()
            conf = conf * valid[:, None].to(conf.dtype)
            if isinstance(fitter, SubjectFitter) != (subjects is not None):
                raise ValueError('Predictor.refine: subjects= is required for a SubjectFitter and taken by no other fitter')
            if isinstance(fitter, SilhouetteFitter):
                # the silhouette the regressor was given is the target; an invalid sample's mask is emptied: with zero confidences every gradient is zero
                target = (out['proxy_rep'][:, 0] != 0) & valid[:, None, None].to(torch.bool)
                if subjects is not None:      # (a SubjectFitter: an invalid sample does not count towards its subject's shape either)
                    fit = fitter(out['cam_wp'].contiguous(), out['pose'].contiguous(), out['shape'].contiguous(), subjects, target, jc, conf=conf, frame_mask=valid)
                else:
                    fit = fitter(out['cam_wp'].contiguous(), out['pose'].contiguous(), out['shape'].contiguous(), target, jc, conf=conf)
            else:
                fit = fitter(out['cam_wp'].contiguous(), out['pose'].contiguous(), out['shape'].contiguous(), jc, conf=conf)
            res = self._tail(out['proxy_rep'], fit['cam_wp'], fit['pose'], fit['shape'], fit['pose_rotmats'], jc, out['boxes'], None)
        res['energy0'], res['energy'] = fit['energy0'], fit['energy']
        if 'energy_terms' in fit:
            res['energy_terms'] = fit['energy_terms']
        if subjects is not None:
            res['subject_shape'], res['subject_energy0'], res['subject_energy'] = fit['subject_shape'], fit['subject_energy0'], fit['subject_energy']
            res['subjects'] = [int(n) for n in subjects]
        return res

    @hipabi.on_tensor_device
    def refine_shape(self, out, mfitter, targets, weights=None):
        """the predicted shape made to agree with KNOWN measurements of the subject (a height, a girth): `out` a result of __call__ or refine,
        `mfitter` a fit.MeasurementFitter on this SMPL module, targets / weights as MeasurementFitter.__call__ takes them ([B,M] tensors in the
        order of the measurer's names, NaN = unknown; targets may be a dict by name).  The fit starts from out['shape'] and uses it as the
        centre of the shape prior; cam and pose stay as they are.  An invalid sample gets all-zero weights and keeps its shape bit for bit.
        -> a dict with the keys of __call__, rebuilt from the fitted shape by the same tail, plus the fitter's 'energy0' and 'energy' [B] and
        'measurements' [B,M]: the values at the fitted shape.  Never synchronises (with tensor targets); capturable after a warm-up call."""
        with torch.no_grad():
            shape, valid = out['shape'].contiguous(), out['valid']
            B = shape.shape[0]
            targets = mfitter.targets_tensor(targets, B, shape.device)
            w = torch.ones_like(targets) if weights is None else weights.float()
            w = w * valid[:, None].to(w.dtype)
            fit = mfitter(shape, targets, weights=w.contiguous())
            res = self._tail(out['proxy_rep'], out['cam_wp'], out['pose'], fit['shape'], out['pose_rotmats'], out['joints2D_cropped'], out['boxes'], None)
        res['energy0'], res['energy'], res['measurements'] = fit['energy0'], fit['energy'], fit['values']
        return res

    @hipabi.on_tensor_device
    def render(self, out, renderer, images=None):
        """predict_3D.py:170-174 for the batch: `out` a result of __call__ or refine, `renderer` a nmr_renderer.WeakPerspectiveMeshRenderer on the
        same GPU, images None or uint8 [B,wh,wh,3] on the GPU (the pictures the predictions are drawn over; wh must be renderer.img_wh:
        ValueError otherwise).
        -> {'rend': out['vertices'] under out['cam_wp'] over `images` (over the renderer's background colour without them),
            'reposed': out['reposed_vertices'] under the camera [0.8, 0, -0.2], turned by 180 degrees about x, over the background colour},
        uint8 [B,wh,wh,3] each.  Never synchronises after the first call on a device (which uploads the two constants); capturable after it."""
        verts = out['vertices']
        B, wh = verts.shape[0], renderer.img_wh
        if images is not None and (images.dim() != 4 or tuple(images.shape[1:3]) != (wh, wh)):
            raise ValueError('Predictor.render: the renderer draws %d x %d pictures, `images` is %s' % (wh, wh, tuple(images.shape)))
        key = str(verts.device)
        if key not in self._render_consts:
            self._render_consts[key] = (torch.tensor([0.8, 0.0, -0.2], device=verts.device, dtype=torch.float32),
                                        torch.tensor([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]], device=verts.device, dtype=torch.float32))
        cam, rx180 = self._render_consts[key]
        with torch.no_grad():
            return {'rend': renderer(verts, out['cam_wp'], background=images),
                    'reposed': renderer(out['reposed_vertices'], cam.expand(B, 3).contiguous(), rotation=rx180)}

    @hipabi.on_tensor_device
    def measure(self, out, measurer, posed=False):
        """body measurements of the prediction: `out` a result of __call__ or refine, `measurer` a measure.BodyMeasurer on the same GPU.  Measures
        out['reposed_vertices'] -- the predicted shape in the T-pose -- with the T-pose joints as anchor points: one extra SMPL forward on
        out['shape'] with identity rotations (its vertices are the reposed vertices again and are dropped).  posed=True: measures
        out['vertices'], the body as posed, with out['joints'] as anchor points instead (no SMPL forward) -- for specs whose planes follow the
        body (measure.posed_measurements(): `toward=`); planes with a fixed normal mean little there.  `out` is not changed.
        -> {'values': [B,M] float32, name: [B], ...} (BodyMeasurer.forward).  Never synchronises; capturable after a warm-up call."""
        if posed:
            with torch.no_grad():
                return measurer(out['vertices'], out['joints'])
        with torch.no_grad():
            shape = out['shape'].contiguous()
            B = shape.shape[0]
            _, joints = self.smpl.forward_arrays(shape, self._identity_rotmats(B, shape.device))
            return measurer(out['reposed_vertices'], joints)

    @hipabi.on_tensor_device
    def measure_subjects(self, out, measurer):
        """body measurements per SUBJECT: `out` a result of refine(..., subjects=...), `measurer` a measure.BodyMeasurer on the same GPU.  Measures the
        T-pose of out['subject_shape'] with the T-pose joints as anchor points -- `measure`'s non-posed route on G bodies: one SMPL forward with identity
        rotations.  -> {'values': [G,M] float32, name: [G], ...}.  Never synchronises; capturable after a warm-up call."""
        if 'subject_shape' not in out:
            raise ValueError("Predictor.measure_subjects: `out` has no 'subject_shape': refine it with a SubjectFitter and subjects= first")
        with torch.no_grad():
            shape = out['subject_shape'].contiguous()
            G = shape.shape[0]
            verts, joints = self.smpl.forward_arrays(shape, self._identity_rotmats(G, shape.device))
            return measurer(verts, joints)
