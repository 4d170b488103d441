"""The validation half of the reference's epoch (train/train_synthetic_otf_rendering.py:242-363) on the device.

  ValStep        one validation batch (:251-348): target rotations / meshes / 2-D joints at the MEAN camera, the part rasteriser without
                 vertex noise, the crop without jitter, the proxy input without augmentation, the regressor in eval mode, SMPL on the
                 prediction, and straps_val_head -- the five task losses and the tracker's eleven metric sums, forward only, added to a
                 24-double accumulator that lives on the device.  A whole pass costs one device-to-host copy (`summary()`).
  EpochHistory   the part of metrics/train_loss_and_metrics_tracker.py that decides things: the history dict under the reference's key
                 names, its pickle, and the rule that picks the epoch whose weights become `best_model_state_dict` (:267-273).

No random number is drawn and no parameter, BatchNorm buffer or optimiser state is touched: a ValStep between two training steps
leaves them bit for bit what they would have been without it.
"""
import ctypes as C
import pickle

import numpy as np
import torch

from . import config, hipabi
from .metrics import BatchMetrics
from .multi_task_loss import TASKS

ACC_SLOTS = 24      # straps_val_head's accumulator: total, 5 weighted task losses, 5 raw MSEs (each x batch), visible joints, 11 metric sums, samples
# the tracker's normalisers (update_per_epoch :232-251)
PER_SAMPLE = {'pves': 6890, 'pves_sc': 6890, 'pves_pa': 6890, 'pve-ts': 6890, 'pve-ts_sc': 6890, 'mpjpes': 14, 'mpjpes_sc': 14, 'mpjpes_pa': 14,
              'shape_mses': 10, 'pose_mses': 24 * 9, 'joints2D_l2es': 17}


def summarise(acc):
    """the accumulator of straps_val_head (24 doubles, host) -> the dict `ValStep.summary()` returns: 'losses' and the five
    '<task>_losses' per sample (loss_metric_sums / num_samples, :216-230), the eleven metrics of BatchMetrics.KEYS over
    num_samples x the tracker's per-sample count, 'num_samples'.  Pure host arithmetic."""
    acc = np.asarray(acc, np.float64).reshape(-1)
    if acc.shape[0] != ACC_SLOTS:
        raise ValueError('summarise: expected the %d accumulator slots of straps_val_head, got %d' % (ACC_SLOTS, acc.shape[0]))
    n = float(acc[23])
    if not n > 0:
        raise RuntimeError('summarise: the accumulator holds no sample (run at least one whole batch first)')
    out = {'losses': float(acc[0]) / n}
    for k, task in enumerate(TASKS):
        out[task + '_losses'] = float(acc[1 + k]) / n
    for k, key in enumerate(BatchMetrics.KEYS):
        out[key] = float(acc[12 + k]) / (n * PER_SAMPLE[key])
    out['num_samples'] = int(n)
    return out


class ValStep:
    """ValStep(regressor, smpl, criterion, batch_size)(pose_aa [B,72], shape [B,10]) -> the 12-float loss record of the batch (device
    tensor, no synchronisation; the layout of straps_loss_fwd_bwd's loss_out).  `reset()` / `summary()` / `run(pose_pool, shape_pool)`
    drive a whole pass.  bbox_augment_params: the dictionary of run_train.py:150-153 -- only 'crop_input' and 'mean_scale_factor' matter
    here (validation crops without jitter, :276-283)."""

    def __init__(self, regressor, smpl, criterion, batch_size, mean_cam_t=(0., 0.2, 42.), bbox_augment_params=None, renderer=None,
                 img_wh=config.REGRESSOR_IMG_WH):
        p0 = next(regressor.parameters())
        if not (isinstance(p0, torch.Tensor) and p0.is_cuda):
            raise RuntimeError('ValStep: regressor parameters must be GPU tensors (call .to(device) first): the STRAPS hot path runs only '
                               'through the HIP library (no CPU fallback)')
        if getattr(criterion, 'reduction', 'mean') != 'mean':
            raise NotImplementedError("ValStep: straps_val_head implements reduction='mean' (run_train.py:196)")
        if int(batch_size) < 1:
            raise ValueError('ValStep: batch_size must be positive (got %r)' % (batch_size,))
        self.reg, self.smpl, self.crit = regressor, smpl, criterion
        self.dev, self.B, self.img_wh = p0.device, int(batch_size), int(img_wh)
        from .train_step import BBOX_AUGMENT_PARAMS
        self.bbox_augment_params = dict(BBOX_AUGMENT_PARAMS if bbox_augment_params is None else bbox_augment_params)
        d, B, wh = self.dev, self.B, self.img_wh
        with torch.cuda.device(d):
            L = hipabi.lib()
            self.mean_cam_t = torch.tensor(mean_cam_t, dtype=torch.float32, device=d).expand(B, 3).contiguous()
            self._eye = torch.eye(3, device=d).expand(B, 24, 3, 3).contiguous()        # rest pose of the 'reposed' SMPL passes
            if renderer is None:
                if smpl.faces is None or smpl.face_parts is None:
                    raise RuntimeError('ValStep: the SMPL model carries no faces / face_parts; pass renderer=NMRRenderer(...)')
                from .nmr_renderer import NMRRenderer
                K = torch.tensor([[config.FOCAL_LENGTH, 0., wh / 2.0], [0., config.FOCAL_LENGTH, wh / 2.0], [0., 0., 1.]])
                renderer = NMRRenderer(B, K, torch.eye(3), wh, rend_parts_seg=True, faces=smpl.faces, face_parts=smpl.face_parts).to(d)
            self.renderer = renderer
            f32 = lambda *s: torch.empty(*s, device=d, dtype=torch.float32)
            crop = bool(self.bbox_augment_params['crop_input'])
            # every buffer of the step, once
            self.buf = dict(rot=f32(B, 24, 3, 3), verts=f32(B, 6890, 3), joints=f32(B, 90, 3), reposed=f32(B, 6890, 3),
                            joints2d_uncropped=f32(B, 17, 2), joints3d=f32(B, 14, 3), seg=f32(B, wh, wh),
                            seg_cropped=f32(B, wh, wh) if crop else None, joints2d=f32(B, 17, 2) if crop else None,
                            input=f32(B, 18, wh, wh), pred_rot=f32(B, 24, 3, 3), pred_shape=f32(B, 10), pred_verts=f32(B, 6890, 3),
                            pred_joints=f32(B, 90, 3), pred_reposed=f32(B, 6890, 3), loss=f32(12), per_sample=f32(B, len(BatchMetrics.KEYS)))
            self._ws = torch.empty((L.straps_val_head_workspace_bytes(B) + 7) // 8, device=d, dtype=torch.float64)
            self.acc = torch.zeros(ACC_SLOTS, device=d, dtype=torch.float64)

    # ------------------------------------------------------------------ one batch
    def _forward_eval(self, x):
        """regressor.eval()(x) under no_grad through the module's own forward, the previous mode restored; -> (cam, pose, shape)"""
        reg = self.reg
        modes = [(m, m.training) for m in reg.modules()]
        reg.eval()
        try:
            for m in reg.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training:
                    raise RuntimeError('ValStep: %s stays in training mode after regressor.eval(): the forward would update its running statistics'
                                       % type(m).__name__)
            with torch.no_grad():
                return reg(x)
        finally:
            for m, t in modes:
                m.training = t

    @staticmethod
    def _estimate_buffer(cam, pose, shape):
        """the regressor returns three views of one [B, ld] estimate buffer (ief_module.py); the head reads that buffer as it is"""
        ld = cam.stride(0)
        if not (cam.stride() == (ld, 1) and pose.stride() == (ld, 1) and shape.stride() == (ld, 1) and ld >= 157
                and pose.data_ptr() == cam.data_ptr() + 4 * 3 and shape.data_ptr() == cam.data_ptr() + 4 * 147):
            raise RuntimeError('ValStep: the regressor\'s (cam, pose, shape) are not the three views of one estimate buffer that IEFModule.forward returns')
        return cam, ld

    def step(self, pose_aa, shape, keep=None):
        with torch.cuda.device(self.dev), torch.no_grad():
            return self._step(pose_aa, shape, keep)

    __call__ = step

    def _step(self, pose_aa, shape, keep):
        L, st, B, wh, buf = hipabi.lib(), hipabi.stream_ptr(), self.B, self.img_wh, self.buf
        P = hipabi.ptr
        hipabi.require_gpu_tensor(pose_aa, 'pose_aa', torch.float32)
        hipabi.require_gpu_tensor(shape, 'shape', torch.float32)
        if pose_aa.dim() != 2 or pose_aa.shape[1] != 72 or shape.dim() != 2 or shape.shape[1] != 10 or shape.shape[0] != pose_aa.shape[0]:
            raise ValueError('ValStep: expected pose_aa [B,72] and shape [B,10], got %s and %s' % (tuple(pose_aa.shape), tuple(shape.shape)))
        if pose_aa.shape[0] != B:
            raise ValueError('ValStep: whole batches only (drop_last=True in the reference): got %d samples, batch_size is %d' % (pose_aa.shape[0], B))
        pose_aa, shape = pose_aa.contiguous(), shape.contiguous()
        # 1. target rotations (batch_rodrigues, :322)
        hipabi.check(L.straps_rodrigues_fwd(P(pose_aa), P(buf['rot']), B * 24, st), 'straps_rodrigues_fwd')
        # 2. posed and reposed target meshes (:258-270)
        self.smpl.forward_arrays(shape, buf['rot'], out_verts=buf['verts'], out_joints=buf['joints'])
        self.smpl.forward_arrays(shape, self._eye, want_joints=False, out_verts=buf['reposed'])
        # 3. H36M-LSP joints + perspective projection of the COCO joints at the MEAN camera translation (:263-268)
        hipabi.check(L.straps_project_targets(P(buf['joints']), P(self.mean_cam_t), config.FOCAL_LENGTH, config.FOCAL_LENGTH, wh / 2.0, wh / 2.0,
                                              P(buf['joints2d_uncropped']), P(buf['joints3d']), B, st), 'straps_project_targets')
        # 4. part segmentation, no vertex noise (:273)
        seg = self.renderer.render_arrays(buf['verts'], self.mean_cam_t, out=buf['seg'])
        # 5. bounding-box crop at mean_scale_factor, no jitter (:276-288)
        bp = self.bbox_augment_params
        if bp['crop_input']:
            from .image_utils import batch_crop_and_resize
            seg_c, j2d, boxes = batch_crop_and_resize(seg, buf['joints2d_uncropped'], wh, bp['mean_scale_factor'], None, None,
                                                      out=buf['seg_cropped'], jout=buf['joints2d'])
        else:
            seg_c, j2d, boxes = seg, buf['joints2d_uncropped'], None
        # 6. proxy input: binary silhouette + joint heat-maps, nothing removed, occluded or jittered (:291-295)
        x = buf['input']
        hipabi.check(L.straps_build_proxy_input(P(seg_c), P(j2d), P(x), B, 17, wh, st), 'straps_build_proxy_input')
        # 7. eval-mode forward (:298)
        cam, pose, pshape = self._forward_eval(x)
        est, ld = self._estimate_buffer(cam, pose, pshape)
        # 8. rot6d + SMPL on the prediction (:300-318)
        hipabi.check(L.straps_rot6d_fwd(C.c_void_p(est.data_ptr() + 4 * 3), ld, 24, P(buf['pred_rot']), B, st), 'straps_rot6d_fwd')
        hipabi.check(L.straps_masked_copy(C.c_void_p(est.data_ptr() + 4 * 147), ld, None, 0, P(buf['pred_shape']), 10, B, 10, 0, st), 'pred_shape')
        self.smpl.forward_arrays(buf['pred_shape'], buf['pred_rot'], out_verts=buf['pred_verts'], out_joints=buf['pred_joints'])
        self.smpl.forward_arrays(buf['pred_shape'], self._eye, want_joints=False, out_verts=buf['pred_reposed'])
        # 9. heads, losses and metric sums into the accumulator (:320-348, tracker :118-213)
        lv = self.crit.log_var_vector()
        hipabi.check(L.straps_val_head(P(buf['pred_verts']), P(buf['pred_reposed']), P(buf['pred_joints']), P(est), ld, P(buf['pred_rot']),
                                       P(buf['verts']), P(buf['reposed']), P(j2d), P(buf['joints3d']), P(shape), P(buf['rot']), P(lv),
                                       P(buf['loss']), P(buf['per_sample']), P(self.acc), P(self._ws), B, 6890, wh, st), 'straps_val_head')
        if keep is not None:
            keep.update(rot=buf['rot'], verts=buf['verts'], joints=buf['joints'], reposed=buf['reposed'], joints2d_uncropped=buf['joints2d_uncropped'],
                        joints3d=buf['joints3d'], seg=seg, seg_cropped=seg_c, boxes=boxes, joints2d=j2d, input=x, cam=cam, pose=pose, pred_shape_view=pshape,
                        est=est, ld_est=ld, pred_rot=buf['pred_rot'], pred_shape=buf['pred_shape'], pred_verts=buf['pred_verts'],
                        pred_joints=buf['pred_joints'], pred_reposed=buf['pred_reposed'], shape=shape, log_vars=lv, loss=buf['loss'],
                        per_sample=buf['per_sample'])
        return buf['loss']

    # ------------------------------------------------------------------ a whole pass
    def reset(self):
        """zero the accumulator (start of a validation pass)"""
        with torch.cuda.device(self.dev):
            hipabi.check(hipabi.lib().straps_memset_zero(hipabi.ptr(self.acc), ACC_SLOTS * 8, hipabi.stream_ptr()), 'straps_memset_zero(accumulator)')

    def summary(self):
        """one device-to-host copy of the accumulator -> `summarise()`'s dict"""
        return summarise(self.acc.cpu().numpy())

    def run(self, pose_pool, shape_pool):
        """a validation pass over two resident tensors [N,72] / [N,10]: N // batch_size whole batches in order, the remainder dropped like
        the reference's drop_last=True -> summary()"""
        if pose_pool.shape[0] != shape_pool.shape[0]:
            raise ValueError('ValStep.run: %d poses and %d shapes' % (pose_pool.shape[0], shape_pool.shape[0]))
        if pose_pool.shape[0] < self.B:
            raise ValueError('ValStep.run: %d samples hold no whole batch of %d' % (pose_pool.shape[0], self.B))
        self.reset()
        for k in range(pose_pool.shape[0] // self.B):
            self.step(pose_pool[k * self.B:(k + 1) * self.B], shape_pool[k * self.B:(k + 1) * self.B])
        return self.summary()


class EpochHistory:
    """metrics/train_loss_and_metrics_tracker.py without the per-batch arithmetic (that is straps_val_head's and the training step's):
    the `history` dict under the reference's key names, one value per epoch and key (0.0 for what is not tracked or not supplied),
    pickled to `log_path` after every epoch in the reference's format, and the rule that decides whether this epoch's weights become
    the best ones.  load_logs=True continues an existing log up to `current_epoch`, like the reference's constructor (:40-41, :52-90)."""

    TASKS = ('verts', 'shape_params', 'pose_params', 'joints2D', 'joints3D')
    METRICS = ('pves', 'pves_sc', 'pves_pa', 'pve-ts', 'pve-ts_sc', 'pve-ts_pa', 'mpjpes', 'mpjpes_sc', 'mpjpes_pa', 'pose_mses', 'shape_mses',
               'joints2D_l2es')

    def __init__(self, losses_to_track, metrics_to_track, log_path=None, load_logs=False, current_epoch=None):
        unknown = [m for m in metrics_to_track if m not in self.METRICS] + [t for t in losses_to_track if t not in self.TASKS]
        if unknown:
            raise ValueError('EpochHistory: unknown losses / metrics %s' % unknown)
        self.losses_to_track, self.metrics_to_track, self.log_path = list(losses_to_track), list(metrics_to_track), log_path
        self.all_per_task_loss_types = [s + '_' + t + '_losses' for t in self.TASKS for s in ('train', 'val')]
        self.all_metrics_types = [s + '_' + m for m in self.METRICS for s in ('train', 'val')]
        if load_logs:
            self.history = self.load_history(log_path, current_epoch)
        else:
            self.history = {k: [] for k in ['train_losses', 'val_losses'] + self.all_per_task_loss_types + self.all_metrics_types}

    def load_history(self, load_log_path, current_epoch):
        """:52-90: every list cut to `current_epoch` entries; lists the file lacks are filled with zeros"""
        with open(load_log_path, 'rb') as f:
            history = pickle.load(f)
        for k in ['train_losses', 'val_losses'] + self.all_per_task_loss_types + self.all_metrics_types:
            history[k] = list(history[k][:current_epoch]) if k in history else [0.0] * current_epoch
        for k, v in history.items():
            if len(v) != current_epoch:
                raise ValueError('EpochHistory: %d elements in %s of %s when the current epoch is %d' % (len(v), k, load_log_path, current_epoch))
        return history

    def update_per_epoch(self, train_summary, val_summary):
        """append one epoch: the summaries are `ValStep.summary()`-style dicts ('losses', '<task>_losses', metric names; a TrainStep's
        metrics_summary() serves as a train summary without losses); None or a missing key gives 0.0, as does anything not tracked.
        Then the history is pickled to log_path (:263-265)."""
        for split, s in (('train', train_summary), ('val', val_summary)):
            s = s or {}
            self.history[split + '_losses'].append(float(s.get('losses', 0.0)))
            for t in self.TASKS:
                self.history['%s_%s_losses' % (split, t)].append(float(s.get(t + '_losses', 0.0)) if t in self.losses_to_track else 0.0)
            for m in self.METRICS:
                self.history[split + '_' + m].append(float(s.get(m, 0.0)) if m in self.metrics_to_track else 0.0)
        if self.log_path is not None:
            with open(self.log_path, 'wb') as f:
                pickle.dump(self.history, f)

    def determine_save_model_weights_this_epoch(self, save_val_metrics, best_epoch_val_metrics):
        """:267-273: save unless some tracked validation metric of the last epoch is strictly greater than its best"""
        for metric in save_val_metrics:
            if self.history['val_' + metric][-1] > best_epoch_val_metrics[metric]:
                return False
        return True

    @staticmethod
    def checkpoint_dict(epoch, regressor, optimiser, criterion, best_epoch, best_epoch_val_metrics, best_model_wts):
        """the seven-key dict of :369-375 (checkpoint_utils.CHECKPOINT_KEYS); `optimiser`: a torch optimiser or a TrainStep"""
        from .checkpoint_utils import save_checkpoint
        return save_checkpoint(None, epoch, regressor, optimiser, criterion, best_epoch=best_epoch, best_epoch_val_metrics=best_epoch_val_metrics,
                               best_model_wts=best_model_wts)
