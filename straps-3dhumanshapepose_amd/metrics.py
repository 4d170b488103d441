"""On-device evaluation metrics: the quantities the reference's
TrainingLossesAndMetricsTracker.update_per_batch adds up per batch
(metrics/train_loss_and_metrics_tracker.py:127-213) without copying vertices to the host or running a
per-sample numpy SVD (utils/eval_utils.py:58-63)."""
import torch

from . import config, hipabi


def point_error_sums(pred, target):
    """pred, target [B,N,3] GPU fp32 -> [B,3] per-sample sums of (raw, scale+translation-corrected,
    Procrustes-aligned) point-wise L2 errors."""
    hipabi.require_gpu_tensor(pred, 'pred points', torch.float32)
    hipabi.require_gpu_tensor(target, 'target points', torch.float32)
    assert pred.shape == target.shape and pred.dim() == 3 and pred.shape[2] == 3
    p, t = pred.detach().contiguous(), target.detach().contiguous()
    out = torch.empty(p.shape[0], 3, device=p.device, dtype=torch.float32)
    hipabi.check(hipabi.lib().straps_point_metrics(hipabi.ptr(p), hipabi.ptr(t), hipabi.ptr(out), p.shape[0], p.shape[1], hipabi.stream_ptr()),
                 'straps_point_metrics')
    return out


class BatchMetrics:
    """running sums with the tracker's key names; `update` takes the same dicts as the reference's
    update_per_batch (pred_dict / target_dict with 'verts', 'joints3D', 'joints2D', 'shape_params',
    'pose_params_rot_matrices') and stays on the device -- call `summary()` once per epoch."""

    KEYS = ('pves', 'pves_sc', 'pves_pa', 'pve-ts', 'pve-ts_sc', 'mpjpes', 'mpjpes_sc', 'mpjpes_pa', 'shape_mses', 'pose_mses',
            'joints2D_l2es')

    def __init__(self, device, img_wh=config.REGRESSOR_IMG_WH):
        self.sums = torch.zeros(len(self.KEYS), device=device, dtype=torch.float64)
        self.n = 0
        self.img_wh = img_wh

    def update(self, pred_dict, target_dict, pred_reposed_vertices=None, target_reposed_vertices=None):
        v = point_error_sums(pred_dict['verts'], target_dict['verts']).double().sum(0)
        j = point_error_sums(pred_dict['joints3D'], target_dict['joints3D']).double().sum(0)
        add = torch.zeros_like(self.sums)
        add[0:3] = v
        add[5:8] = j
        if pred_reposed_vertices is not None:
            add[3:5] = point_error_sums(pred_reposed_vertices, target_reposed_vertices).double().sum(0)[:2]
        add[8] = ((pred_dict['shape_params'] - target_dict['shape_params']).double() ** 2).sum()
        add[9] = ((pred_dict['pose_params_rot_matrices'] - target_dict['pose_params_rot_matrices']).double() ** 2).sum()
        p2 = (pred_dict['joints2D'] + 1) * (self.img_wh / 2.0)          # undo_keypoint_normalisation (utils/joints2d_utils.py:5-10)
        add[10] = (p2 - target_dict['joints2D']).double().norm(dim=-1).sum()
        self.sums += add
        self.n += pred_dict['verts'].shape[0]

    def summary(self):
        """per-epoch means with the tracker's normalisers (update_per_epoch :215-251): per vertex (6890), per joint
        (14 / 17), per sample for the parameter MSE sums."""
        s = self.sums.cpu().numpy()
        n = max(self.n, 1)
        per = {'pves': 6890, 'pves_sc': 6890, 'pves_pa': 6890, 'pve-ts': 6890, 'pve-ts_sc': 6890, 'mpjpes': 14, 'mpjpes_sc': 14,
               'mpjpes_pa': 14, 'shape_mses': 10, 'pose_mses': 24 * 9, 'joints2D_l2es': 17}
        return {k: float(s[i]) / (n * per[k]) for i, k in enumerate(self.KEYS)}


def aligned_points(pred, target):
    """pred, target [B,N,3] GPU fp32 -> (sums [B,3], pred_sc [B,N,3], pred_pa [B,N,3]): point_error_sums (bit-identical) and the
    prediction after scale+translation correction and after Procrustes alignment (utils/eval_utils.py:7-85) -- what the reference's
    EvalMetricsTracker returns with return_transformed_points=True, without the host copy and the per-sample SVD loop."""
    hipabi.require_gpu_tensor(pred, 'pred points', torch.float32)
    hipabi.require_gpu_tensor(target, 'target points', torch.float32)
    if pred.shape != target.shape or pred.dim() != 3 or pred.shape[2] != 3 or pred.shape[1] < 3:
        raise RuntimeError('aligned_points: expected pred and target [B,N>=3,3], got %s and %s' % (tuple(pred.shape), tuple(target.shape)))
    p, t = pred.detach().contiguous(), target.detach().contiguous()
    sums = torch.empty(p.shape[0], 3, device=p.device, dtype=torch.float32)
    sc, pa = torch.empty_like(p), torch.empty_like(p)
    hipabi.check(hipabi.lib().straps_point_align(hipabi.ptr(p), hipabi.ptr(t), hipabi.ptr(sums), hipabi.ptr(sc), hipabi.ptr(pa), p.shape[0], p.shape[1],
                                                 hipabi.stream_ptr()), 'straps_point_align')
    return sums, sc, pa


def _byte_mask(m, name):
    if not isinstance(m, torch.Tensor) or not m.is_cuda:
        raise RuntimeError('%s must be a GPU tensor: the STRAPS hot path runs only through the HIP library (no CPU fallback)' % name)
    if m.dtype == torch.uint8:
        return m.contiguous()
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    if m.is_floating_point():
        return (m != 0).contiguous().view(torch.uint8)          # NaN != 0: foreground, as np.logical_and treats it; a comparison keeps its input's strides
    raise RuntimeError('%s must be bool, uint8 or a float type (got %s)' % (name, m.dtype))


def silhouette_counts(pred, target):
    """pred, target [B,H,W] GPU masks (bool, uint8 or a float type; non-zero is foreground) -> int32 [B,4] = true positives, false
    positives, true negatives, false negatives per frame (metrics/eval_metrics_tracker.py:158-172).  Exact integer counts."""
    if pred.shape != target.shape or pred.dim() != 3:
        raise RuntimeError('silhouette_counts: expected two [B,H,W] masks of one shape, got %s and %s' % (tuple(pred.shape), tuple(target.shape)))
    p, t = _byte_mask(pred, 'pred silhouettes'), _byte_mask(target, 'target silhouettes')
    hipabi.require_gpu_tensor(p, 'pred silhouettes')
    hipabi.require_gpu_tensor(t, 'target silhouettes')
    counts = torch.empty(p.shape[0], 4, device=p.device, dtype=torch.int32)
    hipabi.check(hipabi.lib().straps_silhouette_counts(hipabi.ptr(p), hipabi.ptr(t), hipabi.ptr(counts), p.shape[0], p.shape[1] * p.shape[2],
                                                       hipabi.stream_ptr()), 'straps_silhouette_counts')
    return counts


class EvalMetricsTracker:
    """metrics/eval_metrics_tracker.py::EvalMetricsTracker on the device: same constructor, method names, dict keys, metric names,
    divisors and file names; pred_dict / target_dict hold GPU tensors and nothing synchronises before compute_final_metrics().

    Inputs (as tracked metrics need them): 'verts', 'reposed_verts' [B,6890,3], 'joints3D' [B,14,3], 'joints2D' [B,17,2],
    'shape_params' [B,10], 'pose_params_rot_matrices' [B,24,3,3], 'silhouettes' [B,H,W] (bool, uint8 or float; non-zero = foreground).
    Running sums are float64 on the device.  Four decisions where the reference misbehaves or is ambiguous:
      * 'pve-ts_pa' works, under that key (the reference raises KeyError('pve_ts_pa'): its per-frame list key is misspelt);
      * 'pose_mses' / 'shape_mses' have no per-frame values and write no file (the reference raises in np.concatenate);
      * a frame whose union is empty has per-frame IoU NaN (0 / 0), as in the reference, without a warning; the final IoU comes from
        the summed counts;
      * 'joints2D' is compared as given: like the reference's evaluation tracker (and unlike BatchMetrics, which follows the training
        tracker) the keypoint normalisation is not undone here.
    compute_final_metrics() returns the dict the reference only prints.  Two smaller departures: a metric name outside METRICS raises
    ValueError in the constructor (the reference accepts it and fails, or silently tracks nothing, later), and compute_final_metrics()
    before any batch raises RuntimeError (the reference divides by its zero sample count)."""

    METRICS = ('pves', 'pves_sc', 'pves_pa', 'pve-ts', 'pve-ts_sc', 'pve-ts_pa', 'mpjpes', 'mpjpes_sc', 'mpjpes_pa', 'pose_mses', 'shape_mses',
               'joints2D_l2es', 'silhouette_ious')
    COUNT_KEYS = ('num_true_positives', 'num_false_positives', 'num_true_negatives', 'num_false_negatives')
    # metric family -> (dict key of the points, column of the [B,3] sums, key of the returned transformed points or None)
    _POINTS = {'pves': ('verts', 0, None), 'pves_sc': ('verts', 1, 'pred_vertices_sc'), 'pves_pa': ('verts', 2, 'pred_vertices_pa'),
               'pve-ts': ('reposed_verts', 0, None), 'pve-ts_sc': ('reposed_verts', 1, 'pred_reposed_vertices_sc'),
               'pve-ts_pa': ('reposed_verts', 2, 'pred_reposed_vertices_pa'),
               'mpjpes': ('joints3D', 0, None), 'mpjpes_sc': ('joints3D', 1, 'pred_joints3D_h36mlsp_sc'),
               'mpjpes_pa': ('joints3D', 2, 'pred_joints3D_h36mlsp_pa')}

    def __init__(self, metrics_to_track, img_wh=None, save_path=None, save_per_frame_metrics=False):
        unknown = [m for m in metrics_to_track if m not in self.METRICS]
        if unknown:
            raise ValueError('EvalMetricsTracker: unknown metrics %s (known: %s)' % (unknown, ', '.join(self.METRICS)))
        self.metrics_to_track = list(metrics_to_track)
        self.img_wh = img_wh
        self.metric_sums = None
        self.per_frame_metrics = None
        self.total_samples = 0
        self.save_per_frame_metrics = save_per_frame_metrics
        self.save_path = save_path

    def initialise_metric_sums(self):
        self.metric_sums = {}
        for metric_type in self.metrics_to_track:
            for k in (self.COUNT_KEYS if metric_type == 'silhouette_ious' else (metric_type,)):
                self.metric_sums[k] = 0.0          # becomes a float64 device scalar with the first batch

    def initialise_per_frame_metric_lists(self):
        self.per_frame_metrics = {metric_type: [] for metric_type in self.metrics_to_track}

    def _add(self, key, value):
        self.metric_sums[key] = self.metric_sums[key] + value

    @staticmethod
    def num_per_sample(metric_type):
        if 'pve' in metric_type:
            return 6890
        if 'mpjpe' in metric_type:
            return 14
        if 'joints2D' in metric_type:
            return 17
        if 'shape_mse' in metric_type:
            return 10
        if 'pose_mse' in metric_type:
            return 24 * 3 * 3
        raise KeyError(metric_type)

    @hipabi.on_tensor_device
    def update_per_batch(self, pred_dict, target_dict, num_input_samples, return_transformed_points=False):
        if self.metric_sums is None or self.per_frame_metrics is None:
            raise RuntimeError('EvalMetricsTracker: call initialise_metric_sums() and initialise_per_frame_metric_lists() first')
        self.total_samples += num_input_samples
        return_dict = {}
        tracked = self.metrics_to_track
        for key in ('verts', 'reposed_verts', 'joints3D'):          # one launch per point set serves its raw / _sc / _pa metrics
            mine = [m for m in tracked if m in self._POINTS and self._POINTS[m][0] == key]
            if not mine:
                continue
            if return_transformed_points and any(self._POINTS[m][2] for m in mine):
                sums, sc, pa = aligned_points(pred_dict[key], target_dict[key])
            else:
                sums, sc, pa = point_error_sums(pred_dict[key], target_dict[key]), None, None
            sums = sums.double()
            n = pred_dict[key].shape[1]
            for m in mine:
                _, col, out_key = self._POINTS[m]
                self._add(m, sums[:, col].sum())
                self.per_frame_metrics[m].append(sums[:, col] / n)
                if return_transformed_points and out_key:
                    return_dict[out_key] = sc if col == 1 else pa
        if 'pose_mses' in tracked:
            self._add('pose_mses', ((pred_dict['pose_params_rot_matrices'].double() - target_dict['pose_params_rot_matrices'].double()) ** 2).sum())
        if 'shape_mses' in tracked:
            self._add('shape_mses', ((pred_dict['shape_params'].double() - target_dict['shape_params'].double()) ** 2).sum())
        if 'joints2D_l2es' in tracked:
            l2 = (pred_dict['joints2D'].double() - target_dict['joints2D'].double()).norm(dim=-1)
            self._add('joints2D_l2es', l2.sum())
            self.per_frame_metrics['joints2D_l2es'].append(l2.mean(dim=-1))
        if 'silhouette_ious' in tracked:
            c = silhouette_counts(pred_dict['silhouettes'], target_dict['silhouettes']).double()
            for i, k in enumerate(self.COUNT_KEYS):
                self._add(k, c[:, i].sum())
            self.per_frame_metrics['silhouette_ious'].append(c[:, 0] / (c[:, 0] + c[:, 1] + c[:, 3]))      # 0 / 0 = NaN for an empty union
        if return_transformed_points:
            return return_dict

    def compute_final_metrics(self):
        import os
        import numpy as np
        if self.metric_sums is None or self.total_samples <= 0:
            raise RuntimeError('EvalMetricsTracker: compute_final_metrics() needs at least one update_per_batch() with samples')
        val = lambda v: float(v.item()) if isinstance(v, torch.Tensor) else float(v)
        final_metrics = {}
        for metric_type in self.metrics_to_track:
            if metric_type == 'silhouette_ious':
                tp, fp, fn = (val(self.metric_sums[k]) for k in ('num_true_positives', 'num_false_positives', 'num_false_negatives'))
                final_metrics[metric_type] = tp / (tp + fn + fp) if tp + fn + fp > 0 else float('nan')
            else:
                final_metrics[metric_type] = val(self.metric_sums[metric_type]) / (self.total_samples * self.num_per_sample(metric_type))
        if self.save_per_frame_metrics:
            for metric_type in self.metrics_to_track:
                if metric_type in ('pose_mses', 'shape_mses') or not self.per_frame_metrics[metric_type]:
                    continue
                per_frame = torch.cat(self.per_frame_metrics[metric_type], dim=0).cpu().numpy()
                np.save(os.path.join(self.save_path, metric_type + '_per_frame.npy'), per_frame)
        return final_metrics
