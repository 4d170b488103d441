"""Train-mode forward and backward of SingleInputRegressor through the C ABI (straps_regressor_fwd_train / straps_regressor_bwd,
include/straps_hip.h).

`flat_training_params` and `flat_bn_state` write the regressor's tensors in the flat layouts the header defines; `CompositeTrainer`
keeps them as its own buffers and runs the whole train-mode forward, and then the whole backward, as ONE library call each: the
launches the module's autograd path makes, with the same arguments, hence bit-identical estimates, gradients and running statistics,
without the per-layer Python scheduling.  The optimiser update is the host's: `straps_adam_step` over `params` / `grads` runs unchanged
(the layout is the first part of a training step's flat parameter buffer).  `write_back` copies the state into the module.
"""
import torch
import torch.nn as nn

from . import hipabi
from .ief_module import EST_LD
from .infer import N_PARAMS, regressor_desc


def flat_training_params(regressor):
    """1-D float32 tensor on the regressor's device: torch.cat([p.reshape(-1) for p in regressor.parameters()])."""
    return torch.cat([p.detach().reshape(-1).float() for p in regressor.parameters()])


def _batchnorms(regressor):
    return [m for m in regressor.modules() if isinstance(m, nn.BatchNorm2d)]


def flat_bn_state(regressor):
    """1-D float32 tensor: running_mean then running_var of every BatchNorm, in module order."""
    return torch.cat([t.detach().reshape(-1).float() for m in _batchnorms(regressor) for t in (m.running_mean, m.running_var)])


class CompositeTrainer:
    """`forward(x)` == `reg.train(); reg(x)` and `backward(dest)` == `torch.autograd.backward` of that estimate, bit for bit.

    The trainer owns copies of the parameters (`params`), of the running statistics (`bn_state`, updated by every forward) and the
    gradient buffer (`grads`, overwritten by every backward with param_grads=True).  The workspace holds the tape between a forward
    and its backward; it grows with the batch / image size and is reused.  Every call runs on the current torch stream and can be
    captured in `torch.cuda.graph` once the workspace has its size."""

    def __init__(self, regressor, precision=None):
        for m in _batchnorms(regressor):
            if m.eps != 1e-5 or m.momentum != 0.1 or not m.track_running_stats or not m.affine:
                raise NotImplementedError('CompositeTrainer: BatchNorm must have eps 1e-5, momentum 0.1, running statistics and affine parameters')
        self.precision = precision or getattr(regressor.image_encoder, 'conv_precision', 'fp32')
        if self.precision == 'bf16':
            raise RuntimeError("CompositeTrainer: conv_precision / precision 'bf16' is an inference-only route (no gradients): train on 'bf16x3' "
                               "or 'fp32'")
        self.desc = regressor_desc(regressor, self.precision)
        self.device = regressor.image_encoder.conv1.weight.device
        hipabi.require_gpu_tensor(regressor.image_encoder.conv1.weight, 'regressor parameters (call .to(device))')
        L = hipabi.lib()
        with torch.cuda.device(self.device):
            self.params = flat_training_params(regressor).contiguous()
            self.bn_state = flat_bn_state(regressor).contiguous()
            self.init_est = regressor.ief_module.initial_params_estimate.detach().float().to(self.device).contiguous()
        for name, t, n in (('parameter', self.params, L.straps_regressor_train_param_floats(self.desc)),
                           ('running-statistic', self.bn_state, L.straps_regressor_bn_state_floats(self.desc))):
            if t.numel() != n:
                raise RuntimeError('CompositeTrainer: the regressor has %d %s floats, the library expects %d' % (t.numel(), name, n))
        self.grads = torch.zeros_like(self.params)
        self.workspace = None
        self.batches_tracked = 0        # forwards since the last write_back (num_batches_tracked belongs to the host)
        self._shape = None

    def workspace_bytes(self, batch, h, w):
        return hipabi.lib().straps_regressor_train_workspace_bytes(self.desc, batch, h, w)

    @hipabi.on_tensor_device
    def forward(self, x):
        """x [B, in_channels, H, W] float32 on the trainer's GPU -> (cam [B,3], pose [B,144], shape [B,10]), views of one [B,160]
        estimate buffer like the module's.  Updates `bn_state` and records the tape the next `backward` consumes."""
        hipabi.require_gpu_tensor(x, 'CompositeTrainer input', torch.float32)
        if x.dim() != 4 or x.shape[1] != self.desc.in_channels:
            raise RuntimeError('CompositeTrainer expects [B,%d,H,W], got %s' % (self.desc.in_channels, tuple(x.shape)))
        if x.device != self.device:
            raise RuntimeError('CompositeTrainer: input on %s, parameters on %s' % (x.device, self.device))
        x = x.detach().contiguous()
        B, _, H, W = x.shape
        L = hipabi.lib()
        need = L.straps_regressor_train_workspace_bytes(self.desc, B, H, W)
        if need == 0:
            raise RuntimeError('CompositeTrainer: input %s is not supported' % (tuple(x.shape),))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, device=self.device, dtype=torch.uint8)
        est = torch.empty(B, EST_LD, device=self.device, dtype=torch.float32)      # (columns 157.. are not written)
        hipabi.check(L.straps_regressor_fwd_train(self.desc, hipabi.ptr(self.params), hipabi.ptr(self.bn_state), hipabi.ptr(self.init_est),
                                                  hipabi.ptr(x), B, H, W, hipabi.ptr(est), EST_LD, hipabi.ptr(self.workspace),
                                                  self.workspace.numel(), hipabi.stream_ptr()), 'straps_regressor_fwd_train')
        self._x = x             # (the backward reads the input: kept alive and unchanged until then)
        self._shape = (B, H, W)
        self.batches_tracked += 1
        return est[:, :3], est[:, 3:3 + 24 * 6], est[:, 3 + 24 * 6:N_PARAMS]

    __call__ = forward

    @hipabi.on_tensor_device
    def backward(self, dest, want_dx=False, param_grads=True):
        """dest: gradient w.r.t. the estimate of the last forward, [B, >= 157] (columns 157.. are not read).  Returns (grads, dx):
        the flat parameter gradients (`grads`, overwritten; None with param_grads=False) and the NCHW input gradient (None unless
        want_dx)."""
        if self._shape is None:
            raise RuntimeError('CompositeTrainer.backward: no forward to differentiate')
        hipabi.require_gpu_tensor(dest, 'CompositeTrainer dest', torch.float32)
        B, H, W = self._shape
        if dest.dim() != 2 or dest.shape[0] != B or dest.shape[1] < N_PARAMS:
            raise RuntimeError('CompositeTrainer.backward: dest must be [%d, >= %d], got %s' % (B, N_PARAMS, tuple(dest.shape)))
        if dest.stride(1) != 1:
            dest = dest.contiguous()
        dx = torch.empty_like(self._x) if want_dx else None
        g = self.grads if param_grads else None
        L = hipabi.lib()
        hipabi.check(L.straps_regressor_bwd(self.desc, hipabi.ptr(self.params), hipabi.ptr(self._x), B, H, W, hipabi.ptr(dest), dest.stride(0),
                                            hipabi.ptr(g), hipabi.ptr(dx), hipabi.ptr(self.workspace), self.workspace.numel(), hipabi.stream_ptr()),
                     'straps_regressor_bwd')
        return g, dx

    @torch.no_grad()
    def write_back(self, regressor):
        """copy the parameters and running statistics into the module, and add the forwards since the last write_back to every
        BatchNorm's num_batches_tracked."""
        off = 0
        for p in regressor.parameters():
            n = p.numel()
            p.copy_(self.params[off:off + n].view_as(p))
            off += n
        off = 0
        for m in _batchnorms(regressor):
            for t in (m.running_mean, m.running_var):
                n = t.numel()
                t.copy_(self.bn_state[off:off + n].view_as(t))
                off += n
            m.num_batches_tracked.add_(self.batches_tracked)
        self.batches_tracked = 0
        return regressor

    def export_infer_params(self):
        """the straps_regressor_param_floats() buffer of the current state (what straps_regressor_prepare takes)."""
        L = hipabi.lib()
        out = torch.empty(L.straps_regressor_param_floats(self.desc), device=self.device, dtype=torch.float32)
        hipabi.check(L.straps_regressor_export_infer_params(self.desc, hipabi.ptr(self.params), hipabi.ptr(self.bn_state), hipabi.ptr(self.init_est),
                                                            hipabi.ptr(out), hipabi.stream_ptr()), 'straps_regressor_export_infer_params')
        return out
