"""One-call inference of SingleInputRegressor through the C ABI (straps_regressor_*, include/straps_hip.h).

`flat_inference_params` writes the regressor's tensors in the flat layout the header defines; `InferenceRegressor` prepares them
once (folded BatchNorm, packed weights) and runs the whole eval-mode forward as ONE library call: the same launches, with the same
arguments, as `SingleInputRegressor.eval()`, hence bit-identical outputs, without the per-layer Python scheduling.  Inference only:
no gradients, BatchNorm on its running statistics.  The module and its own forward are left untouched.
"""
import torch
import torch.nn as nn

from . import hipabi
from .ief_module import EST_LD

PRECISIONS = {'bf16x3': 0, 'fp32': 1, 'bf16': 3}      # (2 is unassigned; 'bf16' = single-product bf16 convolutions, inference only)
N_PARAMS = 3 + 24 * 6 + 10


def flat_inference_params(regressor):
    """1-D float32 tensor on the regressor's device: every state_dict() tensor in its order, without `num_batches_tracked` and the
    `ief_module.ief_layers.*` aliases, then the IEF's initial estimate (157 floats)."""
    parts = [v.detach().reshape(-1).float() for k, v in regressor.state_dict().items()
             if not k.endswith('num_batches_tracked') and '.ief_layers.' not in k]
    dev = parts[0].device
    parts.append(regressor.ief_module.initial_params_estimate.detach().reshape(-1).float().to(dev))
    return torch.cat(parts)


def regressor_desc(regressor, precision=None):
    enc = regressor.image_encoder
    precision = precision or getattr(enc, 'conv_precision', 'fp32')
    if precision not in PRECISIONS:
        raise ValueError("precision must be 'bf16x3', 'fp32' or 'bf16' (got %r)" % (precision,))
    layers = 18 if enc.kind == 'basic' else 50
    return hipabi.RegressorDesc(layers, enc.in_channels, regressor.ief_module.iterations, PRECISIONS[precision])


class InferenceRegressor:
    """`InferenceRegressor(reg)(x)` == `reg.eval()(x)` bit for bit, for a float32 NCHW GPU input.

    The prepared buffer holds the weights and running statistics as they were at construction or at the last `refresh()`: after an
    optimiser step or a `load_state_dict`, call `refresh()`.  The workspace grows with the batch / image size and is reused.  Every
    call runs on the current torch stream and can be captured in `torch.cuda.graph`."""

    def __init__(self, regressor, precision=None):
        for m in regressor.modules():
            if isinstance(m, nn.BatchNorm2d) and m.eps != 1e-5:
                raise NotImplementedError('InferenceRegressor: BatchNorm eps must be 1e-5 (got %g)' % m.eps)
        self.regressor = regressor
        self.precision = precision or getattr(regressor.image_encoder, 'conv_precision', 'fp32')
        self.desc = regressor_desc(regressor, self.precision)
        self.device = regressor.image_encoder.conv1.weight.device
        self.prepared = None
        self.workspace = None
        self.refresh()

    def refresh(self):
        """re-prepare from the module's current weights and running statistics (synchronises the current stream)."""
        L = hipabi.lib()
        dref = self.desc
        hipabi.require_gpu_tensor(self.regressor.image_encoder.conv1.weight, 'regressor parameters (call .to(device))')
        with torch.cuda.device(self.device):
            params = flat_inference_params(self.regressor).contiguous()
            n = L.straps_regressor_param_floats(dref)
            if params.numel() != n:
                raise RuntimeError('InferenceRegressor: the regressor has %d inference floats, the library expects %d' % (params.numel(), n))
            if self.prepared is None:
                self.prepared = torch.empty(L.straps_regressor_prepared_bytes(dref), device=self.device, dtype=torch.uint8)
            hipabi.check(L.straps_regressor_prepare(dref, hipabi.ptr(params), hipabi.ptr(self.prepared), hipabi.stream_ptr()),
                         'straps_regressor_prepare')
        return self

    def workspace_bytes(self, batch, h, w):
        return hipabi.lib().straps_regressor_workspace_bytes(self.desc, batch, h, w)

    @hipabi.on_tensor_device
    def __call__(self, x, rotmats=False):
        """x [B, in_channels, H, W] float32 on the regressor's GPU -> (cam [B,3], pose [B,144], shape [B,10]) -- views of one [B,160]
        estimate buffer, like the module's -- plus the rotation matrices [B*24, 3, 3] with rotmats=True."""
        hipabi.require_gpu_tensor(x, 'InferenceRegressor input', torch.float32)
        if x.dim() != 4 or x.shape[1] != self.desc.in_channels:
            raise RuntimeError('InferenceRegressor expects [B,%d,H,W], got %s' % (self.desc.in_channels, tuple(x.shape)))
        if x.device != self.device:
            raise RuntimeError('InferenceRegressor: input on %s, regressor on %s' % (x.device, self.device))
        x = x.contiguous()
        B, _, H, W = x.shape
        L = hipabi.lib()
        need = L.straps_regressor_workspace_bytes(self.desc, B, H, W)
        if need == 0:
            raise RuntimeError('InferenceRegressor: input %s is not supported' % (tuple(x.shape),))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, device=self.device, dtype=torch.uint8)
        est = torch.empty(B, EST_LD, device=self.device, dtype=torch.float32)      # (columns 157.. are not written)
        rot = torch.empty(B * 24, 3, 3, device=self.device, dtype=torch.float32) if rotmats else None
        hipabi.check(L.straps_regressor_fwd_infer(self.desc, hipabi.ptr(self.prepared), hipabi.ptr(x), B, H, W, hipabi.ptr(est), EST_LD,
                                                  hipabi.ptr(rot), hipabi.ptr(self.workspace), self.workspace.numel(), hipabi.stream_ptr()),
                     'straps_regressor_fwd_infer')
        out = (est[:, :3], est[:, 3:3 + 24 * 6], est[:, 3 + 24 * 6:N_PARAMS])
        return out + (rot,) if rotmats else out
