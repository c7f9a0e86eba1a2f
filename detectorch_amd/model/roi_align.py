"""RoIAlign -- same call surface as the reference's lib/model/roi_align.py (RoIAlignFunction :23, RoIAlign :150,
preprocess_rois :172), backed by the hand-written gfx950 kernels (forward: detectorch_amd/csrc/roi_align.hip; backward:
detectorch_amd/csrc/grad/roi_align_backward.hip) instead of the torch-0.4 JIT / torch-0.3 cffi CUDA extensions the reference
selects at :8-20.

Differences a caller can observe:
  * GPU only: CPU tensors raise (the reference's CPU branch :67-83 is what oracle/ restates as the checker);
  * features may be NCHW-contiguous or channels_last, float32, float16 or bfloat16;
  * backward (the reference's :93-145) gives the gradient with respect to the features only, as the reference does: the bits of
    the reference's serial CPU loop, the same on every run (no atomics).  The native gradient is float32 NCHW; for 16-bit or
    channels_last features it is cast back to their dtype and layout with torch ops.  With no input requiring grad nothing is
    saved and backward is never called;
  * roi_align_fpn / RoIAlignFPNFunction: the multi-level form (one launch forward, one call backward for all levels), which the
    reference does not have -- it pools level by level.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.module import Module

from .. import hip, hip_grad


def _like_features(grad, features_dtype, channels_last):
    """The native float32 NCHW gradient in the dtype and layout of the feature map it belongs to."""
    if channels_last:
        return grad.to(dtype=features_dtype, memory_format=torch.channels_last)
    return grad.to(dtype=features_dtype)


def _is_channels_last(t):
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


class RoIAlignFunction(Function):
    @staticmethod
    def forward(ctx, features, rois, pooled_height, pooled_width, spatial_scale, sampling_ratio):
        # reference: roi_align.py:33-89
        if features.is_cuda != rois.is_cuda:
            raise TypeError('features and rois should be on same device (CPU or GPU)')   # :43-44
        ctx.rois = rois                                    # :35-40
        ctx.features_size = features.size()
        ctx.pooled_height = int(pooled_height)
        ctx.pooled_width = int(pooled_width)
        ctx.spatial_scale = float(spatial_scale)
        ctx.sampling_ratio = int(sampling_ratio)
        ctx.features_dtype, ctx.channels_last = features.dtype, _is_channels_last(features)
        return hip.roi_align_forward(features, float(spatial_scale), rois, int(pooled_height), int(pooled_width),
                                     int(sampling_ratio))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        # reference: roi_align.py:93-145
        rois = ctx.rois.detach().contiguous()
        if ctx.features_size[0] == 1 and rois.dim() == 2 and rois.shape[1] == 5:
            rois = rois[:, 1:].contiguous()                # one image: the batch column can only hold 0 (as the forward call)
        grad_input, = hip_grad.roi_align_backward(grad_output.contiguous().float(), rois, tuple(ctx.features_size), ctx.spatial_scale,
                                                  ctx.pooled_height, ctx.pooled_width, ctx.sampling_ratio)
        return _like_features(grad_input, ctx.features_dtype, ctx.channels_last), None, None, None, None, None


class RoIAlignFPNFunction(Function):
    """RoIAlign over several levels: RoI r pools from features[roi_levels[r]].  forward: hip.roi_align_forward (one launch);
    backward: hip_grad.roi_align_backward (one call), a gradient for every level that requires one."""

    @staticmethod
    def forward(ctx, spatial_scales, rois, roi_levels, pooled_height, pooled_width, sampling_ratio, *features):
        ctx.rois, ctx.roi_levels = rois, roi_levels
        ctx.spatial_scales = [float(s) for s in spatial_scales]
        ctx.pooled_height, ctx.pooled_width, ctx.sampling_ratio = int(pooled_height), int(pooled_width), int(sampling_ratio)
        ctx.features_sizes = [tuple(f.size()) for f in features]
        ctx.features_dtype, ctx.channels_last = features[0].dtype, [_is_channels_last(f) for f in features]
        return hip.roi_align_forward(list(features), ctx.spatial_scales, rois, ctx.pooled_height, ctx.pooled_width, ctx.sampling_ratio,
                                     roi_levels=roi_levels)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        levels = None if ctx.roi_levels is None else ctx.roi_levels.detach().to(torch.int32).contiguous()
        grads = hip_grad.roi_align_backward(grad_output.contiguous().float(), ctx.rois.detach().contiguous(), ctx.features_sizes,
                                            ctx.spatial_scales, ctx.pooled_height, ctx.pooled_width, ctx.sampling_ratio,
                                            roi_levels=levels)
        grads = [_like_features(g, ctx.features_dtype, cl) if need else None
                 for g, cl, need in zip(grads, ctx.channels_last, ctx.needs_input_grad[6:])]
        return (None,) * 6 + tuple(grads)


def roi_align_fpn(features, spatial_scales, rois, roi_levels, pooled_height, pooled_width, sampling_ratio=0):
    """features: list of [B,C,H_l,W_l] maps (equal B, C and dtype); rois float32 [R,5]; roi_levels int32 [R] (None: level 0).
    -> [R,C,pooled_height,pooled_width] float32, differentiable with respect to every map."""
    return RoIAlignFPNFunction.apply(tuple(spatial_scales), preprocess_rois(rois), roi_levels, pooled_height, pooled_width,
                                     sampling_ratio, *features)


class RoIAlign(Module):
    def __init__(self, pooled_height, pooled_width, spatial_scale, sampling_ratio=0):
        super(RoIAlign, self).__init__()
        self.pooled_height = int(pooled_height)
        self.pooled_width = int(pooled_width)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)

    def forward(self, features, rois):
        rois = preprocess_rois(rois)
        return RoIAlignFunction.apply(features, rois, self.pooled_height, self.pooled_width, self.spatial_scale,
                                      self.sampling_ratio)


def preprocess_rois(rois):
    """reference: roi_align.py:172-187 -- list -> cat; [1,R,k] -> [R,k]; 4 columns -> prepend a zero batch column."""
    if isinstance(rois, list):
        rois = torch.cat(tuple(rois), 0)
    if torch.is_tensor(rois):
        if rois.dim() == 3:
            if rois.size(0) == 1:
                rois = rois.squeeze(0)
            else:
                raise ValueError("rois has wrong size")
        if rois.size(1) == 4:
            zeros = torch.zeros((rois.size(0), 1), dtype=rois.dtype, device=rois.device)
            rois = torch.cat((zeros, rois), 1).contiguous()
    return rois
