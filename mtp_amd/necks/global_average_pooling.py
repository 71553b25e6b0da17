"""GlobalAveragePooling (mmpretrain's neck between the backbone and the classification head; every reference scene-classification config sets
`neck=dict(type='GlobalAveragePooling')`).

mmpretrain is not part of the reference tree, so this restates the class from its published behaviour: `nn.AdaptiveAvgPool2d((1, 1))` on each map and
a flatten to (N, C); a tuple in gives a tuple out, a tensor a tensor.  Here the pooling is an autograd function over mtp_gap_fwd / mtp_gap_bwd: the
pooled vectors are f32 whatever the map's dtype, the gradient comes back in the map's dtype.
"""
import torch
import torch.nn as nn

from .. import ops
from ..registry import MODELS


class _GapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape, ctx.dtype = x.shape, x.dtype
        return ops.gap_fwd(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        dx = ops._scratch(tuple(ctx.shape), g.device, ctx.dtype)
        return ops.gap_bwd(g.contiguous(), dx)


def global_average_pool(x):
    """(N, C, H, W) f32 / bf16 -> (N, C) f32, differentiable"""
    if x.dim() != 4:
        raise ValueError("GlobalAveragePooling: expected an NCHW map, got shape %s" % (tuple(x.shape),))
    return _GapFn.apply(x)


@MODELS.register_module()
class GlobalAveragePooling(nn.Module):
    """GlobalAveragePooling(dim=2).  No parameters."""

    def __init__(self, dim=2):
        super().__init__()
        if dim not in (1, 2, 3):
            raise ValueError("GlobalAveragePooling: dim must be 1, 2 or 3, got %r" % (dim,))
        if dim != 2:
            raise NotImplementedError("GlobalAveragePooling: dim=%d is not implemented (2: the NCHW maps of every MTP config)" % dim)
        self.dim = dim

    def init_weights(self):
        pass

    def forward(self, inputs):
        if isinstance(inputs, (tuple, list)):
            return tuple(global_average_pool(x) for x in inputs)
        if torch.is_tensor(inputs):
            return global_average_pool(inputs)
        raise TypeError("neck inputs should be tuple or torch.tensor")
