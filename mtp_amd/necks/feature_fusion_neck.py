"""FeatureFusionNeck (open-cd's neck between the siamese backbone passes and the decode head; every reference change-detection config sets
`neck=dict(type='FeatureFusionNeck', policy='abs_diff', out_indices=(0, 1, 2, 3))`).

open-cd is not part of the reference tree, so this restates the class from open-cd's published behaviour: the two feature tuples are fused level by
level with `policy` -- 'concat' (channels of x1 then x2), 'sum', 'diff' (x2 - x1), 'abs_diff' (|x1 - x2|) -- and the levels in `out_indices` are
returned.  Here the fusion is an autograd function over mtp_fuse_pair_fwd / _bwd (NCHW in, NCHW out).  It is the module surface and the inference
path; training takes the fast path that fuses inside the head (UNetHead.loss_and_grads(fusion=...)) and never builds the fused NCHW maps.
"""
import torch
import torch.nn as nn

from .. import ops
from ..registry import MODELS


def fuse_rows(f, policy, dtype=None):
    """f (2N, C, H, W), 'from' samples first -> the fused pairs as channels-last rows (N*H*W, C -- 2C for 'concat')"""
    B, C, H, W = f.shape
    out = torch.empty(B // 2 * H * W, 2 * C if policy == "concat" else C, device=f.device, dtype=dtype or f.dtype)
    return ops.fuse_pair_fwd(f.contiguous(), out, policy)


class _FuseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, policy):
        B, C, H, W = f.shape
        f = f.contiguous()
        rows = fuse_rows(f, policy)
        ctx.save_for_backward(f)
        ctx.policy = policy
        out = torch.empty(B // 2, rows.shape[1], H, W, device=f.device, dtype=f.dtype)
        return ops.tokens_to_nchw(rows, out, B // 2, H, W, 0)

    @staticmethod
    def backward(ctx, dout):
        f, = ctx.saved_tensors
        N, Cf, H, W = dout.shape
        g = ops.nchw_to_tokens(dout.contiguous(), torch.empty(N * H * W, Cf, device=dout.device, dtype=torch.float32), N, H, W, 0)
        df = ops.fuse_pair_bwd(g, f, torch.empty(f.shape, device=f.device, dtype=torch.float32), ctx.policy)
        return df.to(f.dtype), None


def fuse_pair(x1, x2, policy):
    """one level: x1, x2 (N, C, H, W) f32 / bf16 -> (N, C | 2C, H, W), differentiable"""
    if x1.shape != x2.shape:
        raise ValueError("FeatureFusionNeck: the two inputs' shapes differ: %s / %s" % (tuple(x1.shape), tuple(x2.shape)))
    return _FuseFn.apply(torch.cat([x1, x2], 0), policy)


@MODELS.register_module()
class FeatureFusionNeck(nn.Module):
    """FeatureFusionNeck(policy, in_channels=None, channels=None, out_indices=(0, 1, 2, 3)); forward(x1, x2) on tuples of NCHW maps"""

    def __init__(self, policy, in_channels=None, channels=None, out_indices=(0, 1, 2, 3), init_cfg=None):
        super().__init__()
        ops.fuse_policy(policy)          # ValueError on an unknown policy
        self.policy, self.in_channels, self.channels = policy, in_channels, channels
        self.out_indices = tuple(int(i) for i in out_indices)

    @staticmethod
    def fusion(x1, x2, policy):
        return fuse_pair(x1, x2, policy)

    def forward(self, x1, x2):
        if len(x1) != len(x2):
            raise ValueError("FeatureFusionNeck: the two inputs have %d and %d levels" % (len(x1), len(x2)))
        outs = [fuse_pair(a, b, self.policy) for a, b in zip(x1, x2)]
        return tuple(outs[i] for i in self.out_indices)

    def forward_batch(self, feats):
        """the same on the backbone's maps of the 2N-batch cat([img_from, img_to]) (no split and re-concatenation)"""
        outs = [_FuseFn.apply(f, self.policy) for f in feats]
        return tuple(outs[i] for i in self.out_indices)
