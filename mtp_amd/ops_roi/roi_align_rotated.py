"""RoIAlignRotated (mmcv.ops.roi_align_rotated; the roi_layer of oriented_rcnn.py:45-49) on mtp_amd.ops.roi_align_rotated_fwd / _bwd.  The kernels
write (R, bins, C), channel last; this module hands out mmcv's (R, C, out_h, out_w) and takes its gradient in that layout.  The backward is
deterministic (entries, a stable sort, one owner per pixel) and there is no gradient to the RoIs, as in mmcv."""
import torch
import torch.nn as nn

from .. import ops
from ..registry import MODELS


class _RoIAlignRotatedFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rois, out_size, spatial_scale, sample_num, clockwise):
        x32 = x.detach().to(torch.float32).contiguous()
        r32 = rois.detach().to(torch.float32).contiguous()
        N, Cc, H, W = x32.shape
        R = r32.shape[0]
        ctx.geom = (N, Cc, H, W, out_size, float(spatial_scale), sample_num, bool(clockwise), x.dtype)
        ctx.save_for_backward(r32)
        if R == 0:
            return x.new_zeros((0, Cc, out_size, out_size))
        out = ops.roi_align_rotated_fwd([ops.rpn_map_nchw(x32)], [(H, W)], [spatial_scale], Cc, N, r32, out_size, sample_num, clockwise)
        return out.permute(0, 2, 1).reshape(R, Cc, out_size, out_size).to(x.dtype)

    @staticmethod
    def backward(ctx, dout):
        (r32,) = ctx.saved_tensors
        N, Cc, H, W, P, scale, S, clockwise, dtype = ctx.geom
        dx = torch.zeros(N, Cc, H, W, device=dout.device, dtype=torch.float32)
        if r32.shape[0]:
            d = dout.detach().to(torch.float32).reshape(-1, Cc, P * P).permute(0, 2, 1).contiguous()
            ops.roi_align_rotated_bwd(d, [ops.rpn_map_nchw(dx)], [(H, W)], [scale], Cc, N, r32, P, S, clockwise)
        return dx.to(dtype), None, None, None, None, None


def roi_align_rotated(x, rois, out_size, spatial_scale, sample_num=2, aligned=True, clockwise=False):
    if not aligned:
        raise NotImplementedError("roi_align_rotated: aligned=False is not built (no MTP configuration asks for it)")
    if sample_num <= 0:
        raise NotImplementedError("roi_align_rotated: sample_num <= 0 (the adaptive grid) is not built (no MTP configuration asks for it)")
    if x.dim() != 4 or rois.dim() != 2 or rois.shape[1] != 6:
        raise ValueError("roi_align_rotated: x (N, C, H, W) and rois (R, 6) = image, cx, cy, w, h, theta")
    return _RoIAlignRotatedFunction.apply(x, rois, int(out_size), float(spatial_scale), int(sample_num), bool(clockwise))


@MODELS.register_module(name=["RoIAlignRotated", "mmcv.RoIAlignRotated"])
class RoIAlignRotated(nn.Module):
    """RoIAlignRotated(out_size | output_size, spatial_scale, sample_num | sampling_ratio, aligned=True, clockwise=False): square outputs,
    sample_num > 0, aligned only."""

    def __init__(self, out_size=None, spatial_scale=1.0, sample_num=None, aligned=True, clockwise=False, output_size=None, sampling_ratio=None):
        super().__init__()
        size = output_size if out_size is None else out_size
        num = sampling_ratio if sample_num is None else sample_num
        if size is None:
            raise TypeError("RoIAlignRotated: out_size (or output_size) is needed")
        if isinstance(size, (tuple, list)):
            if len(size) != 2 or size[0] != size[1]:
                raise NotImplementedError("RoIAlignRotated: only square outputs are built")
            size = size[0]
        num = 2 if num is None else int(num)
        if num <= 0:
            raise NotImplementedError("RoIAlignRotated: sample_num <= 0 (the adaptive grid) is not built (no MTP configuration asks for it)")
        if not aligned:
            raise NotImplementedError("RoIAlignRotated: aligned=False is not built (no MTP configuration asks for it)")
        if size < 1 or size * size * num * num > ops.ROI_MAX_POINTS:
            raise ValueError("RoIAlignRotated: out_size^2 * sample_num^2 must lie in 1 .. %d" % ops.ROI_MAX_POINTS)
        self.out_size = self.output_size = int(size)
        self.spatial_scale, self.sample_num, self.aligned, self.clockwise = float(spatial_scale), num, True, bool(clockwise)
        self.sampling_ratio = num

    def forward(self, input, rois):
        return roi_align_rotated(input, rois, self.out_size, self.spatial_scale, self.sample_num, True, self.clockwise)

    def extra_repr(self):
        return "out_size=%d, spatial_scale=%g, sample_num=%d, aligned=True, clockwise=%s" % (self.out_size, self.spatial_scale, self.sample_num, self.clockwise)
