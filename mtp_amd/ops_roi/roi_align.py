"""RoIAlign (mmcv.ops.roi_align; the roi_layer of mask_rcnn.py: output_size=14, sampling_ratio=0) on mtp_amd.ops.roi_align_fwd / _bwd.  The kernels
write (R, bins, C), channel last; this module hands out mmcv's (R, C, out_h, out_w) and takes its gradient in that layout.  The backward is
deterministic (a gather per map pixel over the RoIs in index order) and there is no gradient to the RoIs, as in mmcv."""
import torch
import torch.nn as nn

from .. import ops
from ..registry import MODELS


class _RoIAlignFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rois, out_size, spatial_scale, sampling_ratio, aligned):
        x32 = x.detach().to(torch.float32).contiguous()
        r32 = rois.detach().to(torch.float32).contiguous()
        N, Cc, H, W = x32.shape
        R = r32.shape[0]
        ctx.geom = (N, Cc, H, W, out_size, float(spatial_scale), sampling_ratio, bool(aligned), x.dtype)
        ctx.save_for_backward(r32)
        if R == 0:
            return x.new_zeros((0, Cc, out_size, out_size))
        out = ops.roi_align_fwd([ops.rpn_map_nchw(x32)], [(H, W)], [spatial_scale], Cc, N, r32, out_size, sampling_ratio, aligned)
        return out.permute(0, 2, 1).reshape(R, Cc, out_size, out_size).to(x.dtype)

    @staticmethod
    def backward(ctx, dout):
        (r32,) = ctx.saved_tensors
        N, Cc, H, W, P, scale, sampling, aligned, dtype = ctx.geom
        if r32.shape[0] == 0:
            return torch.zeros(N, Cc, H, W, device=dout.device, dtype=dtype), None, None, None, None, None
        dx = torch.empty(N, Cc, H, W, device=dout.device, dtype=torch.float32)      # the kernel stores every pixel
        d = dout.detach().to(torch.float32).reshape(-1, Cc, P * P).permute(0, 2, 1).contiguous()
        ops.roi_align_bwd(d, [ops.rpn_map_nchw(dx)], [(H, W)], [scale], Cc, N, r32, P, sampling, aligned)
        return dx.to(dtype), None, None, None, None, None


def _square(size, who):
    if isinstance(size, (tuple, list)):
        if len(size) != 2 or size[0] != size[1]:
            raise NotImplementedError("%s: only square outputs are built" % who)
        size = size[0]
    return int(size)


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode="avg", aligned=True):
    """mmcv.ops.roi_align: input (N, C, H, W), rois (R, 5) = image, x1, y1, x2, y2 -> (R, C, output_size, output_size)"""
    if pool_mode != "avg":
        raise NotImplementedError("roi_align: pool_mode %r is not built ('avg' is; no MTP configuration asks for 'max')" % (pool_mode,))
    size = _square(output_size, "roi_align")
    if not 1 <= size <= ops.ROI_ALIGN_MAX_OUT or not 0 <= int(sampling_ratio) <= ops.ROI_ALIGN_MAX_SAMPLING:
        raise ValueError("roi_align: output_size in 1 .. %d, sampling_ratio in 0 .. %d" % (ops.ROI_ALIGN_MAX_OUT, ops.ROI_ALIGN_MAX_SAMPLING))
    if input.dim() != 4 or rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError("roi_align: input (N, C, H, W) and rois (R, 5) = image, x1, y1, x2, y2")
    return _RoIAlignFunction.apply(input, rois, size, float(spatial_scale), int(sampling_ratio), bool(aligned))


@MODELS.register_module(name=["RoIAlign", "mmcv.RoIAlign"])
class RoIAlign(nn.Module):
    """RoIAlign(output_size, spatial_scale, sampling_ratio=0, pool_mode='avg', aligned=True): square outputs up to 32, 'avg' only;
    sampling_ratio 0 is the adaptive grid every MTP configuration uses."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode="avg", aligned=True, use_torchvision=False):
        super().__init__()
        if pool_mode != "avg":
            raise NotImplementedError("RoIAlign: pool_mode %r is not built ('avg' is; no MTP configuration asks for 'max')" % (pool_mode,))
        if use_torchvision:
            raise NotImplementedError("RoIAlign: use_torchvision is not built")
        size = _square(output_size, "RoIAlign")
        if not 1 <= size <= ops.ROI_ALIGN_MAX_OUT or not 0 <= int(sampling_ratio) <= ops.ROI_ALIGN_MAX_SAMPLING:
            raise ValueError("RoIAlign: output_size in 1 .. %d, sampling_ratio in 0 .. %d" % (ops.ROI_ALIGN_MAX_OUT, ops.ROI_ALIGN_MAX_SAMPLING))
        self.output_size = self.out_size = size
        self.spatial_scale, self.sampling_ratio, self.pool_mode, self.aligned = float(spatial_scale), int(sampling_ratio), "avg", bool(aligned)

    def forward(self, input, rois):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, self.pool_mode, self.aligned)

    def extra_repr(self):
        return "output_size=%d, spatial_scale=%g, sampling_ratio=%d, pool_mode=avg, aligned=%s" % (self.output_size, self.spatial_scale, self.sampling_ratio,
                                                                                                   self.aligned)
