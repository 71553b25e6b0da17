"""mmdet's SingleRoIExtractor (mask_rcnn.py:58-62 and 94-98): every RoI is pooled from the one level its scale maps to.  The reference loops over the
levels with nonzero(); here the level is worked out inside the one RoIAlign launch that serves all RoIs and all levels."""
import torch
import torch.nn as nn

from .. import ops
from ..ops_roi import RoIAlign
from ..registry import MODELS


@MODELS.register_module(name=["SingleRoIExtractor", "mmdet.SingleRoIExtractor"])
class SingleRoIExtractor(nn.Module):
    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56, init_cfg=None):
        super().__init__()
        cfg = dict(roi_layer)
        kind = str(cfg.pop("type", "RoIAlign"))
        if kind.split(".")[-1] != "RoIAlign":
            raise NotImplementedError("SingleRoIExtractor: roi_layer %r is not built (RoIAlign is)" % kind)
        cfg.pop("spatial_scale", None)
        self.roi_layers = nn.ModuleList([RoIAlign(spatial_scale=1.0 / s, **cfg) for s in featmap_strides])
        if not 1 <= len(self.roi_layers) <= ops.ROI_MAX_LEVELS:
            raise ValueError("SingleRoIExtractor: 1 .. %d levels" % ops.ROI_MAX_LEVELS)
        self.out_channels, self.featmap_strides, self.finest_scale = int(out_channels), [int(s) for s in featmap_strides], float(finest_scale)

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def map_roi_levels(self, rois, num_levels):
        """rois (R, 5) -> (R) int64: floor(log2(sqrt((x2 - x1)(y2 - y1)) / finest_scale + 1e-6)) clamped to the levels (what the kernel computes)"""
        scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
        return torch.floor(torch.log2(scale / self.finest_scale + 1e-6)).clamp(min=0, max=num_levels - 1).long()

    def geometry(self):
        l0 = self.roi_layers[0]
        return dict(out_size=l0.output_size, sampling_ratio=l0.sampling_ratio, aligned=l0.aligned, finest_scale=self.finest_scale)

    def extract(self, maps, sizes, images, rois, roi_levels=None, valid=None, out=None, levels_out=None):
        """maps: per level an ops.rpn_map_nchw / rpn_map_rows triple of out_channels channels -> (R, output_size^2, out_channels) f32, channel last"""
        return ops.roi_align_fwd(maps, sizes, [l.spatial_scale for l in self.roi_layers], self.out_channels, images, rois, roi_levels=roi_levels,
                                 valid=valid, out=out, levels_out=levels_out, **self.geometry())

    def extract_bwd(self, dout, dmaps, sizes, images, rois, roi_levels=None, valid=None, accumulate=False):
        """every pixel of every level's gradient map is stored (accumulate: added to)"""
        return ops.roi_align_bwd(dout, dmaps, sizes, [l.spatial_scale for l in self.roi_layers], self.out_channels, images, rois,
                                 roi_levels=roi_levels, valid=valid, accumulate=accumulate, **self.geometry())

    @torch.no_grad()
    def forward(self, feats, rois, roi_scale_factor=None):
        """feats: one NCHW map per level, rois (R, 5) -> (R, out_channels, output_size, output_size) f32.  No autograd graph: training goes through
        the head's loss_and_grads (a single level with a graph: mtp_amd.ops_roi.RoIAlign)."""
        if roi_scale_factor is not None:
            raise NotImplementedError("SingleRoIExtractor: roi_scale_factor is not built (no MTP configuration sets it)")
        feats = list(feats)
        if len(feats) != self.num_inputs or any(f.dim() != 4 or f.shape[1] != self.out_channels for f in feats):
            raise ValueError("SingleRoIExtractor: expected %d NCHW maps of %d channels" % (self.num_inputs, self.out_channels))
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError("SingleRoIExtractor: rois (R, 5) = image, x1, y1, x2, y2")
        P, R = self.roi_layers[0].output_size, rois.shape[0]
        if R == 0:
            return feats[0].new_zeros((0, self.out_channels, P, P), dtype=torch.float32)
        maps = [ops.rpn_map_nchw(f.detach().to(torch.float32).contiguous()) for f in feats]
        sizes = [(int(f.shape[2]), int(f.shape[3])) for f in feats]
        out = self.extract(maps, sizes, int(feats[0].shape[0]), rois.detach().to(torch.float32).contiguous())
        return out.permute(0, 2, 1).reshape(R, self.out_channels, P, P)
