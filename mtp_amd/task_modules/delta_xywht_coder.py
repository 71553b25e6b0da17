"""mmrotate's DeltaXYWHTRBBoxCoder as oriented_rcnn.py:58-66 configures it (angle_version 'le90', norm_factor None, edge_swap, proj_xy), on the
__device__ functions of csrc/roi_head.hip through their stand-alone launches (mtp_amd.ops.rbox_delta_encode / rbox_delta_decode).  The definition is
restated from the published algorithm."""
import torch

from .. import ops
from ..registry import TASK_UTILS
from .iou_calculators import box_tensor


@TASK_UTILS.register_module(name=["DeltaXYWHTRBBoxCoder", "mmrotate.DeltaXYWHTRBBoxCoder"])
class DeltaXYWHTRBBoxCoder:
    encode_size = 5

    def __init__(self, target_means=(0., 0., 0., 0., 0.), target_stds=(1., 1., 1., 1., 1.), angle_version="le90", norm_factor=None, edge_swap=True,
                 proj_xy=True, add_ctr_clamp=False, ctr_clamp=32, use_box_type=False, **kwargs):
        me = "DeltaXYWHTRBBoxCoder"
        if angle_version != "le90":
            raise NotImplementedError("%s: angle_version %r is not built ('le90' is what the MTP configs use)" % (me, angle_version))
        if norm_factor is not None:
            raise NotImplementedError("%s: norm_factor is not built (the MTP configs set None)" % me)
        if not edge_swap or not proj_xy:
            raise NotImplementedError("%s: edge_swap=False and proj_xy=False are not built (the MTP configs set both)" % me)
        if add_ctr_clamp:
            raise NotImplementedError("%s: add_ctr_clamp is not built" % me)
        if kwargs:
            raise TypeError("%s: unknown arguments %s" % (me, sorted(kwargs)))
        self.means, self.stds = tuple(float(v) for v in target_means), tuple(float(v) for v in target_stds)
        if len(self.means) != 5 or len(self.stds) != 5 or min(self.stds) <= 0:
            raise ValueError("%s: 5 target_means and 5 positive target_stds" % me)
        self.angle_version, self.norm_factor, self.edge_swap, self.proj_xy = angle_version, None, True, True

    @staticmethod
    def _f32(t):
        return box_tensor(t).detach().to(torch.float32).contiguous()

    def encode(self, bboxes, gt_bboxes):
        """bboxes (n, 5), gt_bboxes (n, 5), both cx cy w h theta -> deltas (n, 5)"""
        p, g = self._f32(bboxes), self._f32(gt_bboxes)
        if p.dim() != 2 or p.shape[1] != 5 or g.shape != p.shape:
            raise ValueError("DeltaXYWHTRBBoxCoder.encode: bboxes (n, 5) and gt_bboxes (n, 5)")
        if p.shape[0] == 0:
            return p.new_zeros((0, 5))
        return ops.rbox_delta_encode(p, g, self.means, self.stds)

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        """bboxes (n, 5), pred_bboxes (n, 5) deltas -> rotated boxes (n, 5), w >= h, theta in [-pi/2, pi/2).  max_shape is accepted: rotated boxes
        are not clipped."""
        if abs(wh_ratio_clip - 16 / 1000) > 1e-12:
            raise NotImplementedError("DeltaXYWHTRBBoxCoder.decode: wh_ratio_clip other than 16 / 1000 is not built")
        p, d = self._f32(bboxes), self._f32(pred_bboxes)
        if p.dim() != 2 or p.shape[1] != 5 or d.shape != p.shape:
            raise ValueError("DeltaXYWHTRBBoxCoder.decode: bboxes (n, 5) and pred_bboxes (n, 5)")
        if p.shape[0] == 0:
            return p.new_zeros((0, 5))
        return ops.rbox_delta_decode(p, d, self.means, self.stds)
