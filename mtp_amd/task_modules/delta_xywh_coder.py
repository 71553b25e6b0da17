"""mmdet's DeltaXYWHBBoxCoder as mask_rcnn.py:25-28, 43-46 configures it (clip_border, no centre clamp), on the __device__ functions of
csrc/hbox_head.hip through their stand-alone launches (mtp_amd.ops.hbox_delta_encode / hbox_delta_decode).  The definition is restated from the
published mmdet 3.x algorithm, bbox2delta / delta2bbox."""
import torch

from .. import ops
from ..registry import TASK_UTILS
from .iou_calculators import box_tensor


@TASK_UTILS.register_module(name=["DeltaXYWHBBoxCoder", "mmdet.DeltaXYWHBBoxCoder"])
class DeltaXYWHBBoxCoder:
    encode_size = 4

    def __init__(self, target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.), clip_border=True, add_ctr_clamp=False, ctr_clamp=32,
                 use_box_type=False, **kwargs):
        me = "DeltaXYWHBBoxCoder"
        if not clip_border:
            raise NotImplementedError("%s: clip_border=False is not built (the MTP configs clip to the image)" % me)
        if add_ctr_clamp:
            raise NotImplementedError("%s: add_ctr_clamp=True is not built" % me)
        if use_box_type:
            raise NotImplementedError("%s: use_box_type=True is not built (boxes are plain (n, 4) tensors)" % me)
        if kwargs:
            raise TypeError("%s: unknown arguments %s" % (me, sorted(kwargs)))
        self.means, self.stds = tuple(float(v) for v in target_means), tuple(float(v) for v in target_stds)
        if len(self.means) != 4 or len(self.stds) != 4 or min(self.stds) <= 0:
            raise ValueError("%s: 4 target_means and 4 positive target_stds" % me)
        self.clip_border, self.add_ctr_clamp, self.ctr_clamp, self.use_box_type = True, False, ctr_clamp, False

    @staticmethod
    def _f32(t):
        return box_tensor(t).detach().to(torch.float32).contiguous()

    def encode(self, bboxes, gt_bboxes):
        """bboxes (n, 4), gt_bboxes (n, 4), both x1 y1 x2 y2 -> deltas (n, 4)"""
        p, g = self._f32(bboxes), self._f32(gt_bboxes)
        if p.dim() != 2 or p.shape[1] != 4 or g.shape != p.shape:
            raise ValueError("DeltaXYWHBBoxCoder.encode: bboxes (n, 4) and gt_bboxes (n, 4)")
        if p.shape[0] == 0:
            return p.new_zeros((0, 4))
        return ops.hbox_delta_encode(p, g, self.means, self.stds)

    @staticmethod
    def shape_table(pairs, device):
        """[(h, w), ...] (or any per-image pairs) -> the (images, 2) f32 device table the kernels index by image; built per call: a few bytes"""
        return torch.tensor([(float(a), float(b)) for a, b in pairs], dtype=torch.float32, device=device).reshape(-1, 2)

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        """bboxes (n, 4), pred_bboxes (n, 4) deltas -> boxes (n, 4); max_shape (h, w): x clipped to [0, w], y to [0, h]"""
        p, d = self._f32(bboxes), self._f32(pred_bboxes)
        if p.dim() != 2 or p.shape[1] != 4 or d.shape != p.shape:
            raise ValueError("DeltaXYWHBBoxCoder.decode: bboxes (n, 4) and pred_bboxes (n, 4)")
        if p.shape[0] == 0:
            return p.new_zeros((0, 4))
        table = None if max_shape is None else self.shape_table([tuple(max_shape)[:2]], p.device)
        return ops.hbox_delta_decode(p, d, self.means, self.stds, table, None, wh_ratio_clip)
