"""The IoU calculators the reference's train_cfg dicts name: BboxOverlaps2D (mask_rcnn.py:72-99), RBboxOverlaps2D and MTP_RD_RBbox2HBboxOverlaps2D
(oriented_rcnn.py:85,107; rotated_detection/max_iou_assigner.py:20-80).  Each is callable like the reference's; `kind` names the fused assignment's
calculator (mtp_amd.ops.ASSIGN_CALCULATOR)."""
import torch

from ..ops_box import bbox_overlaps, box_iou_rotated
from ..registry import TASK_UTILS


def box_tensor(b):
    """a plain tensor, or a box object holding one in .tensor (mmdet's HorizontalBoxes, mmrotate's RotatedBoxes)"""
    return b.tensor if hasattr(b, "tensor") and not isinstance(b, torch.Tensor) else b


def rbox2hbox(r):
    """(n, 5) cx, cy, w, h, theta -> (n, 4) the circumscribed x1, y1, x2, y2 (mmrotate's RotatedBoxes.convert_to('hbox'))"""
    hw, hh, c, s = r[:, 2] * 0.5, r[:, 3] * 0.5, torch.cos(r[:, 4]), torch.sin(r[:, 4])
    ex, ey = (hw * c).abs() + (hh * s).abs(), (hw * s).abs() + (hh * c).abs()
    return torch.stack([r[:, 0] - ex, r[:, 1] - ey, r[:, 0] + ex, r[:, 1] + ey], 1)


class _Calculator:
    kind = None
    cols = (4, 4)      # box columns of bboxes1 / bboxes2; one more (a score) is cut off

    def __init__(self, scale=1., dtype=None):
        if dtype == "fp16":
            raise NotImplementedError("%s: dtype='fp16' is not built (the kernels compute in float32 and hold no K x N matrix to shrink)" % type(self).__name__)
        if dtype is not None:
            raise ValueError("%s: dtype must be None, got %r" % (type(self).__name__, dtype))
        self.scale, self.dtype = scale, dtype

    def boxes(self, bboxes1, bboxes2):
        out = []
        for b, c in zip((bboxes1, bboxes2), self.cols):
            b = box_tensor(b)
            if b.shape[-1] not in (0, c, c + 1):
                raise ValueError("%s: boxes of %d columns, expected %d (or %d with a score)" % (type(self).__name__, b.shape[-1], c, c + 1))
            out.append(b[..., :c] if b.shape[-1] == c + 1 else b.reshape(-1, c))
        return out

    def __repr__(self):
        return "%s(scale=%s, dtype=%s)" % (type(self).__name__, self.scale, self.dtype)


@TASK_UTILS.register_module()
class BboxOverlaps2D(_Calculator):
    kind = "box"

    def __call__(self, bboxes1, bboxes2, mode="iou", is_aligned=False):
        b1, b2 = self.boxes(bboxes1, bboxes2)
        return bbox_overlaps(b1, b2, mode, is_aligned)


@TASK_UTILS.register_module()
class RBboxOverlaps2D(_Calculator):
    kind = "rotated"
    cols = (5, 5)

    def __call__(self, bboxes1, bboxes2, mode="iou", is_aligned=False):
        b1, b2 = self.boxes(bboxes1, bboxes2)
        return box_iou_rotated(b1, b2, mode, is_aligned)


@TASK_UTILS.register_module(name=["RBbox2HBboxOverlaps2D", "MTP_RD_RBbox2HBboxOverlaps2D"])
class RBbox2HBboxOverlaps2D(_Calculator):
    """rotated bboxes1 -> their circumscribed boxes, then box / box overlaps with bboxes2"""
    kind = "rbox2hbox"
    cols = (5, 4)

    def __call__(self, bboxes1, bboxes2, mode="iou", is_aligned=False):
        b1, b2 = self.boxes(bboxes1, bboxes2)
        return bbox_overlaps(rbox2hbox(b1.to(torch.float32)), b2, mode, is_aligned)
