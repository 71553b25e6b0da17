"""Assigner, IoU calculators, anchor generator, box coder and sampler of the detection heads (mmdet / mmrotate task_modules), on the kernels of
csrc/box_ops.hip, csrc/rpn.hip, csrc/roi_head.hip and csrc/hbox_head.hip."""
from .anchor_generator import AnchorGenerator  # noqa: F401
from .assign_result import AssignResult  # noqa: F401
from .delta_xywh_coder import DeltaXYWHBBoxCoder  # noqa: F401
from .delta_xywht_coder import DeltaXYWHTRBBoxCoder  # noqa: F401
from .iou_calculators import BboxOverlaps2D, RBbox2HBboxOverlaps2D, RBboxOverlaps2D  # noqa: F401
from .max_iou_assigner import MTP_RD_MaxIoUAssigner, MaxIoUAssigner  # noqa: F401
from .midpoint_offset_coder import MidpointOffsetCoder  # noqa: F401
from .random_sampler import RandomSampler, SampleList  # noqa: F401

__all__ = ["AssignResult", "BboxOverlaps2D", "RBboxOverlaps2D", "RBbox2HBboxOverlaps2D", "MaxIoUAssigner", "MTP_RD_MaxIoUAssigner",
           "AnchorGenerator", "MidpointOffsetCoder", "DeltaXYWHTRBBoxCoder", "DeltaXYWHBBoxCoder", "RandomSampler", "SampleList"]
