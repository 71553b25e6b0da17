"""Assigner and IoU calculators of the detection heads (mmdet / mmrotate task_modules), on the kernels of csrc/box_ops.hip."""
from .assign_result import AssignResult  # noqa: F401
from .iou_calculators import BboxOverlaps2D, RBbox2HBboxOverlaps2D, RBboxOverlaps2D  # noqa: F401
from .max_iou_assigner import MTP_RD_MaxIoUAssigner, MaxIoUAssigner  # noqa: F401

__all__ = ["AssignResult", "BboxOverlaps2D", "RBboxOverlaps2D", "RBbox2HBboxOverlaps2D", "MaxIoUAssigner", "MTP_RD_MaxIoUAssigner"]
