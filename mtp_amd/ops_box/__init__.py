"""MI355X-native box operators under the names the reference imports them by: mmdet's bbox_overlaps, mmcv's box_iou_rotated, nms, nms_rotated and
batched_nms (the sibling of ops_dcnv3)."""
from .functions import batched_nms, bbox_overlaps, box_iou_rotated, nms, nms_rotated  # noqa: F401

__all__ = ["bbox_overlaps", "box_iou_rotated", "nms", "nms_rotated", "batched_nms"]
